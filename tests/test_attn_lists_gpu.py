"""Block lists in the attention kernels (csrc/attn_hd.hip, csrc/attn_f32.hip with ``kl_ptr`` / ``kl_idx`` / ``ql_ptr`` /
``ql_idx``; BigBird): forward and dQ follow each query block's list of 64-key blocks, dK / dV its transpose, and a block
listed n times counts n times.

Method: an fp64 reference of the dense definition (multiplicity x exp(score), written here), the per-ROW error of
tests/attn_refs.py ``row_err`` for o / dq / dk / dv beside the whole-tensor rel-L2, and for bf16 the torch-bf16 floor —
the same dense computation carried out by torch in bf16 on the same inputs.  Bounds are those of
tests/test_attn_global_gpu.py (bf16: 2e-2 on the output, 3e-2 on the gradients; fp32: 2e-6 / 2e-5), held per row for
bf16 unless 1.5 x the floor's own row error is larger, and for fp32 per row at the suite's fp32 row bound 1e-5
(tests/rowwise_refs.py ROW_BOUND).  A spy asserts which binding ran and that it got the tables.  Beyond parity: the
full list is the list-free call bit for bit, unlisted blocks are skipped and not masked, an empty list and an unlisted
key block give exact zeros, and what the binding and the routing refuse."""
import numpy as np
import pytest
import torch

import attn_refs as R
from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.models.bigbird import bigbird_plan
from distributed_llms_example_amd.ops import attention as A
from distributed_llms_example_amd.ops import routing
from distributed_llms_example_amd.ops.rng import attention_keep_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
_NAMES = ("attn_fwd", "attn_bwd", "attn_hd_fwd", "attn_hd_bwd", "attn_f32_fwd", "attn_f32_bwd")
_TABLES = ("kl_ptr", "kl_idx", "ql_ptr", "ql_idx")


@pytest.fixture
def calls(monkeypatch):
    """The attention bindings that ran, as (name, the four tables or None)."""
    out = []
    real = _ext.native()

    class Spy:
        def __getattr__(self, n):
            f = getattr(real, n)
            if n not in _NAMES:
                return f

            def g(*a, **kw):
                out.append((n, tuple(kw.get(t) for t in _TABLES) if kw.get("kl_ptr") is not None else None))
                return f(*a, **kw)
            return g

    monkeypatch.setattr(A._ext, "native", lambda: Spy())
    return out


def _assert_calls(calls, names, heads, nq, nk):
    assert [c[0] for c in calls] == list(names), calls
    for _, t in calls:
        assert t is not None and all(x.dtype == torch.int32 and x.is_cuda for x in t)
        assert t[0].shape == (heads, nq + 1) and t[2].shape == (heads, nk + 1) and t[1].shape == t[3].shape


def _random_lists(heads, nq, nk, seed):
    """Per head and query block 1 .. 6 key blocks drawn WITH replacement (so repeats), in drawn order; query block 1 of
    head 0 lists a block three times."""
    rs = np.random.RandomState(seed)
    kl = [[rs.randint(0, nk, size=rs.randint(1, 7)).tolist() for _ in range(nq)] for _ in range(heads)]
    kl[0][1] = [2, 0, 2, 2]
    return kl


def _counts(bl, Sq, Sk):
    m = torch.from_numpy(bl.counts()).to(DEV)
    return m.repeat_interleave(bl.block, 1)[:, :Sq].repeat_interleave(bl.block, 2)[:, :, :Sk]


def _dense(q, k, v, lut, mask, cnt, p, seed, scale, dtype):
    """The dense definition in ``dtype`` (fp64: the reference; bf16: the torch-bf16 floor): softmax over score +
    log(multiplicity), hidden where the multiplicity is 0 or the key is padding; a row that sees nothing gives 0."""
    B, Sq, H, _ = q.shape
    Sk = k.shape[1]
    qf, kf, vf = (t.to(dtype).permute(0, 2, 1, 3) for t in (q, k, v))
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if lut is not None:
        rel = torch.arange(Sk, device=DEV)[None, :] - torch.arange(Sq, device=DEV)[:, None] + (Sq - 1)
        s = s + lut.to(dtype)[:, rel].unsqueeze(0)
    see = (cnt > 0)[None].expand(B, H, Sq, Sk) if cnt.shape[0] == H else (cnt > 0)[None].expand(B, 1, Sq, Sk)
    if mask is not None:
        see = see & mask.bool()[:, None, None, :]
    s = s + torch.log(cnt.clamp_min(1).to(dtype))[None]
    s = s.masked_fill(~see, float("-inf"))
    live = see.any(-1, keepdim=True)
    pr = torch.softmax(torch.where(live, s, torch.zeros_like(s)), dim=-1) * live.to(dtype)
    if p > 0.0:
        pr = pr * attention_keep_mask(seed, p, B, H, Sq, Sk, DEV).to(dtype) * (1.0 / (1.0 - p))
    return torch.matmul(pr, vf).permute(0, 2, 1, 3)


def _grads(fn, q, k, v, lut, g, dtype):
    ins = [t.detach().to(dtype).requires_grad_(True) for t in (q, k, v)]
    # the bias LUT stays fp32 below fp64 (the kernels take it so; the bf16 floor rounds it inside _dense)
    ldt = torch.float64 if dtype == torch.float64 else torch.float32
    lt = lut.detach().to(ldt).requires_grad_(True) if lut is not None else None
    o = fn(ins[0], ins[1], ins[2], lt)
    gr = torch.autograd.grad(o, ins + ([lt] if lt is not None else []), g.to(o.dtype))
    return (o.detach(),) + tuple(gr) + ((None,) if lt is None else ())


def _inputs(B, S, H, D, dtype, seed, bias=True, pad_from=None):
    torch.manual_seed(seed)
    q, k, v = (torch.randn(B, S, H, D, device=DEV).to(dtype) for _ in range(3))
    lut = torch.randn(H, 2 * S - 1, device=DEV) * 0.5 if bias else None
    mask = None
    if pad_from is not None:
        mask = torch.ones(B, S, dtype=torch.bool, device=DEV)
        mask[1, pad_from:] = False
    g = torch.randn(B, S, H, D, device=DEV).to(dtype)
    return q, k, v, lut, mask, g


def _native(q, k, v, lut, mask, bl, p, seed, scale, g):
    return _grads(lambda a, b, c, lt: A.attention(a, b, c, scale=scale, key_padding_mask=mask, bias_lut=lt,
                                                  dropout_p=p, seed=seed, block_lists=bl), q, k, v, lut, g, q.dtype)


def _check(tag, dtype, got, ref, floor=None):
    """Prints every figure, then asserts them together."""
    bad = []
    for i, n in enumerate(("o", "dq", "dk", "dv", "dlut")):
        if got[i] is None:
            continue
        l2 = R.rel_l2(got[i], ref[i])
        if n == "dlut":
            bound = 3e-2 if dtype == BF16 else 2e-5
            print(f"[fig] {tag} {n}: rel-L2 {l2:.3e} bound {bound:.1e}")
            if not l2 <= bound:
                bad.append((n, l2, bound))
            continue
        row = R.row_err(got[i], ref[i])
        if dtype == BF16:
            base = 2e-2 if n == "o" else 3e-2
            frow = R.row_err(floor[i], ref[i])
            rb = max(base, 1.5 * frow)
            print(f"[fig] {tag} {n}: rel-L2 {l2:.3e} bound {base:.1e}; row {row:.3e} torch-bf16 floor {frow:.3e} "
                  f"bound {rb:.2e}")
        else:
            base, rb = (2e-6 if n == "o" else 2e-5), 1e-5
            print(f"[fig] {tag} {n}: rel-L2 {l2:.3e} bound {base:.1e}; row {row:.3e} bound {rb:.1e}")
        if not l2 <= base:
            bad.append((n, "rel-L2", l2, base))
        if not row <= rb:
            bad.append((n, "row", row, rb))
    assert not bad, (tag, bad)


def _parity(tag, calls, dtype, D, kl, S, H, p, pad_from, seed, B=2, scale=None):
    scale = D ** -0.5 if scale is None else scale
    q, k, v, lut, mask, g = _inputs(B, S, H, D, dtype, seed, pad_from=pad_from)
    bl = A.block_lists(kl)
    nb = (S + 63) // 64
    got = _native(q, k, v, lut, mask, bl, p, 4242, scale, g)
    fam = "attn_f32" if dtype == F32 else "attn_hd"
    _assert_calls(calls, (fam + "_fwd", fam + "_bwd"), bl.heads, nb, nb)
    assert got[0].dtype == dtype and got[0].shape == (B, S, H, D)
    cnt = _counts(bl, S, S)
    ref = _grads(lambda a, b, c, lt: _dense(a, b, c, lt, mask, cnt, p, 4242, scale, torch.float64), q, k, v, lut, g,
                 torch.float64)
    floor = None
    if dtype == BF16:
        floor = _grads(lambda a, b, c, lt: _dense(a, b, c, lt, mask, cnt, p, 4242, scale, BF16), q, k, v, lut, g, BF16)
    _check(tag, dtype, got, ref, floor)
    for t in got:
        assert t is None or torch.isfinite(t.float()).all()
    return got, ref, mask


# S = 300: 5 blocks, a partial tail of 44; batch row 1 padded from key 230 (block 3 partly, block 4 wholly)
@pytest.mark.parametrize("dtype,D,heads,p", [(BF16, 64, 2, 0.0), (BF16, 64, 1, 0.1), (BF16, 40, 2, 0.0),
                                              (BF16, 128, 1, 0.0), (F32, 64, 2, 0.1), (F32, 64, 1, 0.0)],
                         ids=lambda x: str(x).replace("torch.", ""))
def test_random_lists_with_repeats(dtype, D, heads, p, calls):
    kl = _random_lists(heads, 5, 5, seed=D + heads)
    assert any(len(r) != len(set(r)) for hd in kl for r in hd)
    got, _, mask = _parity(f"lists {str(dtype)[6:]} D={D} Hl={heads} p={p}", calls, dtype, D,
                           kl if heads > 1 else kl[0], 300, 2, p, 230, seed=D)
    # padded keys: no gradient, exactly
    assert got[2][1, 230:].abs().max().item() == 0 and got[3][1, 230:].abs().max().item() == 0


@pytest.mark.parametrize("training", [True, False])
def test_the_bigbird_pattern(training, calls):
    """The pattern of models/bigbird.py at S = 832 (13 blocks), H = 4; eval mode has the repeats (block 0 four times in
    every sliding row)."""
    kl = bigbird_plan(832, 64, 3, 4, 0, training)
    if not training:
        assert all(r.count(0) == 4 for hd in kl for r in hd[1:-1])
    _parity(f"bigbird S=832 train={training}", calls, BF16, 64, kl, 832, 4, 0.0, 700, seed=7)


@pytest.mark.parametrize("dtype,D", [(BF16, 64), (BF16, 96), (F32, 64)], ids=lambda x: str(x).replace("torch.", ""))
def test_full_list_is_the_plain_call(dtype, D):
    """Every block once, ascending: the walk of the list-free call, block for block — o, LSE, dq, dk, dv bit for bit
    (the same binding with and without the tables; the bias gradient is summed by atomics, so to rounding)."""
    B, S, H = 2, 300, 2
    q, k, v, lut, mask, g = _inputs(B, S, H, D, dtype, 3, pad_from=230)
    C = _ext.native()
    fwd, bwd = (C.attn_f32_fwd, C.attn_f32_bwd) if dtype == F32 else (C.attn_hd_fwd, C.attn_hd_bwd)
    m8 = mask.to(torch.uint8)
    for heads in (1, 2):
        full = [[list(range(5))] * 5] * heads
        t = A.block_lists(full if heads > 1 else full[0]).tables(DEV, S, S)
        res = []
        for kw in ({}, t):
            o, lse = fwd(q, k, v, m8, lut, 0.125, False, 0.1, 77, **kw)
            dq, dk, dv, dlut = bwd(g, q, k, v, o, lse, m8, lut, 0.125, False, 0.1, 77, True, **kw)
            res.append((o, lse, dq, dk, dv, dlut))
        for n, a, b in zip(("o", "lse", "dq", "dk", "dv"), res[0], res[1]):
            assert torch.equal(a, b), (heads, n)
        assert R.rel_l2(res[1][5], res[0][5]) < 1e-5
    rev = A.block_lists([list(range(4, -1, -1))] * 5).tables(DEV, S, S)  # another order: another rounding, same sum
    o2, _ = fwd(q, k, v, m8, lut, 0.125, False, 0.1, 77, **rev)
    assert not torch.equal(o2, res[0][0]) and R.rel_l2(o2, res[0][0]) < (1e-2 if dtype == BF16 else 1e-5)


def test_unlisted_blocks_are_not_loaded(calls):
    """S = 512 (8 blocks); no list names key blocks 3 and 4, whose K and V rows are NaN.  A kernel that loaded and
    masked them would give NaN (0 x NaN in P V and dS K); following the lists, o and dq are finite and bitwise those of
    the run on zero-filled inputs, and so are dk / dv of the listed blocks.  The two unlisted key blocks walk nothing:
    their dk / dv are exactly 0, NaN operands or not."""
    B, S, H, D = 1, 512, 2, 64
    q, k, v, _, _, g = _inputs(B, S, H, D, BF16, 4, bias=False)
    rs = np.random.RandomState(0)
    allowed = [0, 1, 2, 5, 6, 7]
    kl = [[[allowed[i] for i in rs.randint(0, 6, size=rs.randint(1, 5))] for _ in range(8)] for _ in range(H)]
    bl = A.block_lists(kl)
    kz, vz = k.clone(), v.clone()
    kz[:, 192:320] = 0
    vz[:, 192:320] = 0
    kn, vn = k.clone(), v.clone()
    kn[:, 192:320] = float("nan")
    vn[:, 192:320] = float("nan")
    poison = _native(q, kn, vn, None, None, bl, 0.0, 0, D ** -0.5, g)
    _assert_calls(calls, ("attn_hd_fwd", "attn_hd_bwd"), H, 8, 8)
    clean = _native(q, kz, vz, None, None, bl, 0.0, 0, D ** -0.5, g)
    for n, a, b in zip(("o", "dq", "dk", "dv"), poison, clean):
        assert torch.isfinite(a.float()).all(), n
        assert torch.equal(a, b), n
    assert poison[2][:, 192:320].abs().max().item() == 0 and poison[3][:, 192:320].abs().max().item() == 0
    assert poison[2][:, :192].abs().max().item() > 0
    # the poison is real: the full list reads it
    o = A.attention(q, kn, vn, scale=D ** -0.5, block_lists=A.block_lists([list(range(8))] * 8))
    assert torch.isnan(o.float()).any()


@pytest.mark.parametrize("dtype", [BF16, F32], ids=lambda x: str(x).replace("torch.", ""))
def test_empty_list_and_unlisted_key_block(dtype):
    """Query block 2 of head 0 lists nothing: output 0, LSE +inf, dq 0.  Key block 3 of head 1 stands in no list:
    dk = dv = 0 exactly.  An out-of-range entry is passed over."""
    B, S, H, D = 2, 300, 2, 64
    kl = [[[0, 1], [1, 1, 2], [], [0, 4, 9], [4, 3, 0]], [[0], [1, 0, 1], [2], [2, 4, -1], [4, 4, 4]]]
    kl_clean = [[[0, 1], [1, 1, 2], [], [0, 4], [4, 3, 0]], [[0], [1, 0, 1], [2], [2, 4], [4, 4, 4]]]
    q, k, v, lut, _, g = _inputs(B, S, H, D, dtype, 5)
    # out-of-range entries reach the kernels only through hand-made tables: block_lists drops them on the host
    t = A.block_lists(kl_clean).tables(DEV, S, S)
    raw = {n: x.clone() for n, x in t.items()}

    def insert(ptr, idx, row, value):
        """``value`` appended to the list of flat row ``row`` of the CSR table."""
        flat = raw[ptr].view(-1)
        pos = int(flat[row + 1])
        raw[idx] = torch.cat((raw[idx][:pos], torch.tensor([value], dtype=torch.int32, device=DEV), raw[idx][pos:]))
        flat[row + 1:] += 1

    insert("kl_ptr", "kl_idx", 3, 9)   # head 0, query block 3: [0, 4, 9]
    insert("ql_ptr", "ql_idx", 0, -5)  # head 0, key block 0: a negative query block
    assert raw["kl_idx"].numel() == raw["ql_idx"].numel() == t["kl_idx"].numel() + 1
    C = _ext.native()
    fwd, bwd = (C.attn_f32_fwd, C.attn_f32_bwd) if dtype == F32 else (C.attn_hd_fwd, C.attn_hd_bwd)
    res = []
    for tab in (t, raw):
        o, lse = fwd(q, k, v, None, lut, 0.125, False, 0.0, 0, **tab)
        dq, dk, dv, dlut = bwd(g, q, k, v, o, lse, None, lut, 0.125, False, 0.0, 0, True, **tab)
        res.append((o, lse, dq, dk, dv))
        assert o[:, 128:192, 0].abs().max().item() == 0 and dq[:, 128:192, 0].abs().max().item() == 0
        assert torch.isposinf(lse[:, 0, 128:192]).all() and torch.isfinite(lse[:, 1]).all()
        assert torch.isfinite(lse[:, 0, :128]).all() and torch.isfinite(lse[:, 0, 192:]).all()
        assert dk[:, 192:256, 1].abs().max().item() == 0 and dv[:, 192:256, 1].abs().max().item() == 0
        assert dk[:, 192:256, 0].abs().max().item() > 0
        for x in (o, dq, dk, dv, dlut):
            assert torch.isfinite(x.float()).all()
    for n, a, b in zip(("o", "lse", "dq", "dk", "dv"), *res):
        assert torch.equal(a, b), n  # the out-of-range entry changes nothing
    assert A.block_lists(kl).counts().tolist() == A.block_lists(kl_clean).counts().tolist()


# --------------------------------------------------------------------------------------------------- the binding
@pytest.mark.parametrize("family,dtype", [("attn_hd", BF16), ("attn_f32", F32)])
def test_binding_rejects(family, dtype):
    C = _ext.native()
    fwd, bwd = getattr(C, family + "_fwd"), getattr(C, family + "_bwd")
    B, S = 2, 128
    q = torch.randn(B, S, 2, 64, device=DEV).to(dtype)
    t = A.block_lists([[0, 1], [1, 1]]).tables(DEV, S, S)
    o, lse = fwd(q, q, q, None, None, 0.125, False, 0.0, 0, **t)
    o2, _ = fwd(q, q, q, None, None, 0.125, False, 0.0, 0)  # the trailing arguments default to no lists
    o3, _ = fwd(q, q, q, None, None, 0.125, False, 0.0, 0, -1, None, None, None, None, None, None, None, None, None,
                None)
    assert torch.equal(o2, o3) and not torch.equal(o, o2)
    seg = A.segments(torch.zeros(B, S, dtype=torch.int32, device=DEV))
    gk = A.global_keys(torch.zeros(B, S, dtype=torch.bool, device=DEV))
    one = {**t, "kl_ptr": t["kl_ptr"].repeat(3, 1)}
    bad = [
        (dict(t, window=5), "block lists with a window"),
        (dict(t, q_seg=seg.ids, k_seg=seg.ids, q_blk=seg.blk, k_blk=seg.blk), "block lists with segments"),
        (dict(t, window=5, k_glob=gk.flags, k_gblk=gk.blk), "block lists with global keys"),
        ({n: x for n, x in t.items() if n != "ql_idx"}, "together"),
        (dict(kl_ptr=t["kl_ptr"]), "together"),
        (one, r"kl_ptr: expected \[H or 1, 3\]"),
        ({**t, "kl_ptr": t["kl_ptr"][:, :2].contiguous()}, r"kl_ptr: expected \[H or 1, 3\]"),
        ({**t, "ql_ptr": t["ql_ptr"].repeat(2, 1)}, r"ql_ptr: expected \[1, 3\]"),
        ({**t, "ql_idx": t["ql_idx"][:-1].contiguous()}, "one length"),
        ({**t, "kl_idx": t["kl_idx"].long()}, "kl_idx must be int32"),
        ({**t, "ql_ptr": t["ql_ptr"].long()}, "ql_ptr must be int32"),
        ({**t, "kl_ptr": t["kl_ptr"].cpu()}, "kl_ptr must be a GPU tensor"),
        ({**t, "ql_idx": t["ql_idx"].cpu()}, "ql_idx must be a GPU tensor"),
    ]
    for kw, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            fwd(q, q, q, None, None, 0.125, False, 0.0, 0, **kw)
        with pytest.raises(RuntimeError, match=msg):
            bwd(o, q, q, q, o, lse, None, None, 0.125, False, 0.0, 0, False, **kw)
    with pytest.raises(RuntimeError, match="block lists with causal"):
        fwd(q, q, q, None, None, 0.125, True, 0.0, 0, **t)
    with pytest.raises(RuntimeError, match="block lists with causal"):
        bwd(o, q, q, q, o, lse, None, None, 0.125, True, 0.0, 0, False, **t)
    torch.cuda.synchronize()


def test_attn_lists_0_takes_the_composite(calls, monkeypatch):
    B, S, H, D = 1, 300, 2, 64
    q, k, v, lut, _, _ = _inputs(B, S, H, D, BF16, 6)
    bl = A.block_lists(_random_lists(H, 5, 5, seed=1))
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(attn_lists=0))
    o = A.attention(q, k, v, scale=0.125, bias_lut=lut, block_lists=bl)
    assert calls == []
    assert torch.equal(o, A._reference(q, k, v, 0.125, False, None, lut, 0.0, 0, bl=bl))
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(attn_lists=1))
    o1 = A.attention(q, k, v, scale=0.125, bias_lut=lut, block_lists=bl)
    assert [c[0] for c in calls] == ["attn_hd_fwd"]
    assert R.rel_l2(o1, o) < 2e-2


def test_head_dim_32_takes_the_composite(calls):
    """csrc/attn_hd.hip serves no lists at head dim 32 (its three kernels stay as they were): the binding rejects the
    tables and the op runs the composite, while the list-free call at head dim 32 stays on the kernel."""
    B, S, H, D = 1, 130, 2, 32
    x = torch.randn(B, S, H, D, device=DEV, dtype=BF16)
    bl = A.block_lists([[0, 1, 1], [2], [0, 2]])
    o = A.attention(x, x, x, scale=D ** -0.5, block_lists=bl)
    assert calls == []
    assert torch.equal(o, A._reference(x, x, x, D ** -0.5, False, None, None, 0.0, 0, bl=bl))
    A.attention(x, x, x, scale=D ** -0.5)
    assert [c[0] for c in calls] == ["attn_hd_fwd"]
    with pytest.raises(RuntimeError, match="head dim 32"):
        _ext.native().attn_hd_fwd(x, x, x, None, None, D ** -0.5, False, 0.0, 0, **bl.tables(DEV, S, S))


def test_other_block_sizes(calls):
    """A block size that is a multiple of 64 is expanded to 64-blocks and runs the kernel; any other takes the
    composite."""
    B, S, H, D = 1, 300, 2, 64
    q, k, v, _, _, _ = _inputs(B, S, H, D, BF16, 8, bias=False)
    kl128 = [[0, 2], [1, 1], [2, 0]]
    o = A.attention(q, k, v, scale=0.125, block_lists=A.block_lists(kl128, block=128))
    _assert_calls(calls, ("attn_hd_fwd",), 1, 5, 5)
    ref = A._reference(q.float(), k.float(), v.float(), 0.125, False, None, None, 0.0, 0,
                       bl=A.block_lists(kl128, block=128))
    assert R.row_err(o, ref) < 2e-2
    del calls[:]
    kl100 = [[0, 2], [1, 1], [2, 0]]
    bl = A.block_lists(kl100, block=100)
    o = A.attention(q, k, v, scale=0.125, block_lists=bl)
    assert calls == []
    assert torch.equal(o, A._reference(q, k, v, 0.125, False, None, None, 0.0, 0, bl=bl))
