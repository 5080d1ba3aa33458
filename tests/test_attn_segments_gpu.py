"""Segment-masked attention kernels (csrc/attn_hd.hip, csrc/attn_f32.hip with ``q_seg`` / ``k_seg``): forward +
backward against the composite ``A._reference(..., q_seg, k_seg)`` on fp32 copies of the same values, at the bounds of
tests/test_attn_window_gpu.py (bf16: rel-L2 2e-2 on the output, 3e-2 on dq / dk / dv, the bias gradient on the bucket
table; fp32 against an fp64 composite: 2e-6 / 2e-5).  A spy asserts which binding ran and that it was given segments.
Beyond parity: one segment over everything is bitwise the call without segments, blocks of other segments are skipped,
not masked (NaN poison in them never reaches a segment whose own blocks are clean), and indices hold at 16K tokens."""
import pytest
import torch

from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops import attention as A
from distributed_llms_example_amd.ops.rng import attention_keep_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
_NAMES = ("attn_fwd", "attn_bwd", "attn_hd_fwd", "attn_hd_bwd", "attn_f32_fwd", "attn_f32_bwd")


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


class _Spy:
    """The native module with the attention bindings' calls recorded as (name, window argument, segments given)."""

    def __init__(self, calls, real):
        self.calls = calls
        self.real = real

    def __getattr__(self, n):
        real = getattr(self.real, n)
        if n in _NAMES:
            def f(*a, **kw):
                w, seg = None, False
                if n not in ("attn_fwd", "attn_bwd"):  # the trailing `window`, then q_seg, k_seg, q_blk, k_blk
                    pos = 9 if n.endswith("fwd") else 16
                    w = a[pos] if len(a) > pos else kw.get("window", -1)
                    seg = all(t is not None for t in a[pos + 1:pos + 5]) and len(a) == pos + 5
                self.calls.append((n, w, seg))
                return real(*a, **kw)
            return f
        return real


@pytest.fixture
def calls(monkeypatch):
    out = []
    spy = _Spy(out, _ext.native())
    monkeypatch.setattr(A._ext, "native", lambda: spy)
    return out


def _ids(bounds, S, tail):
    """ids 0, 1, 2, ... with segment starts at 0 and ``bounds`` and -1 from ``tail`` on (int64, on the GPU)."""
    seg = torch.zeros(S, dtype=torch.int64)
    for b in bounds:
        seg[b:] += 1
    seg[tail:] = -1
    return seg.to(DEV)


# a one-token segment, a boundary exactly on a block edge, one just past it, a segment spanning three blocks, a -1 tail
SEG333 = [1, 64, 65, 128, 200]


def _seg_self(S, B=2):
    if S == 333:
        rows = [_ids(SEG333, S, 300), _ids([10, 100, 190], S, S)]
    else:  # a single segment plus tail / a single segment
        rows = [_ids([], S, S - S // 4), _ids([], S, S)]
    return torch.stack(rows[:B])


def _visible(qs, ks, kpm, causal):
    """[B, Sq, Sk] bool: the key is visible to the query."""
    Sq, Sk = qs.shape[1], ks.shape[1]
    vis = (ks[:, None, :] >= 0) & (qs[:, :, None] == ks[:, None, :])
    if kpm is not None:
        vis = vis & kpm[:, None, :]
    if causal:
        vis = vis & (torch.arange(Sk, device=DEV)[None, :] <= torch.arange(Sq, device=DEV)[:, None] + (Sk - Sq))[None]
    return vis


def _lut(tab, Sq, Sk, causal):
    return A.relative_bias_lut(tab, Sq, Sk, not causal, 32, 128) if tab is not None else None


def _run(q, kv, table, mask, qs, ks, causal, p, seed, mode, g, scale=1.0):
    """One native forward + backward: (o, dq, dk, dv, dtable).  ``kv`` is [B, Sk, 2, H, D]; ``mode``: "qkv" (one packed
    tensor, self-attention), "q_kv" or "sep"."""
    Sq, Sk = q.shape[1], kv.shape[1]
    tab = table.clone().requires_grad_(True) if table is not None else None
    kw = dict(scale=scale, causal=causal, key_padding_mask=mask, bias_lut=_lut(tab, Sq, Sk, causal), dropout_p=p,
              seed=seed)
    if mode == "qkv":
        x = torch.cat([q[:, :, None], kv], 2).clone().requires_grad_(True)
        o = A.attention_qkv(x, segments=qs, **kw) if qs is not None else A.attention_qkv(x, **kw)
        (o.float() * g.float()).sum().backward()
        dq, dk, dv = x.grad[:, :, 0], x.grad[:, :, 1], x.grad[:, :, 2]
    else:
        xq, xkv = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
        if qs is not None:
            kw.update(q_segments=qs, k_segments=ks)
        if mode == "q_kv":
            o = A.attention_q_kv(xq, xkv, **kw)
        else:
            o = A.attention(xq, xkv[:, :, 0], xkv[:, :, 1], **kw)
        (o.float() * g.float()).sum().backward()
        dq, dk, dv = xq.grad, xkv.grad[:, :, 0], xkv.grad[:, :, 1]
    return o.detach(), dq, dk, dv, (tab.grad if tab is not None else None)


def _oracle(q, kv, table, mask, qs, ks, causal, p, seed, g, scale=1.0):
    """The composite on fp32 copies: (o, dq, dk, dv, dtable)."""
    Sq, Sk = q.shape[1], kv.shape[1]
    xq, xkv = q.detach().float().requires_grad_(True), kv.detach().float().requires_grad_(True)
    tab = table.clone().requires_grad_(True) if table is not None else None
    lut = _lut(tab, Sq, Sk, causal)
    o = A._reference(xq, xkv[:, :, 0], xkv[:, :, 1], scale, causal, mask, lut, p, seed, None, qs, ks)
    (o * g.float()).sum().backward()
    return o.detach(), xq.grad, xkv.grad[:, :, 0], xkv.grad[:, :, 1], (tab.grad if tab is not None else None)


def _check(tag, got, ref, tol_o=2e-2, tol_g=3e-2):
    errs = {n: _rel(a, b) for n, a, b in zip(("o", "dq", "dk", "dv", "dtable"), got, ref) if a is not None}
    print(f"[{tag}] {errs}")
    for n, e in errs.items():
        assert e < (tol_o if n == "o" else tol_g), (tag, n, e)


def _problem(kind, B, H, D, S, bias, kpm, seed, dtype=torch.bfloat16):
    """(q, kv, table, mask, q ids, k ids, causal, g) of a case: ``kind`` "self" / "causal" (S x S) or "cross" (130 x
    300, three segments of unequal share)."""
    torch.manual_seed(seed)
    causal = kind == "causal"
    if kind == "cross":
        Sq, Sk = 130, 300
        qs = torch.stack([_ids([20, 90], Sq, 120), _ids([64, 100], Sq, Sq)][:B])
        ks = torch.stack([_ids([100, 130], Sk, 280), _ids([10, 250], Sk, 290)][:B])
    else:
        Sq = Sk = S
        qs = ks = _seg_self(S, B)
    q = torch.randn(B, Sq, H, D, device=DEV).to(dtype)
    kv = torch.randn(B, Sk, 2, H, D, device=DEV).to(dtype)
    table = torch.randn(32, H, device=DEV) * 0.5 if bias else None
    mask = None
    if kpm:  # the last three keys of batch 0's last segment (>= 10 keys long in every case) and two keys inside batch 1
        mask = torch.ones(B, Sk, dtype=torch.bool, device=DEV)
        last = int((ks[0] >= 0).sum())
        mask[0, last - 3:last] = False
        if B > 1:
            mask[1, 70:72] = False
    g = torch.randn(B, Sq, H, D, device=DEV).to(dtype)
    return q, kv, table, mask, qs, ks, causal, g


BF16_CASES = [
    # kind, H, S, D, bias, kpm, p, mode
    ("self", 2, 333, 64, True, True, 0.1, "qkv"),      # the packed encoder's own call; D = 64 must not reach attn_fwd
    ("self", 3, 333, 64, False, False, 0.0, "sep"),
    ("self", 2, 200, 64, True, False, 0.0, "qkv"),     # a single segment plus tail
    ("causal", 2, 333, 64, True, False, 0.1, "qkv"),   # the packed decoder's self-attention
    ("causal", 3, 333, 40, False, True, 0.0, "sep"),
    ("cross", 2, 0, 64, False, True, 0.1, "q_kv"),     # the packed decoder's cross-attention
    ("cross", 3, 0, 128, False, False, 0.0, "sep"),
    ("self", 2, 333, 40, True, True, 0.1, "sep"),      # DP = 64 with D = 40
    ("self", 2, 333, 128, False, True, 0.0, "qkv"),    # DP = 128
]


@pytest.mark.parametrize("kind,H,S,D,bias,kpm,p,mode", BF16_CASES)
def test_segments_bf16(kind, H, S, D, bias, kpm, p, mode, calls):
    B = 2
    q, kv, table, mask, qs, ks, causal, g = _problem(kind, B, H, D, S, bias, kpm, seed=S * 7 + D + H)
    # rows without a visible key (padding rows; none else by construction): the kernels return 0 there, and they are
    # left out of the output comparison and carry no output gradient on either side, as in tests/test_attn_window_gpu.py
    vis = _visible(qs, ks, mask, causal).any(-1)
    assert torch.equal(vis, qs >= 0)
    g[~vis] = 0
    scale = 1.0 if bias else D ** -0.5
    got = _run(q, kv, table, mask, qs, ks, causal, p, 4242, mode, g, scale)
    assert calls == [("attn_hd_fwd", -1, True), ("attn_hd_bwd", -1, True)], calls
    assert got[0].dtype == torch.bfloat16 and got[0].shape == q.shape
    for t in got[:4]:
        assert torch.isfinite(t.float()).all()
    assert got[0][~vis].abs().max().item() == 0 and got[1][~vis].abs().max().item() == 0
    assert got[2][ks < 0].abs().max().item() == 0 and got[3][ks < 0].abs().max().item() == 0
    ref = _oracle(q, kv, table, mask, qs, ks, causal, p, 4242, g, scale)
    _check(f"segments bf16 {kind} S={S} D={D} {mode}", (got[0][vis],) + got[1:], (ref[0][vis],) + ref[1:])


def test_lse_of_padding_rows_is_inf():
    B, H, D, S = 2, 2, 64, 333
    q, kv, _, _, qs, ks, _, _ = _problem("self", B, H, D, S, False, False, seed=1)
    sq = A.segments(qs)
    _, lse = _ext.native().attn_hd_fwd(q, kv[:, :, 0], kv[:, :, 1], None, None, D ** -0.5, False, 0.0, 0, -1,
                                       sq.ids, sq.ids, sq.blk, sq.blk)
    pad = (qs < 0)[:, None, :].expand(B, H, S)
    assert torch.isposinf(lse[pad]).all() and torch.isfinite(lse[~pad]).all()


# ---------------------------------------------------------------------------------------------------------- fp32
def _ref64(q, k, v, scale, causal, kpm, lut, p, seed, qs, ks):
    """fp64 composite with the segment mask; rows without a visible key return 0."""
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    qf, kf, vf = (t.double().permute(0, 2, 1, 3) for t in (q, k, v))
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if lut is not None:
        rel = torch.arange(Sk, device=DEV)[None, :] - torch.arange(Sq, device=DEV)[:, None] + (Sq - 1)
        s = s + lut.double()[:, rel].unsqueeze(0)
    vis = _visible(qs, ks, kpm, causal)
    s = s.masked_fill(~vis[:, None], torch.finfo(torch.float64).min)
    pr = torch.softmax(s, dim=-1) * vis.any(-1)[:, None, :, None]
    if p > 0.0:
        pr = pr * attention_keep_mask(seed, p, B, H, Sq, Sk, q.device).double() / (1.0 - p)
    return torch.matmul(pr, vf).permute(0, 2, 1, 3)


@pytest.mark.parametrize("kind,bias,kpm,p", [("self", True, True, 0.1), ("causal", True, False, 0.0),
                                             ("cross", False, True, 0.1)])
def test_segments_fp32_matches_fp64(kind, bias, kpm, p, calls):
    B, H, S = 2, 3, 333
    q, kv, _, mask, qs, ks, causal, g = _problem(kind, B, H, 64, S, False, kpm, seed=S + len(kind), dtype=torch.float32)
    Sq, Sk = q.shape[1], kv.shape[1]
    q.requires_grad_(True)
    k, v = (kv[:, :, i].clone().requires_grad_(True) for i in range(2))
    lut = (torch.randn(H, Sq + Sk - 1, device=DEV) * 0.5).requires_grad_(True) if bias else None
    ins = [t for t in (q, k, v, lut) if t is not None]
    g[qs < 0] = 0
    o = A.attention(q, k, v, scale=0.125, causal=causal, key_padding_mask=mask, bias_lut=lut, dropout_p=p, seed=1234,
                    q_segments=qs, k_segments=ks)
    assert o.dtype == torch.float32
    grads = torch.autograd.grad(o, ins, g)
    assert calls == [("attn_f32_fwd", -1, True), ("attn_f32_bwd", -1, True)], calls
    ins64 = [t.detach().double().requires_grad_(True) for t in ins]
    o64 = _ref64(*ins64[:3], 0.125, causal, mask, ins64[3] if bias else None, p, 1234, qs, ks)
    grads64 = torch.autograd.grad(o64, ins64, g.double())
    assert o[qs < 0].abs().max().item() == 0
    errs = {"o": _rel(o, o64)}
    errs.update({n: _rel(a, b) for n, a, b in zip(("dq", "dk", "dv", "dlut"), grads, grads64)})
    print(f"[segments fp32 {kind}] {errs}")
    assert errs.pop("o") < 2e-6
    for n, e in errs.items():
        assert e < 2e-5, (n, e)
    # the composite (fp32) agrees with the fp64 one on the same segments: the oracle of the bf16 cases
    oc = A._reference(q.detach(), k.detach(), v.detach(), 0.125, causal, mask, lut.detach() if bias else None, p, 1234,
                      None, qs, ks)
    assert _rel(oc, o64) < 1e-5


# --------------------------------------------------------------------------------------------------------- bitwise
@pytest.mark.parametrize("dtype,D,family", [(torch.bfloat16, 40, "attn_hd"), (torch.float32, 64, "attn_f32")])
def test_one_segment_over_everything_is_no_segments(dtype, D, family, calls):
    """One segment, no tail, masks nothing and skips nothing: bitwise the call without segments in the same family.
    The bias gradient is accumulated with fp32 atomics whose order differs between two launches of the very same call,
    so it is held to fp32 summation noise (1e-5), as test_window_wider_than_the_sequence_is_no_window does."""
    B, H, S = 2, 3, 150
    torch.manual_seed(2)
    q = torch.randn(B, S, H, D, device=DEV).to(dtype)
    kv = torch.randn(B, S, 2, H, D, device=DEV).to(dtype)
    table = torch.randn(32, H, device=DEV) * 0.5
    g = torch.randn(B, S, H, D, device=DEV).to(dtype)
    one = torch.zeros(B, S, dtype=torch.int64, device=DEV)
    seven = torch.full((B, S), 7, dtype=torch.int32, device=DEV)
    a = _run(q, kv, table, None, one, one, False, 0.1, 77, "sep", g, D ** -0.5)
    b = _run(q, kv, table, None, None, None, False, 0.1, 77, "sep", g, D ** -0.5)
    c = _run(q, kv, table, None, seven, seven, False, 0.1, 77, "qkv", g, D ** -0.5)
    assert [n for n, _, _ in calls] == [family + "_fwd", family + "_bwd"] * 3, calls
    assert [s for _, _, s in calls] == [True, True, False, False, True, True], calls
    for n, x, y, z in zip(("o", "dq", "dk", "dv"), a, b, c):
        assert torch.equal(x, y), n
        assert torch.equal(z, y), n
    assert _rel(a[4], b[4]) < 1e-5 and _rel(c[4], b[4]) < 1e-5


# ------------------------------------------------------------------------------------------- skipping, not masking
def test_blocks_of_other_segments_are_not_loaded(calls):
    """Segments [0, 256), [256, 768), [768, 1024); K, V and dO of the middle segment — eight whole blocks — are NaN.
    Every block the outer segments' rows (and, in dK / dV, their keys) share a segment with is clean, so a kernel that
    skips the other blocks gives finite values there, equal to the run on zero-filled inputs; one that loads and masks
    them gives NaN (0 * NaN in P V and dS^T Q).  (Boundaries inside a block are the parity cases' business: a block that
    holds rows of the poisoned segment is rightly loaded, and those rows' own LSE and delta are NaN.)"""
    B, H, S, D = 1, 2, 1024, 64
    torch.manual_seed(4)
    seg = _ids([256, 768], S, S)[None]
    q = torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16)
    kv = torch.randn(B, S, 2, H, D, device=DEV).to(torch.bfloat16)
    g = torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16)
    clean, gclean = kv.clone(), g.clone()
    clean[:, 256:768] = 0
    gclean[:, 256:768] = 0
    kv[:, 256:768] = float("nan")
    g[:, 256:768] = float("nan")
    xq, xkv = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    o = A.attention_q_kv(xq, xkv, scale=D ** -0.5, q_segments=seg, k_segments=seg)
    o.backward(g)
    assert calls == [("attn_hd_fwd", -1, True), ("attn_hd_bwd", -1, True)], calls
    dq, dk, dv = xq.grad, xkv.grad[:, :, 0], xkv.grad[:, :, 1]
    assert torch.isnan(o[:, 256:768].float()).all()  # the poison is real
    rows = torch.cat([torch.arange(0, 256), torch.arange(768, S)]).to(DEV)
    for n, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert torch.isfinite(t[:, rows].float()).all(), n
    ref = _oracle(q, clean, None, None, seg, seg, False, 0.0, 0, gclean, D ** -0.5)
    got = (o.detach(), dq, dk, dv)
    _check("segments bf16 poison", tuple(t[:, rows] for t in got), tuple(t[:, rows] for t in ref[:4]))


# ------------------------------------------------------------------------------------------------- long indices
def _segment_oracle(q, kv, table, lens, g):
    """Every segment on its own (the composite on its rows and keys): O(sum len^2) memory.  The bias is built from the
    bucket table per segment (not through the LUT the kernel reads); rows past the last segment stay 0."""
    xq, xkv = q.detach().float().requires_grad_(True), kv.detach().float().requires_grad_(True)
    tab = table.clone().requires_grad_(True)
    outs, a = [], 0
    for n in lens:
        qq = xq[:, a:a + n].permute(0, 2, 1, 3)
        k = xkv[:, a:a + n, 0].permute(0, 2, 1, 3)
        v = xkv[:, a:a + n, 1].permute(0, 2, 1, 3)
        rel = torch.arange(n, device=DEV)[None, :] - torch.arange(n, device=DEV)[:, None]
        s = torch.matmul(qq, k.transpose(-1, -2)) + tab[A.relative_position_bucket(rel, True, 32, 128)].permute(2, 0, 1)
        outs.append(torch.matmul(torch.softmax(s, -1), v).permute(0, 2, 1, 3))
        a += n
    outs.append(torch.zeros_like(xq[:, a:]))
    o = torch.cat(outs, 1)
    (o * g.float()).sum().backward()
    return o.detach(), xq.grad, xkv.grad[:, :, 0], xkv.grad[:, :, 1], tab.grad


def test_segments_at_16k_tokens(calls):
    B, H, S, D, tail = 1, 2, 16384, 64, 37
    gen = torch.Generator().manual_seed(5)
    lens = (40 + torch.randint(0, 740, (40,), generator=gen)).tolist()  # 40 segments of 40 .. 779 tokens, mean ~410
    while sum(lens) > S - tail:
        lens.pop()
    lens.append(S - tail - sum(lens))  # the last segment ends 37 rows before the end: the tail is padding
    assert 35 <= len(lens) <= 41 and min(lens) > 0
    bounds = torch.tensor(lens).cumsum(0)[:-1].tolist()
    seg = _ids(bounds, S, S - tail)[None]
    torch.manual_seed(5)
    q = torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16)
    kv = torch.randn(B, S, 2, H, D, device=DEV).to(torch.bfloat16)
    table = torch.randn(32, H, device=DEV) * 0.5
    g = torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16)
    g[:, S - tail:] = 0
    got = _run(q, kv, table, None, seg, seg, False, 0.0, 0, "qkv", g)
    assert calls == [("attn_hd_fwd", -1, True), ("attn_hd_bwd", -1, True)], calls
    assert got[0][:, S - tail:].abs().max().item() == 0
    ref = _segment_oracle(q, kv, table, lens, g)
    _check("segments bf16 S=16384", got, ref)
    # the last rows on their own: an index error far from the origin cannot hide in a whole-tensor norm
    _check("segments bf16 S=16384 tail", tuple(t[:, -200:] for t in got[:4]), tuple(t[:, -200:] for t in ref[:4]))


# --------------------------------------------------------------------------------------------------- the binding
@pytest.mark.parametrize("family,dtype", [("attn_hd", torch.bfloat16), ("attn_f32", torch.float32)])
def test_binding_rejects_bad_segments(family, dtype):
    C = _ext.native()
    fwd, bwd = getattr(C, family + "_fwd"), getattr(C, family + "_bwd")
    q = torch.randn(1, 128, 2, 64, device=DEV).to(dtype)
    k = torch.randn(1, 192, 2, 64, device=DEV).to(dtype)
    sq = A.segments(torch.zeros(1, 128, dtype=torch.int64, device=DEV))
    sk = A.segments(torch.zeros(1, 192, dtype=torch.int64, device=DEV))
    o, lse = fwd(q, k, k, None, None, 0.125, False, 0.0, 0, -1, sq.ids, sk.ids, sq.blk, sk.blk)
    o2, _ = fwd(q, k, k, None, None, 0.125, False, 0.0, 0)  # the trailing arguments default to no segments
    o3, _ = fwd(q, k, k, None, None, 0.125, False, 0.0, 0, q_seg=sq.ids, k_seg=sk.ids, q_blk=sq.blk, k_blk=sk.blk)
    assert torch.equal(o, o2) and torch.equal(o, o3)
    args = (q, k, k, None, None, 0.125, False, 0.0, 0, -1)
    with pytest.raises(RuntimeError, match="together"):
        fwd(*args, sq.ids, None, sq.blk, sk.blk)
    with pytest.raises(RuntimeError, match="together"):
        fwd(*args, sq.ids, sk.ids)
    with pytest.raises(RuntimeError, match="int32"):
        fwd(*args, sq.ids.long(), sk.ids, sq.blk, sk.blk)
    with pytest.raises(RuntimeError, match="expected"):
        fwd(*args, sk.ids, sk.ids, sq.blk, sk.blk)
    with pytest.raises(RuntimeError, match="expected"):
        fwd(*args, sq.ids, sk.ids, sk.blk, sk.blk)
    with pytest.raises(RuntimeError, match="contiguous"):
        fwd(*args, sq.ids, torch.zeros(1, 384, dtype=torch.int32, device=DEV)[:, ::2], sq.blk, sk.blk)
    with pytest.raises(RuntimeError, match="GPU"):
        fwd(*args, sq.ids.cpu(), sk.ids, sq.blk, sk.blk)
    k1 = k[:, :128]
    with pytest.raises(RuntimeError, match="window"):
        fwd(q, k1, k1, None, None, 0.125, False, 0.0, 0, 5, sq.ids, sq.ids, sq.blk, sq.blk)
    with pytest.raises(RuntimeError, match="window"):
        bwd(o, q, k1, k1, o, lse, None, None, 0.125, False, 0.0, 0, False, window=5, q_seg=sq.ids, k_seg=sq.ids,
            q_blk=sq.blk, k_blk=sq.blk)
    with pytest.raises(RuntimeError, match="together"):
        bwd(o, q, k, k, o, lse, None, None, 0.125, False, 0.0, 0, False, q_seg=sq.ids)
    torch.cuda.synchronize()


def test_op_rejects_window_with_segments_on_gpu():
    x = torch.randn(1, 70, 2, 64, device=DEV, dtype=torch.bfloat16)
    seg = torch.zeros(1, 70, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="window"):
        A.attention(x, x, x, window=3, q_segments=seg, k_segments=seg)


def test_unserved_segmented_call_takes_the_composite(calls):
    """Head dim 16 with segments: no kernel, the composite with the segment mask (and no binding call)."""
    x = torch.randn(1, 70, 2, 16, device=DEV, dtype=torch.bfloat16)
    seg = _ids([30], 70, 60)[None]
    o = A.attention(x, x, x, q_segments=seg, k_segments=seg)
    assert calls == []
    assert torch.equal(o, A._reference(x, x, x, 1.0, False, None, None, 0.0, 0, None, seg, seg))
