"""The attention kernels (csrc/attn.hip; matrix only: attn_hd.hip, attn_f32.hip) per row and arm by arm, against the
fp64 reference of tests/attn_refs.py (validated on the CPU by tests/test_attn_refs_cpu.py).

Metrics: per-ROW relative error for o, dq, dk, dv (one wrong row, or a key dropped at a ragged tile edge, passes a
whole-tensor rel-L2: test_attn_refs_cpu.test_metric_sensitivity); absolute LSE error in log2 units; error against the
L1 mass of the terms for the bias-LUT gradient and the column sums; exact zeros where the contract says zero
(gradients of padded keys, everything of a row without a visible key). Every bf16 bound is 4 x the error of the bf16
MODEL (``attn_bf16_model``: the reference rounded where the kernels round) on the same inputs, computed here and
printed beside the kernel's figure — never a number taken from a kernel run. Each ``[fig]`` line shows kernel, model,
bound; a test asserts them together at its end (run with -s to collect them).

Ring depths and the short-query kernel's blocks per workgroup (MB) cannot be observed from Python: ``_fwd_ring``,
``_dkdv2_ring`` and ``_sq_mb`` mirror the launchers' selection rules and the tests assert the arm they mean to reach.
"""
import pytest
import torch

import attn_refs as R
import rowwise_refs as RW
from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops import attention as A
from distributed_llms_example_amd.ops import routing
from distributed_llms_example_amd.parallel import context as cp

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
OUTS = ("o", "dq", "dk", "dv")


class Figures:
    """Collects (name, kernel, model, bound) lines, prints each, asserts them all at the end of the test."""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def add(self, name, val, bound, model=None, comp=None):
        line = (f"[fig] {self.tag} {name}: err {val:.3e}" + (f" model {model:.3e}" if model is not None else "")
                + f" bound {bound:.2e}" + (f" comp {comp:.3e}" if comp is not None else ""))
        print(line)
        if not val <= bound:
            self.bad.append(line)

    def check(self, name, ok):
        print(f"[fig] {self.tag} {name}: {'ok' if ok else 'FAILED'}")
        if not ok:
            self.bad.append(f"{self.tag} {name}")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------ the launchers' selection rules
def _fwd_ring(c):
    """K/V ring depth of the forward. Mirrors csrc/attn.hip dllm_attn_fwd (``lds = 6 * TILE64 * 2 + 3 * FWD_PAD * 4 +
    n_ktiles * (FWD_BN + 1) * 4 (+ (Sk + FWD_BM + FWD_BN) * 4 with a bias)``) and launch_fwd_t (``lds2 = lds - 2 *
    TILE64 * 2 - FWD_PAD * 4``; the 2-deep ring while ``3 * lds2 <= 160 * 1024``)."""
    assert c.D == 64 and c.dtype == BF16
    lds = 6 * 8192 + 3 * 256 * 4 + _cdiv(c.Sk, 64) * 65 * 4 + ((c.Sk + 128 + 64) * 4 if c.bias else 0)
    assert lds <= 160 * 1024
    return 2 if 3 * (lds - 2 * 8192 - 256 * 4) <= 160 * 1024 else 3


def _sq_mb(c, force):
    """Key blocks per workgroup of attn_bwd_dkdv_sq_kernel, 0 = the call takes dkdv2. Mirrors csrc/attn.hip
    dllm_attn_bwd: ``for (m = 8; m >= 2; m /= 2) if (m <= sq_cap && mb == 0 && (force || ceil(n_tiles / m) * H * B >=
    6 * cus)) mb = m`` (sq_cap = 4) and ``lut == nullptr && !causal && Sq <= 2 * K2_QT && mb > 1 && n_tiles >= 2``."""
    n = _cdiv(c.Sk, 128)
    mb = next((m for m in (4, 2) if force or _cdiv(n, m) * c.H * c.B >= 6 * _cus()), 0)
    return mb if (not c.bias and not c.causal and c.Sq <= 128 and mb > 1 and n >= 2) else 0


def _dkdv2_ring(c):
    """(stage ring depth, dynamic LDS bytes) of attn_bwd_dkdv2_kernel. Mirrors csrc/attn.hip dllm_attn_bwd (``lds =
    K2_NBUF * K2_STAGE + BWD_BK * 4 (+ (2 * (Sq + BWD_BK) + K2_QT) * 4 with a bias)``, K2_STAGE = 2 * 64 * 64 * 2 +
    2048) and launch_bwd_dkdv2_t (``!HB && (!DR || Sq <= 256) && 3 * (lds - K2_STAGE) <= 160 * 1024``: depth 2, else
    3; a depth-3 launch above 64 KB opts in through hipFuncSetAttribute)."""
    stage = 2 * 64 * 64 * 2 + 2048
    lds = 3 * stage + 128 * 4 + ((2 * (c.Sq + 128) + 64) * 4 if c.bias else 0)
    if not c.bias and (c.p == 0.0 or c.Sq <= 256) and 3 * (lds - stage) <= 160 * 1024:
        return 2, lds - stage
    return 3, lds


# ------------------------------------------------------------------------------------------------ running and checking
_built = {}


def _case(c):
    """(inputs on the GPU, fp64 reference, model, the model's figures) of a case, computed once and left unchanged."""
    key = R.case_id(c) + f"-s{c.seed}"
    if key not in _built:
        r = R.to_device(R.make_case(c), DEV)
        if c.dtype == BF16:
            ref, fig = R.ref_and_figures(r)
        else:
            ref = R.attn_ref(r.q, r.k, r.v, r.do, r.scale, r.causal, r.kpm, r.lut, r.p, seed=r.seed)
            fig = None
        _built[key] = (r, ref, fig)
    return _built[key]


def _family(c):
    return "attn_f32" if c.dtype == F32 else ("attn" if c.D == 64 else "attn_hd")


def _kernel(r, sat=False, cs=None, outs=(None, None, None), kv=None):
    """Forward + backward through the binding.  Returns a namespace o, lse, dq, dk, dv, dlut."""
    C = _ext.native()
    c = r.case
    k, v = kv if kv is not None else (r.k, r.v)
    fam = _family(c)
    base = (r.q, k, v, r.kpm, r.lut, r.scale, r.causal, r.p, r.seed)
    out = R.types.SimpleNamespace()
    if fam == "attn":
        sat_lo, sat_hi = r.sat if (sat and r.lut is not None) else (-1, -1)
        out.o, out.lse, dmask = C.attn_fwd(*base, sat_lo, sat_hi)
        cs = cs if cs is not None else (None, None, None)
        out.dq, out.dk, out.dv, out.dlut = C.attn_bwd(r.do, r.q, k, v, out.o, out.lse, r.kpm, r.lut, r.scale, r.causal,
                                                      r.p, r.seed, True, *outs, dmask, sat_lo, sat_hi, *cs)
    else:
        fwd, bwd = (C.attn_f32_fwd, C.attn_f32_bwd) if fam == "attn_f32" else (C.attn_hd_fwd, C.attn_hd_bwd)
        out.o, out.lse = fwd(*base)
        out.dq, out.dk, out.dv, out.dlut = bwd(r.do, r.q, k, v, out.o, out.lse, r.kpm, r.lut, r.scale, r.causal, r.p,
                                               r.seed, True, *outs)
    return out


def _lse_composite(r, ref):
    """The fp32 composite's own LSE error (log2 units) on these inputs: fp32 scores, torch.logsumexp."""
    c = r.case
    s = torch.matmul(r.q.float().permute(0, 2, 1, 3), r.k.float().permute(0, 2, 3, 1)) * r.scale
    if r.lut is not None:
        s = s + r.lut[:, R._rel_index(c.Sq, c.Sk, DEV)].unsqueeze(0)
    s = s.masked_fill(~R.visible(c.B, c.Sq, c.Sk, c.causal, r.kpm, DEV), float("-inf"))
    lse = torch.logsumexp(s, -1).double() / R.LN2
    live = ~ref.row_empty
    return (lse[live] - ref.lse2[live]).abs().max().item() if live.any() else 0.0


def _check_zeros(F, ref, got):
    """What the contract makes exactly zero / +inf, and finiteness of everything else."""
    e_bsh = ref.row_empty.permute(0, 2, 1)
    if ref.row_empty.any():
        F.check("empty rows: o == 0, dq == 0, lse == +inf",
                bool((got.o[e_bsh] == 0).all() and (got.dq[e_bsh] == 0).all()
                     and torch.isposinf(got.lse[ref.row_empty]).all()))
    F.check("live rows: lse finite", bool(torch.isfinite(got.lse[~ref.row_empty]).all()))
    if ref.key_dead.any():
        F.check("keys no query sees: dk == 0, dv == 0",
                bool((got.dk[ref.key_dead] == 0).all() and (got.dv[ref.key_dead] == 0).all()))
    F.check("all finite", all(bool(torch.isfinite(getattr(got, n)).all()) for n in OUTS))


def _check(F, c, got, sat=False, lse=True):
    """The kernel's outputs ``got`` against the reference of case ``c``: rows, zeros, LSE, the bias gradient."""
    r, ref, fig = _case(c)
    for n in OUTS:
        F.add(n, R.row_err(getattr(got, n), getattr(ref, n)), R.MODEL_FACTOR * fig[n], fig[n])
    _check_zeros(F, ref, got)
    if lse:
        live = ~ref.row_empty
        comp = _lse_composite(r, ref)
        err = (got.lse.double()[live] - ref.lse2[live]).abs().max().item() if live.any() else 0.0
        F.add("lse (log2 units, abs)", err, R.LSE_BOUND if comp <= R.LSE_BOUND / 4 else 4 * comp, comp=comp)
    if c.bias:
        if sat:  # saturated ranges on: the gradient is the kernels' contract per bucket and head only
            F.add("dlut per bucket", R.mass_err(R.per_bucket(got.dlut.double(), r.idx), R.per_bucket(ref.dlut, r.idx),
                                                R.per_bucket(ref.dlut_mass, r.idx)),
                  R.MODEL_FACTOR * fig["dlut_bucket"], fig["dlut_bucket"])
        else:
            F.add("dlut per entry", R.mass_err(got.dlut, ref.dlut, ref.dlut_mass), R.MODEL_FACTOR * fig["dlut"],
                  fig["dlut"])


def _run_case(c, tag, sat_too=True):
    F = Figures(f"{tag} {R.case_id(c)}")
    r, ref, fig = _case(c)
    _check(F, c, _kernel(r))
    if c.bias and sat_too and _family(c) == "attn":
        assert r.sat[0] >= 0 and r.sat[1] <= c.Sq + c.Sk - 1
        F.tag += " sat"
        _check(F, c, _kernel(r, sat=True), sat=True, lse=False)
    F.done()


def _force(monkeypatch, on):
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(attn_dkdv_sq_force=1 if on else 0))


# ------------------------------------------------------------------------------------------------- a. the flag matrix
@pytest.mark.parametrize("c", R.flag_matrix(), ids=R.case_id)
def test_flag_matrix(c, monkeypatch):
    """All 16 (bias, key padding, causal, dropout) combinations, forward and backward, at self-attention 200 x 200,
    cross 77 x 300 and causal-with-cache 130 x 200; dlut per LUT entry with the saturated ranges off and per bucket
    with them on. Unforced: every case takes the 2-deep forward ring and dkdv2."""
    _force(monkeypatch, False)
    assert _fwd_ring(c) == 2 and _sq_mb(c, False) == 0
    _run_case(c, "matrix")


# -------------------------------------------------------------------------------------------- b. forward ring depth 3
@pytest.mark.parametrize("c", R.fwd_ring3_cases(), ids=R.case_id)
def test_fwd_ring3(c, monkeypatch):
    """The forward's 3-deep K/V ring, with bias (Sk = 2500 >= 2368) and without (Sk = 5000 > 4864), causal or not, key
    padding, dropout."""
    _force(monkeypatch, False)
    assert _fwd_ring(c) == 3
    edge = R.case(c.Sq, 2304 if c.bias else 4864, B=1, H=2, bias=c.bias)  # the last length still on the 2-deep ring
    assert _fwd_ring(edge) == 2 and _fwd_ring(R.case(c.Sq, edge.Sk + 64, B=1, H=2, bias=c.bias)) == 3
    _run_case(c, "fwd-ring3")


# -------------------------------------------------------------------------------------------------- c. dkdv2 ring depth
@pytest.mark.parametrize("c,nb,optin", list(zip(R.dkdv2_cases(), (3, 2, 3), (False, False, True))),
                         ids=[R.case_id(c) for c in R.dkdv2_cases()])
def test_dkdv2_ring(c, nb, optin, monkeypatch):
    """dkdv2 at ring depth 3 without bias (dropout, Sq = 320 > 256), depth 2 (the same without dropout), and the bias
    case whose depth-3 launch needs the > 64 KB dynamic-LDS opt-in (Sq = 1100)."""
    _force(monkeypatch, False)
    assert _sq_mb(c, False) == 0
    depth, lds = _dkdv2_ring(c)
    assert depth == nb and (lds > 64 * 1024) == optin
    _run_case(c, f"dkdv2-ring{nb}")


# --------------------------------------------------------------------------------------------- d. short-query kernel
@pytest.mark.parametrize("c", R.sq_forced_cases(), ids=R.case_id)
def test_dkdv_sq_forced_mb4(c, monkeypatch):
    """attn_bwd_dkdv_sq_kernel forced (MB = 4): one and two stages (Sq 40, 100, 128), 5 key blocks (groups of 4 + 1, the
    last block ragged) and 8 (two full groups), key padding and dropout on and off."""
    _force(monkeypatch, True)
    assert _sq_mb(c, True) == 4
    _run_case(c, "sq-mb4")


def _mb2_cases():
    return R.sq_mb2_cases(_cus() if torch.cuda.is_available() else 256)


@pytest.mark.parametrize("i", [0, 1], ids=["5blocks-BHx2CUs", "4blocks-BHx3CUs"])
def test_dkdv_sq_unforced_mb2(i, monkeypatch):
    """attn_bwd_dkdv_sq_kernel as production launches it at mid-size batches, MB = 2: no route override, B sized from
    the device's CU count so that ceil(n / 4) B H < 6 CUs <= ceil(n / 2) B H (n = 5: groups 2 + 2 + 1; n = 4: 2 + 2).
    One batch row keeps 40 keys (four of its five key blocks are all padding)."""
    _force(monkeypatch, False)
    c = _mb2_cases()[i]
    n = _cdiv(c.Sk, 128)
    assert _cdiv(n, 4) * c.B * c.H < 6 * _cus() <= _cdiv(n, 2) * c.B * c.H
    assert _sq_mb(c, False) == 2
    _run_case(c, "sq-mb2")
    del _built[R.case_id(c) + f"-s{c.seed}"]  # the large references are not kept (test_colsum builds the first again)


# -------------------------------------------------------------------------------------------------- e. column sums
def _colsum(c, tag):
    C = _ext.native()
    r, ref, fig = _case(c)
    F = Figures(f"{tag} {R.case_id(c)}")
    nq, nk, HD = c.B * _cdiv(c.Sq, 128), c.B * _cdiv(c.Sk, 128), c.H * 64
    nan = float("nan")
    csq = torch.full((nq, HD), nan, device=DEV)
    pkv = torch.full((nk, 2 * HD), nan, device=DEV)  # dK | dV halves of one buffer, as ops/attention.py passes them
    plain = _kernel(r)
    got = _kernel(r, cs=(csq, pkv[:, :HD], pkv[:, HD:]))
    for n in OUTS:
        F.check(f"{n} bit-equal with and without the column sums", torch.equal(getattr(got, n), getattr(plain, n)))
    for n, part in (("cs_dq", csq), ("cs_dk", pkv[:, :HD]), ("cs_dv", pkv[:, HD:])):
        F.check(f"{n}: every partial row written", bool(torch.isfinite(part).all()))
        F.add(n, R.mass_err(part.double().sum(0), getattr(ref, n), getattr(ref, n + "_mass")), R.MODEL_FACTOR * fig[n],
              fig[n])
        # the partial rows are the per-(batch row, 128-block) sums of the STORED gradient: exact up to fp32 summation
        g = getattr(got, n[3:]).double()
        S = g.shape[1]
        blocks = torch.stack([g[b, 128 * j:min(S, 128 * (j + 1))].sum(0).reshape(-1) for b in range(c.B)
                              for j in range(_cdiv(S, 128))])
        mass = torch.stack([g[b, 128 * j:min(S, 128 * (j + 1))].abs().sum(0).reshape(-1) for b in range(c.B)
                            for j in range(_cdiv(S, 128))])
        F.add(f"{n} per block vs the stored rows", R.mass_err(part, blocks, mass), RW.COL_BOUND)
    F.done()


@pytest.mark.parametrize("c", R.colsum_cases(), ids=R.case_id)
def test_colsum(c, monkeypatch):
    """csq / csk / csv through C.attn_bwd: the dQ kernel's column sums; dkdv2's at ring depth 2 (200 x 200) and 3 (320 x
    200, p = 0.1); the short-query kernel's at MB = 4 (forced, 100 x 520)."""
    sq = c.Sq <= 128
    _force(monkeypatch, sq)
    assert _sq_mb(c, sq) == (4 if sq else 0)
    if not sq:
        assert _dkdv2_ring(c)[0] == (3 if c.Sq == 320 else 2)
    _colsum(c, "colsum")


def test_colsum_sq_mb2(monkeypatch):
    """The short-query kernel's column sums at MB = 2 (the unforced shape of test_dkdv_sq_unforced_mb2)."""
    _force(monkeypatch, False)
    c = _mb2_cases()[0]
    assert _sq_mb(c, False) == 2
    _colsum(c, "colsum-mb2")
    del _built[R.case_id(c) + f"-s{c.seed}"]


# --------------------------------------------------------------------------------------------------------- f. masks
@pytest.mark.parametrize("c", R.mask_cases(), ids=R.case_id)
def test_masks(c, monkeypatch):
    """A batch row with no valid key through forward, dQ, dkdv2 and (100 x 520, forced) dkdv_sq: exact zeros, +inf LSE,
    finite gradients, the other batch row correct. Masks that are no padded suffix (a whole 64-key tile, a whole
    128-key block, scattered keys, key 0). Causal with Sq > Sk: per the contract the first Sq - Sk rows see no key,
    and the kernels honour that (csrc/attn_params.h)."""
    sq = c.Sq <= 128
    _force(monkeypatch, sq)
    assert _sq_mb(c, sq) == (4 if sq else 0)
    r, ref, _ = _case(c)
    if c.kpm == "empty" or c.Sq > c.Sk:
        assert ref.row_empty.any()
    _run_case(c, "masks")


def test_all_padding_shard_merges(monkeypatch):
    """A key shard that is all padding merged with a live one through parallel/context.py ``_merge`` (context-parallel
    key shards can be all padding): the result is the live shard's, bit for bit, with its LSE."""
    _force(monkeypatch, False)
    C = _ext.native()
    c = R.case(200, 200, bias=True, kpm="suffix", p=0.1)
    r, ref, fig = _case(c)
    dead = torch.zeros_like(r.kpm)
    o_live, lse_live, _ = C.attn_fwd(r.q, r.k, r.v, r.kpm, r.lut, r.scale, False, r.p, r.seed)
    o_dead, lse_dead, _ = C.attn_fwd(r.q, r.k, r.v, dead, r.lut, r.scale, False, r.p, r.seed + 1)
    assert (o_dead == 0).all() and torch.isposinf(lse_dead).all()
    for first, second in (((o_dead, lse_dead), (o_live, lse_live)), ((o_live, lse_live), (o_dead, lse_dead))):
        o, lse = cp._merge(first[0].float(), first[1], second[0].float(), second[1])
        assert torch.equal(o, o_live.float()) and torch.equal(lse, lse_live)
    o, lse = cp._merge(o_dead.float(), lse_dead, o_dead.float(), lse_dead)
    assert (o == 0).all() and torch.isposinf(lse).all()
    F = Figures("merge " + R.case_id(c))
    F.add("o", R.row_err(o_live, ref.o), R.MODEL_FACTOR * fig["o"], fig["o"])
    F.done()


# ------------------------------------------------------------------------------------------- g. layouts and stores
@pytest.mark.parametrize("mode,Sq,Sk,force", [("qkv", 200, 200, False), ("q_kv", 77, 300, False),
                                              ("q_kv", 77, 300, True)])
def test_packed_modes_bit_equal(mode, Sq, Sk, force, monkeypatch):
    """The packed ``qkv`` / ``q_kv`` modes are the same kernels on other strides: o, dq, dk, dv bit-equal to the
    separate-tensor call on the same values."""
    _force(monkeypatch, force)
    c = R.case(Sq, Sk, B=2, H=3, bias=mode == "qkv", kpm="suffix", causal=mode == "qkv", p=0.1)
    r, _, _ = _case(c)
    kw = dict(scale=r.scale, causal=r.causal, key_padding_mask=r.kpm.bool(), bias_lut=r.lut, dropout_p=r.p, seed=r.seed)
    q, k, v = (t.clone().requires_grad_(True) for t in (r.q, r.k, r.v))
    o = A.attention(q, k, v, **kw)
    o.backward(r.do)
    if mode == "qkv":
        pk = torch.stack((r.q, r.k, r.v), 2).requires_grad_(True)
        o2 = A.attention_qkv(pk, **kw)
        o2.backward(r.do)
        g = (pk.grad[:, :, 0], pk.grad[:, :, 1], pk.grad[:, :, 2])
    else:
        q2 = r.q.clone().requires_grad_(True)
        pk = torch.stack((r.k, r.v), 2).requires_grad_(True)
        o2 = A.attention_q_kv(q2, pk, **kw)
        o2.backward(r.do)
        g = (q2.grad, pk.grad[:, :, 0], pk.grad[:, :, 1])
    assert torch.equal(o, o2)
    for n, a, b in zip(("dq", "dk", "dv"), (q.grad, k.grad, v.grad), g):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("c,force", [(R.case(200, 200, B=2, H=3, bias=True, causal=True, p=0.1), False),
                                     (R.case(77, 300, B=2, H=3, kpm="suffix", p=0.1), False),
                                     (R.case(77, 300, B=2, H=3, kpm="suffix", p=0.1), True)],
                         ids=lambda x: R.case_id(x) if hasattr(x, "Sq") else f"force{int(x)}")
def test_strided_outputs_and_cache_prefix(c, force, monkeypatch):
    """dq, dk, dv as views inside larger sentinel-filled buffers (extra sequence rows after S, an extra head slot; S no
    multiple of 64 / 128): the staged whole-row stores leave the sentinel untouched. k / v as prefixes of a longer
    cache buffer whose tail is NaN: nothing past Sk is read into a result. Both bit-equal to the plain call."""
    _force(monkeypatch, force)
    assert _sq_mb(c, force) == (4 if force else 0)
    r, _, _ = _case(c)
    plain = _kernel(r)
    SENT = 768.0
    bufs = [torch.full((c.B, S + 3, c.H + 1, 64), SENT, device=DEV, dtype=BF16) for S in (c.Sq, c.Sk, c.Sk)]
    views = [b[:, :S, :c.H] for b, S in zip(bufs, (c.Sq, c.Sk, c.Sk))]
    cache = [torch.full((c.B, c.Sk + 50, c.H, 64), float("nan"), device=DEV, dtype=BF16) for _ in range(2)]
    cache[0][:, :c.Sk] = r.k
    cache[1][:, :c.Sk] = r.v
    got = _kernel(r, outs=tuple(views), kv=(cache[0][:, :c.Sk], cache[1][:, :c.Sk]))
    for n in OUTS:
        assert torch.equal(getattr(got, n), getattr(plain, n)), n
    if plain.dlut is not None and c.bias:
        # the LUT gradient is accumulated with float atomics: equal up to their order
        assert R.rel_l2(got.dlut, plain.dlut) < 1e-5
    for n, b, v, S in zip(("dq", "dk", "dv"), bufs, views, (c.Sq, c.Sk, c.Sk)):
        assert v.data_ptr() == getattr(got, n).data_ptr(), n
        assert (b[:, S:] == SENT).all() and (b[:, :, c.H:] == SENT).all(), f"{n}: sentinel overwritten"


# ------------------------------------------------------------------------------- h. the other families, matrix only
@pytest.mark.parametrize("c", R.flag_matrix(D=40) + R.flag_matrix(D=128), ids=R.case_id)
def test_flag_matrix_attn_hd(c):
    """csrc/attn_hd.hip at head dims 40 (padded to 64) and 128 with the same model and bounds (it rounds at the same
    points)."""
    _run_case(c, "hd")


def _composite32(r):
    """The fp32 composite (ops.attention._reference + autograd) of an fp32 case."""
    q, k, v = (t.clone().requires_grad_(True) for t in (r.q, r.k, r.v))
    lut = r.lut.clone().requires_grad_(True) if r.lut is not None else None
    o = A._reference(q, k, v, r.scale, r.causal, r.kpm.bool() if r.kpm is not None else None, lut, r.p, r.seed)
    g = torch.autograd.grad(o, [t for t in (q, k, v, lut) if t is not None], r.do)
    return R.types.SimpleNamespace(o=o.detach(), dq=g[0], dk=g[1], dv=g[2], dlut=g[3] if lut is not None else None)


@pytest.mark.parametrize("c", R.flag_matrix(dtype=F32), ids=R.case_id)
def test_flag_matrix_attn_f32(c):
    """csrc/attn_f32.hip against fp64 at the fp32 row bound of the row-wise tests (rowwise_refs.ROW_BOUND: 1e-5); the
    fp32 composite on the same inputs must sit under a quarter of it. LSE in natural-log units."""
    r, ref, _ = _case(c)
    got, comp = _kernel(r), _composite32(r)
    F = Figures("f32 " + R.case_id(c))
    bound = RW.ROW_BOUND[F32]
    for n in OUTS:
        cv = R.row_err(getattr(comp, n), getattr(ref, n))
        F.add(n, R.row_err(getattr(got, n), getattr(ref, n)), bound, comp=cv)
        F.check(f"{n}: composite under a quarter of the bound", cv <= bound / 4)
    _check_zeros(F, ref, got)
    live = ~ref.row_empty
    F.add("lse (natural log, abs)", (got.lse.double()[live] - ref.lse2[live] * R.LN2).abs().max().item(), R.LSE_BOUND)
    if c.bias:
        cv = R.mass_err(comp.dlut, ref.dlut, ref.dlut_mass)
        F.add("dlut per entry", R.mass_err(got.dlut, ref.dlut, ref.dlut_mass), RW.COL_BOUND, comp=cv)
        F.check("dlut: composite under a quarter of the bound", cv <= RW.COL_BOUND / 4)
    F.done()
