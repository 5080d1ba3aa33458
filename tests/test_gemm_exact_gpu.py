"""GEMM kernels (csrc/gemm_fused.hip, csrc/gemm_w4.hip, its weight-gradient mode, csrc/colsum.hip) against the fp64
references of tests/gemm_refs.py on EXACT operands: per element, every launch arm.

Operands are k/8 values (``gemm_refs.dyadic``) whose products and partial sums are exact in fp32 in any order, so the
only rounding of a store-only epilogue is the final bf16 / fp32 store: those arms are compared with ``torch.equal``
against the fp64 result cast once.  The transcendental epilogues get the per-element bound derived in gemm_refs.py.  The
only numeric bounds in this module: ``torch.equal``; one bf16 ulp (a dropout scale that is no power of two; a bf16
column sum); ``2^-8 |ref| + 2^-16 (1 + |u|)`` (GELU); ``K 2^-23 mass`` (real-valued operands); ``COL_BOUND`` (fp32
column partials).  None is a share of elements.

Every test that names a launch arm asserts the mirrored launch predicate (gemm_refs.py) for its shape first; shapes
that depend on the CU count are built from the device's.  CU below = multi_processor_count // 8 * 8.

Compiled instantiation -> test that runs it
  gemm_fused staged kernel (variant 1, BK 32 x 4 stages) x BKM {NT, NN} x epilogue {0, 1, 2, 3, 4, 5, 6}
        test_pp_small[1-*]            (epilogues 7-9 and the mask / colsum outputs do not exist on variant 1)
  gemm_pp_kernel, one tile per workgroup x BKM {NT, NN} x epilogue {0, 1, 1 + mask, 2, 3, 4, 5, 6, 4/6 + colsum, 7, 9},
  NT x epilogue 8
        test_pp_small[8-*] and, through variant 9 below the predicate (few tiles, or K = 64), test_pp_small[9-*];
        epilogues 3, 4, 6 at >= 2 CU tiles: test_pp_heavy_epilogues_stay_one_tile_per_workgroup
  gemm_pp_kernel, persistent x BKM {NT, NN} x epilogue {0, 1, 1 + mask, 2, 5, 7}
        test_pp_persistent[*]
  gemm_pp_kernel, persistent, epilogue 8 (NT) and 9 (NN)
        test_pp_persistent_gated[*]
  strided operands / aux, 8-byte bias and aux pointers
        test_pp_strides_and_alignment[*]
  gemm_w4_kernel plain x BKM x BIAS x ACC x RS {0, 1, 2, 3, 257, 769}, one tile per workgroup and persistent
        test_w4_plain[*], test_w4_plain_persistent[*] (RS 769), test_w4_sched[*] (every RS), test_w4_sched_ablations[*]
        (16, 32, 64, 112, 128 of the NT no-bias form)
  gemm_w4_kernel ReLU forward (epilogue 1) x BIAS x RS {1, 257, 769}, ReLU backward (7) x RS {1, 257, 769} x mask layout
        test_w4_relu_mask[*], test_w4_drelu_from_pingpong_mask[*]
  gemm_w4_kernel GELU forward (11) x BIAS, GELU backward (12)
        test_w4_gelu[*], test_w4_dgelu_colsum[*]
  gemm_w4_kernel weight gradient (10) x RS {1, 257, 769}: splits = 1 (direct fp32 / bf16 C, beta) and > 1 (slabs +
  reduce pass), segments
        test_wgrad[*], test_wgrad_sched[*], test_wgrad_segs[*]
  colsum kernels
        test_colsum_acc[*], test_colsum_partials_acc[*]
The CE epilogues (8 / 9): tests/test_loss_kernels_gpu.py (per row / per element, persistent arm included).
"""
import functools

import pytest
import torch

import gemm_refs as R
from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops.rng import rowwise_keep_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
NAN = float("nan")


def _C():
    return _ext.native()


def _mpc():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _cus():
    return R.mirrored_cus(_mpc())


def _slack(name, value):
    """Worst observed value of a bound (captured output: pytest -rP shows it)."""
    print(f"SLACK {name} {value:.4g}")


# ------------------------------------------------------------------------------------------------- shared operands
@functools.lru_cache(maxsize=None)
def _ops(M, K, N):
    """Exact operands of one problem and its fp64 product, shared by every test on that shape and never modified:
    a [M, K] dense, w [N, K] sparse (NT weight) and its k-major copy wt [K, N], bias [N], c0 [M, N]."""
    assert K in R.EXACT_KS
    g = R.gen(DEV, M * 7 + K * 3 + N)
    a = R.dyadic((M, K), DEV, generator=g)
    w = R.dyadic((N, K), DEV, R.density_for(K), generator=g)
    bias = R.dyadic(N, DEV, generator=g)
    c0 = R.dyadic((M, N), DEV, generator=g) if M * N <= (1 << 22) else None
    assert 64.0 * (K + 2) < R.EXACT_LIMIT  # the analytic worst case of exact_headroom for any draw
    if M * N <= (1 << 20):
        assert R.exact_headroom(a, w, extra=bias.double().abs() + 1.0) < R.EXACT_LIMIT
    return {"a": a, "w": w, "wt": w.t().contiguous(), "bias": bias, "c0": c0, "u": R.gemm_ref(a, w)}


def _keep(seed, p, M, N):
    return rowwise_keep_mask(seed, p, M, N, DEV) if p > 0 else None


def _f32scale(p):
    return torch.tensor(1.0 / (1.0 - p), dtype=torch.float32, device=DEV) if p > 0 else 1.0


def _check_scaled(got, v64, live, p, msg):
    """got = v * scale where ``live`` else 0, v exact.  p in {0, 0.5}: the scale is a power of two -> bit-exact; else
    the zero pattern is exact and the values are within one bf16 ulp of bf16(fp32(v) * fp32(scale))."""
    if p in (0.0, 0.5):
        R.assert_exact(got, v64 * live.double() / (1.0 - p), msg=msg)
        return
    assert torch.equal(got != 0, live & (v64 != 0)), f"{msg}: zero pattern differs from the keep / ReLU decisions"
    exp = torch.where(live, (v64.float() * _f32scale(p)).to(BF16), torch.zeros_like(got))
    ulp = R.ulp_bf16(got, exp)
    _slack(f"{msg} ulp", ulp)
    assert ulp <= 1, f"{msg}: {ulp} bf16 ulps from bf16(fp32(v) * fp32(scale))"


# ----------------------------------------------------------------------------------------------------- guard bands
def _guard(M, N, dtype, ld, off, rows_before=1, rows_after=1):
    """(buffer, [M, N] view with row stride ld starting off elements into row rows_before) filled with NaN."""
    buf = torch.full(((M + rows_before + rows_after) * ld,), NAN, device=DEV, dtype=dtype)
    return buf, buf.as_strided((M, N), (ld, 1), rows_before * ld + off)


def _guard_intact(buf, view, msg):
    """Every element of ``buf`` outside ``view`` still holds the sentinel's bit pattern."""
    it = torch.int16 if buf.dtype == BF16 else torch.int32
    c = buf.clone()
    c.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(NAN)
    assert torch.equal(c.view(it), torch.full_like(buf, NAN).view(it)), f"{msg}: wrote outside its output view"


# ===================================================================================== ping-pong / staged gemm_fused
SMALL = [(256, 256), (256, 768), (768, 256), (1280, 768)]
SMALL_K = [64, 128, 192, 320]
FWD_ACT = {2: "gelu", 5: "gelu_new"}
BWD_ACT = {4: "gelu", 6: "gelu_new"}


def _b(o, kmajor):
    return o["wt"] if kmajor else o["w"]


def _fused_forward(o, M, K, N, variant, kmajor, epi, p, seed, bias=True, mask=False, tag=""):
    """One forward epilogue (0, 1, 2, 5) of gemm_fused on the shared operands, checked per element."""
    C = _C()
    msg = f"fused v{variant} {'NN' if kmajor else 'NT'} epi{epi} p={p} {M}x{K}x{N}{tag}"
    bv = o["bias"] if bias else None
    u = o["u"] + o["bias"].double() if bias else o["u"]
    keep = _keep(seed, p, M, N)
    if epi == 0:
        R.assert_exact(C.gemm_fused(o["a"], _b(o, kmajor), kmajor, 0, bv, None, None, 0.0, seed, variant), u, msg=msg)
    elif epi == 1:
        words = torch.full((M * N // 32,), -1, device=DEV, dtype=torch.int32) if mask else None
        h = C.gemm_fused(o["a"], _b(o, kmajor), kmajor, 1, bv, None, None, p, seed, variant, words)
        _, live = R.relu_fwd_ref(u, keep, p)
        _check_scaled(h, torch.relu(u), live, p, msg)
        if mask:
            assert torch.equal(R.decode_mask_pp(words, M, N), live), f"{msg}: stored mask words != relu > 0 & keep"
        return h, words, live
    else:
        aux = torch.full((M, N), NAN, device=DEV, dtype=BF16)
        h = C.gemm_fused(o["a"], _b(o, kmajor), kmajor, epi, bv, None, aux, p, seed, variant)
        rh, rg = R.gelu_fwd_ref(u, FWD_ACT[epi], keep, p)
        if p > 0:  # dropped elements are exact zeros
            assert not bool(h[~keep].any()) and not bool(aux[~keep].any()), f"{msg}: dropped element not zero"
        _slack(msg + " h", R.assert_elem_bound(h, rh, R.gelu_bound(rh, u), msg + " h", u))
        _slack(msg + " G", R.assert_elem_bound(aux, rg, R.gelu_bound(rg, u), msg + " G", u))
        _slack(msg + " abs-term", max(R.gelu_abs_use(h, rh, u), R.gelu_abs_use(aux, rg, u)))
        return aux
    return None


def _fused_backward(o, M, K, N, variant, kmajor, epi, p, seed, aux=None, words=None, live=None, colsum=False, tag=""):
    """One backward epilogue (3, 4, 6, 7): dH = a . b is the shared exact product."""
    C = _C()
    msg = f"fused v{variant} {'NN' if kmajor else 'NT'} epi{epi} p={p} {M}x{K}x{N}{tag}"
    dh = o["u"]
    if epi == 3:
        du = C.gemm_fused(o["a"], _b(o, kmajor), kmajor, 3, None, aux, None, p, seed, variant)
        _check_scaled(du, dh, aux != 0, p, msg)
    elif epi == 7:
        du = C.gemm_fused(o["a"], _b(o, kmajor), kmajor, 7, None, None, None, p, seed, variant, words)
        _check_scaled(du, dh, live, p, msg)
    else:
        cbuf, part = (None, None)
        if colsum:
            cbuf, part = _guard(M // 128, N, torch.float32, N, 0)
        du = C.gemm_fused(o["a"], _b(o, kmajor), kmajor, epi, None, aux, None, 0.0, seed, variant, None, part)
        ref = R.dgelu_ref(dh, aux)
        # dH exact, times a bf16 G: one fp32 product rounding (2^-24 |ref|, inside the 2^-8 |ref| term) and the store
        _slack(msg + " dU", R.assert_elem_bound(du, ref, R.BF16_REL * ref.abs() + 2.0 ** -40, msg))
        if colsum:
            _guard_intact(cbuf, part, msg + " colsum")
            pref, pmass = R.col_partials_ref(ref)
            err = R.col_err(part, pref, pmass)
            _slack(msg + " colsum", err)
            assert err < R.COL_BOUND, f"{msg}: column partials {err:.3g} of their L1 mass"


def _all_epilogues(M, K, N, variant, kmajor, persistent):
    """Every epilogue the (variant, persistent) form takes, on one shape.  ``persistent``: what the mirrored predicate
    must say for the epilogues that may run persistent; the others must come out one tile per workgroup."""
    o = _ops(M, K, N)
    T, cus = (M // 256) * (N // 256), _cus()
    pp = variant in (8, 9)
    for epi in (0, 1, 2, 5, 7):
        assert R.pp_persistent(epi, T, K, cus, variant) == persistent, (epi, T, K, cus, variant)
    for epi in (3, 4, 6):
        assert not R.pp_persistent(epi, T, K, cus, variant)
    _fused_forward(o, M, K, N, variant, kmajor, 0, 0.0, 1, bias=False)
    _fused_forward(o, M, K, N, variant, kmajor, 0, 0.0, 1, bias=True)
    h = {}
    for p in (0.0, 0.5, 0.1):
        h[p] = _fused_forward(o, M, K, N, variant, kmajor, 1, p, 5, bias=p != 0.5, mask=pp)
        if pp and (not persistent or p == 0.1):
            _fused_forward(o, M, K, N, variant, kmajor, 1, p, 5, bias=p != 0.5, mask=False, tag=" no mask")
    G = {2: _fused_forward(o, M, K, N, variant, kmajor, 2, 0.1, 31),
         5: _fused_forward(o, M, K, N, variant, kmajor, 5, 0.0, 31)}
    if persistent:
        _fused_forward(o, M, K, N, variant, kmajor, 2, 0.0, 31, bias=False)
        _fused_forward(o, M, K, N, variant, kmajor, 5, 0.5, 31)
    for p in (0.0, 0.5, 0.1):
        hh, words, live = h[p]
        if pp:
            _fused_backward(o, M, K, N, variant, kmajor, 7, p, 5, words=words, live=live)
        if not persistent:
            _fused_backward(o, M, K, N, variant, kmajor, 3, p, 5, aux=hh)
    if not persistent:
        for epi, fe in ((4, 2), (6, 5)):
            _fused_backward(o, M, K, N, variant, kmajor, epi, 0.0, 9, aux=G[fe])
            if pp:
                _fused_backward(o, M, K, N, variant, kmajor, epi, 0.0, 9, aux=G[fe], colsum=True)


def _gated(M, K, F, persistent):
    """Gated pair on the ping-pong kernel: forward (epi 8, NT, N = 2F) and backward (epi 9, NN, N = F -> [M, 2F])."""
    C, cus = _C(), _cus()
    o = _ops(M, K, 2 * F)
    assert R.pp_persistent(8, (M // 256) * (2 * F // 256), K, cus) == persistent
    gate, up = o["u"][:, :F], o["u"][:, F:]
    g1 = g2 = None
    for p in (0.0, 0.5):
        msg = f"geglu p={p} {M}x{K}x{2 * F}"
        keep = _keep(21, p, M, F)
        h, g1, g2 = C.gemm_geglu(o["a"], o["w"], p, 21)
        rh, r1, r2 = R.geglu_fwd_ref(gate, up, keep, p)
        for name, got, ref in (("h", h, rh), ("G1", g1, r1), ("G2", g2, r2)):
            bound = R.gelu_bound(ref, gate)  # u = the gate pre-activation, the argument of the transcendental
            if p > 0:
                assert not bool(got[~keep].any()), f"{msg} {name}: dropped element not zero"
            _slack(f"{msg} {name}", R.assert_elem_bound(got, ref, bound, f"{msg} {name}", gate))
            _slack(f"{msg} {name} abs-term", R.gelu_abs_use(got, ref, gate))
    # backward on its own shape: dH = a . wo with F output columns
    ob = _ops(M, K, F)
    assert R.pp_persistent(9, (M // 256) * (F // 256), K, cus) == persistent
    g1b, g2b = g1[:, :F].contiguous(), g2[:, :F].contiguous()
    du = C.gemm_dgeglu(ob["a"], ob["wt"], g1b, g2b)
    ref = R.dgeglu_ref(ob["u"], g1b, g2b)
    _slack(f"dgeglu {M}x{K}x{F}", R.assert_elem_bound(du, ref, R.BF16_REL * ref.abs() + 2.0 ** -40, "dgeglu"))


@pytest.mark.parametrize("K", SMALL_K)
@pytest.mark.parametrize("M,N", SMALL)
@pytest.mark.parametrize("variant", [1, 8, 9])
def test_pp_small(variant, M, N, K, monkeypatch):
    """Single-tile grids, tm = 1, tn = 1 and 15 tiles; 1, 2, 3 and 5 k-tiles; tile orders gemm_grp 0 (row-major), 3 (a
    last group shorter than grp) and 4; both operand layouts; every epilogue.  Variant 9 at these sizes (too few tiles,
    or K = 64) must take the one-tile-per-workgroup form: the mirror says so."""
    for grp in ((0, 3, 4) if variant != 1 else (4,)):
        monkeypatch.setenv("DLLM_ROUTE", f"gemm_grp={grp}")
        for kmajor in (False, True):
            _all_epilogues(M, K, N, variant, kmajor, persistent=False)
        if variant == 9:  # gemm_geglu / gemm_dgeglu always ask for variant 9: [M, 2N] forward, [M, N] backward
            _gated(M, K, N, persistent=False)


def _persistent_m(form, tn):
    """Rows of the persistent shapes for tn tile columns: 'uneven' = the first tile count >= 2 CU + 16 (2 and 3 tiles
    per workgroup; 8448 x 4096 on 256 CUs), 'even' = exactly 2 CU tiles."""
    cus = _cus()
    tm = -(-(2 * cus + 16) // tn) if form == "uneven" else 2 * cus // tn
    return 256 * tm


@pytest.mark.parametrize("kmajor", [False, True])
@pytest.mark.parametrize("K", [128, 192, 256])  # 2, 3, 4 k-tiles: both ring parities meet a tile boundary
@pytest.mark.parametrize("form", ["uneven", "even"])
def test_pp_persistent(form, K, kmajor):
    """Persistent ping-pong kernel: one workgroup per CU walking 2-3 tiles, the DMA stream crossing tile boundaries.
    Epilogues 0, 1 (with the mask), 2, 5, 7, all bit-exact or inside the GELU bound PER ELEMENT: one stale k-tile in one
    quadrant of one tile fails."""
    N = 4096
    M = _persistent_m(form, N // 256)
    assert (M // 256) * 16 >= 2 * _cus()
    _all_epilogues(M, K, N, 9, kmajor, persistent=True)


@pytest.mark.parametrize("K", [128, 192, 256])
@pytest.mark.parametrize("form", ["uneven", "even"])
def test_pp_persistent_gated(form, K):
    F = 2048
    M = _persistent_m(form, F // 256)  # by the backward's 8 tile columns: the forward (16) has twice the tiles
    _gated(M, K, F, persistent=True)


def test_pp_heavy_epilogues_stay_one_tile_per_workgroup():
    """Epilogues 3, 4, 6 (with colsum) load aux in the epilogue and never run persistent, even at >= 2 CU tiles with
    variant 9: asserted through the mirror, checked per element at that grid."""
    K, N = 128, 4096
    M = _persistent_m("uneven", 16)
    o, cus = _ops(M, K, N), _cus()
    for epi in (3, 4, 6):
        assert not R.pp_persistent(epi, (M // 256) * 16, K, cus, 9) and R.pp_persistent(1, (M // 256) * 16, K, cus, 9)
    g = R.gen(DEV, 3)
    hs = (R.dyadic((M, N), DEV, 0.5, generator=g)).abs()
    _fused_backward(o, M, K, N, 9, True, 3, 0.5, 6, aux=hs)
    G = (torch.rand(M, N, device=DEV, generator=g) * 1.2).to(BF16)
    _fused_backward(o, M, K, N, 9, True, 4, 0.0, 6, aux=G, colsum=True)
    _fused_backward(o, M, K, N, 9, True, 6, 0.0, 6, aux=G, colsum=False)


@pytest.mark.parametrize("variant", [1, 8, 9])
@pytest.mark.parametrize("kmajor", [False, True])
def test_pp_strides_and_alignment(variant, kmajor):
    """Operands as column slices of wider buffers (lda = K + 64, ldb = K + 8 / N + 8), aux / aux_out with row stride
    N + 4 at a pointer that is 8-byte but not 16-byte aligned inside a NaN guard band, a bias at an 8-byte-only
    offset."""
    C = _C()
    M, K, N = 512, 192, 768
    o = _ops(M, K, N)
    g = R.gen(DEV, 17)
    a_full = R.dyadic((M, K + 64), DEV, generator=g)
    a_full[:, 32:32 + K] = o["a"]
    a = a_full[:, 32:32 + K]
    if kmajor:
        b_full = R.dyadic((K, N + 8), DEV, generator=g)
        b_full[:, 8:] = o["wt"]
        b = b_full[:, 8:]
    else:
        b_full = R.dyadic((N, K + 8), DEV, generator=g)
        b_full[:, 8:] = o["w"]
        b = b_full[:, 8:]
    assert a.stride(0) == K + 64 and b.stride(0) == (N if kmajor else K) + 8 and C.gemm_fused_supported(a, b, kmajor)
    bias_buf = R.dyadic(N + 4, DEV, generator=g)
    bias = bias_buf[4:]
    assert bias.data_ptr() % 16 == 8
    u = o["u"] + bias.double()
    msg = f"strided v{variant} {'NN' if kmajor else 'NT'}"
    R.assert_exact(C.gemm_fused(a, b, kmajor, 0, bias, None, None, 0.0, 0, variant), u, msg=msg + " epi0")
    for epi, p in ((2, 0.5), (5, 0.0)):
        buf, aux = _guard(M, N, BF16, N + 4, 4, rows_before=2)
        assert aux.data_ptr() % 16 == 8 and aux.stride(0) == N + 4
        h = C.gemm_fused(a, b, kmajor, epi, bias, None, aux, p, 31, variant)
        _guard_intact(buf, aux, f"{msg} epi{epi} aux_out")
        keep = _keep(31, p, M, N)
        rh, rg = R.gelu_fwd_ref(u, FWD_ACT[epi], keep, p)
        R.assert_elem_bound(h, rh, R.gelu_bound(rh, u), f"{msg} epi{epi} h", u)
        R.assert_elem_bound(aux, rg, R.gelu_bound(rg, u), f"{msg} epi{epi} G", u)
        # ... and read back through the same strided view by the backward epilogues
        for bepi in (4, 6):
            du = C.gemm_fused(a, b, kmajor, bepi, None, aux, None, 0.0, 0, variant)
            ref = R.dgelu_ref(o["u"], aux)
            R.assert_elem_bound(du, ref, R.BF16_REL * ref.abs() + 2.0 ** -40, f"{msg} epi{bepi} strided aux")
    hbuf, hs = _guard(M, N, BF16, N + 4, 4, rows_before=2)
    hs.copy_(R.dyadic((M, N), DEV, 0.5, generator=g).abs())
    du = C.gemm_fused(a, b, kmajor, 3, None, hs, None, 0.5, 0, variant)
    _check_scaled(du, o["u"], hs != 0, 0.5, msg + " epi3 strided H")


# ========================================================================================================= gemm_w4
W4_SMALL = [(8, 64, 8), (256, 64, 256), (257, 64, 520), (300, 192, 264)]


def _w4_persistent_shape():
    """M = 256 (CU / 8) + 40, N = 2000: CU + 8 tiles, ragged on both edges."""
    cus = _cus()
    return 256 * (cus // 8) + 40, 2000


def _w4_plain(M, K, N, kmajor, bias, acc, persist, expect_persistent, msg):
    C = _C()
    o = _ops(M, K, N)
    T = -(-M // 256) * -(-N // 256)
    assert R.w4_persistent(0, T, K, persist, _cus()) == expect_persistent, (T, K, persist)
    bv = o["bias"] if bias else None
    buf, out = _guard(M, N, BF16, N + 16, 8)
    c0 = None
    if acc:
        c0 = R.dyadic((M, N), DEV, generator=R.gen(DEV, 5))
        out.copy_(c0)
    b = _b(o, kmajor)
    assert C.gemm_w4_supported(o["a"], b, kmajor)
    got = C.gemm_w4(o["a"], b, kmajor, bv, out, acc, -1, persist)
    assert got.data_ptr() == out.data_ptr()
    _guard_intact(buf, out, msg)
    ref = o["u"] + (bv.double() if bias else 0.0) + (c0.double() if acc else 0.0)
    R.assert_exact(out, ref, msg=msg)
    if not acc:  # the binding's own allocation
        R.assert_exact(C.gemm_w4(o["a"], b, kmajor, bv, None, False, -1, persist), ref, msg=msg + " (own out)")


@pytest.mark.parametrize("bias,acc", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("kmajor", [False, True])
@pytest.mark.parametrize("M,K,N", W4_SMALL)
def test_w4_plain(M, K, N, kmajor, bias, acc):
    for persist in (False, True):
        _w4_plain(M, K, N, kmajor, bias, acc, persist, False, f"w4 {M}x{K}x{N} NN={kmajor} bias={bias} acc={acc}")


@pytest.mark.parametrize("bias,acc", [(False, False), (True, True)])
@pytest.mark.parametrize("kmajor", [False, True])
@pytest.mark.parametrize("K,persist,walks", [(128, True, True), (192, True, True), (64, True, False),
                                             (128, False, False)])
def test_w4_plain_persistent(K, persist, walks, kmajor, bias, acc):
    """CU + 8 tiles, ragged on both edges: one workgroup per CU walking 1-2 tiles (K >= 128 and persist), else — K = 64
    with persist, or persist off — one tile per workgroup, as the mirror says."""
    M, N = _w4_persistent_shape()
    assert -(-M // 256) * -(-N // 256) == _cus() + 8
    _w4_plain(M, K, N, kmajor, bias, acc, persist, walks, f"w4 persistent-shape K={K} persist={persist} NN={kmajor}")


@pytest.mark.parametrize("rs", R.W4_SCHED_COMPILED)
def test_w4_sched(rs, monkeypatch):
    """Every compiled schedule of the plain forms (DLLM_ROUTE w4_sched), small ragged and persistent: bit-exact."""
    monkeypatch.setenv("DLLM_ROUTE", f"w4_sched={rs}")
    Mp, Np = _w4_persistent_shape()
    for kmajor in (False, True):
        for bias, acc in ((False, False), (True, True)):
            assert R.w4_sched(rs, kmajor, bias, acc) == rs
            _w4_plain(300, 192, 264, kmajor, bias, acc, True, False, f"w4_sched={rs} small NN={kmajor}")
            _w4_plain(Mp, 192, Np, kmajor, bias, acc, True, True, f"w4_sched={rs} persistent NN={kmajor}")


@pytest.mark.parametrize("rs", R.W4_SCHED_ABLATIONS)
def test_w4_sched_ablations(rs, monkeypatch):
    """The timing ablations of the plain no-bias NT forward delete k-loop DMAs (16), fragment reads (32), the k-loop
    wait and barrier (64) or the epilogue stores (128) — csrc/gemm_w4.hip says their results are garbage, so there is no
    product to compare.  What still holds is checked: they select themselves only for that form, leave the guard band
    around the output alone, 128 stores nothing at all, and every other form under the same route value is exact."""
    monkeypatch.setenv("DLLM_ROUTE", f"w4_sched={rs}")
    C = _C()
    Mp, Np = _w4_persistent_shape()
    for (M, K, N), walks in (((300, 192, 264), False), ((Mp, 192, Np), True)):
        o = _ops(M, K, N)
        assert R.w4_sched(rs) == rs and R.w4_persistent(0, -(-M // 256) * -(-N // 256), K, True, _cus()) == walks
        buf, out = _guard(M, N, BF16, N + 16, 8)
        C.gemm_w4(o["a"], o["w"], False, None, out, False, -1, True)
        torch.cuda.synchronize()
        _guard_intact(buf, out, f"w4_sched={rs}")
        if rs & 128:
            assert bool(out.isnan().all()), "no-store ablation stored"
        # the same route value on the forms the ablations are not built for: the default-schedule family, exact
        assert R.w4_sched(rs, True, False, False) == rs & 3 and R.w4_sched(rs, False, True, False) == rs & 3
        R.assert_exact(C.gemm_w4(o["a"], o["wt"], True, None, None, False, -1, True), o["u"], msg=f"w4_sched={rs} NN")
        R.assert_exact(C.gemm_w4(o["a"], o["w"], False, o["bias"], None, False, -1, True), o["u"] + o["bias"].double(),
                       msg=f"w4_sched={rs} bias")


def _w4_relu(M, K, N, p, bias, persist, walks, rs):
    """ReLU + dropout forward writing its mask, then the backward through that mask."""
    C = _C()
    o = _ops(M, K, N)
    tm, tn = -(-M // 256), -(-N // 256)
    for epi in (1, 7):
        assert R.w4_persistent(epi, tm * tn, K, persist, _cus()) == walks
    msg = f"w4 relu {M}x{K}x{N} p={p} bias={bias} persist={persist} rs={rs}"
    nw = C.gemm_w4_mask_words(M, N)
    assert nw == tm * tn * 2048
    words = torch.full((nw + 64,), 0x5A5A5A5A, device=DEV, dtype=torch.int32)
    bv = o["bias"] if bias else None
    u = o["u"] + o["bias"].double() if bias else o["u"]
    h = C.gemm_w4(o["a"], o["w"], False, bv, None, False, -1, persist, 1, p, 1234, words)
    keep = _keep(1234, p, M, N)
    _, live = R.relu_fwd_ref(u, keep, p)
    _check_scaled(h, torch.relu(u), live, p, msg)
    dec = R.decode_mask_w4(words, M, N)
    assert torch.equal(dec[:M, :N], live), f"{msg}: stored mask words != relu > 0 & keep"
    # csrc/gemm_params.h: bits of columns >= N are 0, bits of rows >= M unspecified, words past the last tile untouched
    assert not bool(dec[:, N:].any()), f"{msg}: mask bits set in columns >= N"
    assert bool((words[nw:] == 0x5A5A5A5A).all()), f"{msg}: mask words past the last tile written"
    du = C.gemm_w4(o["a"], o["wt"], True, None, None, False, -1, persist, 7, p, 1234, words)
    _check_scaled(du, o["u"], live, p, msg + " backward")


@pytest.mark.parametrize("rs", [1, 257, 769])
@pytest.mark.parametrize("p,bias", [(0.0, True), (0.5, False), (0.1, True)])
@pytest.mark.parametrize("shape", ["ragged", "ragged_k64", "persistent", "persistent_k64"])
def test_w4_relu_mask(shape, p, bias, rs, monkeypatch):
    monkeypatch.setenv("DLLM_ROUTE", f"w4_sched={rs}")
    Mp, Np = _w4_persistent_shape()
    M, K, N, walks = {"ragged": (300, 192, 264, False), "ragged_k64": (257, 64, 520, False),
                      "persistent": (Mp, 128, Np, True), "persistent_k64": (Mp, 64, Np, False)}[shape]
    _w4_relu(M, K, N, p, bias, True, walks, rs)


@pytest.mark.parametrize("p", [0.0, 0.5, 0.1])
@pytest.mark.parametrize("shape", ["small", "persistent"])
def test_w4_drelu_from_pingpong_mask(shape, p):
    """The w4 ReLU backward reading the mask a ping-pong ReLU forward wrote (mask_pp): exact against the decoded
    bits."""
    C = _C()
    M, N = (768, 512) if shape == "small" else (256 * (_cus() // 8 + 1), 2048)
    K = 192
    walks = shape == "persistent"
    assert R.w4_persistent(7, (M // 256) * (N // 256), K, True, _cus()) == walks
    o = _ops(M, K, N)
    _, words, live = _fused_forward(o, M, K, N, 8, False, 1, p, 77, bias=True, mask=True)
    du = C.gemm_w4(o["a"], o["wt"], True, None, None, False, -1, True, 7, p, 77, words, True)
    _check_scaled(du, o["u"], live, p, f"w4 drelu mask_pp {M}x{N} p={p}")


@pytest.mark.parametrize("p,bias", [(0.0, False), (0.5, True), (0.1, True)])
@pytest.mark.parametrize("shape", ["ragged", "persistent", "persistent_k64"])
def test_w4_gelu(shape, p, bias):
    """W4_EPI_GELU: h and the derivative output inside a NaN guard band, per element."""
    C = _C()
    Mp, Np = _w4_persistent_shape()
    M, K, N, walks = {"ragged": (300, 192, 264, False), "persistent": (Mp, 128, Np, True),
                      "persistent_k64": (Mp, 64, Np, False)}[shape]
    assert R.w4_persistent(11, -(-M // 256) * -(-N // 256), K, True, _cus()) == walks
    o = _ops(M, K, N)
    msg = f"w4 gelu {M}x{K}x{N} p={p} bias={bias}"
    bv = o["bias"] if bias else None
    u = o["u"] + o["bias"].double() if bias else o["u"]
    buf, aux = _guard(M, N, BF16, N + 16, 8)
    h = C.gemm_w4(o["a"], o["w"], False, bv, None, False, -1, True, 11, p, 31, None, False, None, aux)
    _guard_intact(buf, aux, msg + " aux_out")
    keep = _keep(31, p, M, N)
    rh, rg = R.gelu_fwd_ref(u, "gelu", keep, p)
    if p > 0:
        assert not bool(h[~keep].any()) and not bool(aux[~keep].any()), f"{msg}: dropped element not zero"
    _slack(msg + " h", R.assert_elem_bound(h, rh, R.gelu_bound(rh, u), msg + " h", u))
    _slack(msg + " G", R.assert_elem_bound(aux, rg, R.gelu_bound(rg, u), msg + " G", u))
    _slack(msg + " abs-term", max(R.gelu_abs_use(h, rh, u), R.gelu_abs_use(aux, rg, u)))


@pytest.mark.parametrize("shape", ["small", "ragged_n", "even_m", "largest"])
def test_w4_dgelu_colsum(shape):
    """W4_EPI_DGELU: dU = dH * G per element and the per-128-row column partials against their L1 mass; never
    persistent (the mirror), also at CU + 8 tiles."""
    C = _C()
    M, K, N = {"small": (384, 192, 512), "ragged_n": (640, 64, 520), "even_m": (512, 128, 264),
               "largest": (256 * (_cus() // 8) + 128, 128, 2000)}[shape]
    T = -(-M // 256) * -(-N // 256)
    assert not R.w4_persistent(12, T, K, True, _cus()) and (shape != "largest" or T == _cus() + 8)
    o = _ops(M, K, N)
    G = (torch.rand(M, N + 8, device=DEV, generator=R.gen(DEV, 9)) * 1.2).to(BF16)[:, :N]  # a strided view
    cbuf, part = _guard(M // 128, N, torch.float32, N, 0)
    du = C.gemm_w4(o["a"], o["wt"], True, None, None, False, -1, False, 12, 0.0, 0, None, False, G, None, part)
    _guard_intact(cbuf, part, "w4 dgelu colsum")
    ref = R.dgelu_ref(o["u"], G)
    _slack(f"w4 dgelu {shape} dU", R.assert_elem_bound(du, ref, R.BF16_REL * ref.abs() + 2.0 ** -40, "w4 dgelu"))
    pref, pmass = R.col_partials_ref(ref)
    err = R.col_err(part, pref, pmass)
    _slack(f"w4 dgelu {shape} colsum", err)
    assert err < R.COL_BOUND, err


def test_w4_real_valued_operands():
    """One case per family on realistic magnitudes (randn): the derived forward bound 2^-8 |ref| + K 2^-23 mass, per
    element, at the persistent shapes."""
    C = _C()
    g = R.gen(DEV, 1)
    for fused in (False, True):
        M, N = (_persistent_m("uneven", 16), 4096) if fused else _w4_persistent_shape()
        K = 256
        a = torch.randn(M, K, device=DEV, generator=g).to(BF16)
        w = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).to(BF16)
        bias = torch.randn(N, device=DEV, generator=g).to(BF16)
        ref, mass = R.gemm_ref(a, w, False, bias), R.gemm_mass(a, w, False, bias)
        got = C.gemm_fused(a, w, False, 0, bias, None, None, 0.0, 0, 9) if fused else C.gemm_w4(a, w, False, bias)
        _slack(f"randn {'pp' if fused else 'w4'}", R.assert_elem_bound(got, ref, R.real_bound(ref, mass, K), "randn"))


# ================================================================================================= weight gradient
def _wg_ops(K, M, N, pad):
    g = R.gen(DEV, K + M + N + pad)
    a_full = R.dyadic((K, M + pad), DEV, generator=g)
    a = a_full[:, pad:] if pad else a_full
    b = R.dyadic((K, N), DEV, R.density_for(K), generator=g)
    assert 64.0 * (K + 1) < R.EXACT_LIMIT and K in R.EXACT_KS
    return a, b, R.dyadic((M, N), DEV, generator=g)


def _wgrad(K, M, N, dtype, beta, splits_req, pad, msg):
    C = _C()
    a, b, c0 = _wg_ops(K, M, N, pad)
    splits, kchunk = R.wgrad_split_plan(K, M, N, a.stride(0), b.stride(0), _mpc(), splits_req)
    cbuf, c = _guard(M, N, dtype, N + 8, 8)
    c.copy_(c0)  # beta 0 must overwrite it
    assert C.gemm_wgrad_supported(a, b, c)
    used = C.gemm_wgrad(a, b, c, beta, -1, splits_req)
    assert used == splits, f"{msg}: {used} splits, the mirrored plan says {splits} (chunks of {kchunk})"
    _guard_intact(cbuf, c, msg)
    R.assert_exact(c, R.wgrad_ref(a, b, c0, beta), msg=msg)
    return splits, kchunk


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
@pytest.mark.parametrize("beta", [False, True])
@pytest.mark.parametrize("M", [8, 264, 520])
@pytest.mark.parametrize("N", [256, 768])
def test_wgrad(M, N, beta, dtype):
    """Ragged last M tile TOGETHER with a short last split: K = 960 in 3 chunks of 320 (auto) / 2 of 512 + 448 / one
    split of 15 k-tiles; K = 320 (one split, 5 k-tiles); A as a column slice of a wider buffer."""
    for K, req, pad in ((960, 0, 0), (960, 1, 0), (960, 3, 0), (960, 2, 64), (320, 0, 0), (320, 0, 64)):
        msg = f"wgrad {K}x{M}x{N} {dtype} beta={beta} req={req} pad={pad}"
        splits, kchunk = _wgrad(K, M, N, dtype, beta, req, pad, msg)
        if req in (1, 2, 3):
            assert splits == req
        if K == 960 and req == 2:
            assert kchunk * splits > K  # the short last split the case is about
        if K == 320 or req == 1:
            assert splits == 1


@pytest.mark.parametrize("rs", [1, 257])
def test_wgrad_sched(rs, monkeypatch):
    """The weight-gradient mode's other two schedules (769 is the default every other test runs)."""
    monkeypatch.setenv("DLLM_ROUTE", f"w4_sched={rs}")
    for req in (1, 3):
        _wgrad(960, 264, 256, torch.float32, True, req, 0, f"wgrad w4_sched={rs} req={req}")


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
@pytest.mark.parametrize("beta", [False, True])
@pytest.mark.parametrize("nseg,rows", [(1, 64), (5, 192), (32, 64)])
def test_wgrad_segs(nseg, rows, beta, dtype):
    C = _C()
    M, N = 264, 256
    g = R.gen(DEV, nseg * rows)
    assert nseg * rows in R.EXACT_KS or nseg * rows == 64
    as_ = [R.dyadic((rows, M), DEV, generator=g) for _ in range(nseg)]
    bs = [R.dyadic((rows, N), DEV, R.density_for(nseg * rows), generator=g) for _ in range(nseg)]
    c0 = R.dyadic((M, N), DEV, generator=g)
    cbuf, c = _guard(M, N, dtype, N + 8, 8)
    c.copy_(c0)
    splits, kchunk, chunks = R.wgrad_segs_plan(nseg, rows, M, N, M, N, _mpc())
    used = C.gemm_wgrad_segs(as_, bs, c, beta)
    assert used == splits, (used, splits, kchunk, chunks)
    _guard_intact(cbuf, c, "wgrad_segs")
    R.assert_exact(c, R.wgrad_ref(torch.cat(as_), torch.cat(bs), c0, beta), msg=f"wgrad_segs {nseg}x{rows} beta={beta}")


# ===================================================================================================== column sums
@pytest.mark.parametrize("dtype", [torch.float32, BF16])
@pytest.mark.parametrize("T,N,off", [(37, 770, 2), (1000, 520, 0), (4099, 1024, 0), (4099, 258, 2)])
def test_colsum_acc(T, N, off, dtype):
    """out += x.sum(0) on exact rows: every partial sum is a multiple of 1/8 below 2^24 / 8, so the fp32 result is exact
    whatever the order; a bf16 ``out`` is that sum rounded once — within one bf16 ulp is asserted, as the kernel may
    round its fp32 total and the previous ``out`` separately."""
    g = R.gen(DEV, T + N)
    x_full = R.dyadic((T, N + 8), DEV, generator=g)
    x = x_full[:, off:off + N]
    out0 = R.dyadic(N, DEV, generator=g).to(dtype)
    buf, out = _guard(1, N, dtype, N, 0)
    out = out.view(N)
    out.copy_(out0)
    _C().colsum_acc(x, out)
    _guard_intact(buf, out.view(1, N), "colsum_acc")
    ref = out0.double() + x.double().sum(0)
    assert 8.0 * (x.double().abs().sum(0).max().item() + 1.0) < R.EXACT_LIMIT
    if dtype == torch.float32:
        R.assert_exact(out.view(1, N), ref.view(1, N), msg=f"colsum_acc {T}x{N}")
    else:
        ulp = R.ulp_bf16(out, ref)
        _slack(f"colsum_acc bf16 {T}x{N} ulp", ulp)
        assert ulp <= 1


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
@pytest.mark.parametrize("G,d", [(1, 8), (66, 520), (515, 768), (4100, 264)])
def test_colsum_partials_acc(G, d, dtype):
    """out += part.sum(0) on randn partials: |error| against the column's L1 mass (``col_err``), and for a bf16 ``out``
    one bf16 ulp of the exact sum on top."""
    g = R.gen(DEV, G + d)
    part = torch.randn(G, d, device=DEV, generator=g)
    out0 = torch.randn(d, device=DEV, generator=g).to(dtype)
    buf, out = _guard(1, d, dtype, d, 0)
    out = out.view(d)
    out.copy_(out0)
    _C().colsum_partials_acc(part, out)
    _guard_intact(buf, out.view(1, d), "colsum_partials_acc")
    ref = out0.double() + part.double().sum(0)
    mass = out0.double().abs() + part.double().abs().sum(0)
    if dtype == torch.float32:
        err = R.col_err(out, ref, mass)
        _slack(f"colsum_partials_acc {G}x{d}", err)
        assert err < R.COL_BOUND, err
    else:  # fp32 total inside COL_BOUND of the mass, then one rounding to bf16
        lim = R.COL_BOUND * mass + R.BF16_REL * ref.abs()
        _slack(f"colsum_partials_acc bf16 {G}x{d}", R.assert_elem_bound(out.view(1, d), ref.view(1, d), lim.view(1, d)))
