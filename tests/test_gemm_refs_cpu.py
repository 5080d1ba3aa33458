"""The oracle of tests/test_gemm_exact_gpu.py (tests/gemm_refs.py), validated without a GPU.

* the fp64 references agree with plain fp32 torch composites on randn data and with the package's own activation
  reference (``activations._act_ref`` and its autograd);
* ``dyadic`` operands meet the exactness precondition at every reduction length the GPU tests use, and an fp32 matmul of
  them, summed in another order, equals the fp64 one bit for bit;
* the mask decoders invert scalar encoders written from the layout comments of csrc/gemm_params.h;
* the launch-predicate mirrors reproduce the split counts documented above csrc/bind_gemm.cpp ``wgrad_splits``;
* SENSITIVITY: the smallest plausible kernel faults, injected into a correct synthetic output at the persistent
  ping-pong shape (8448 x 4096), are rejected by the new checks — and, as a record of the gap they close, accepted by
  the whole-tensor numbers the GEMM tests used so far (``_rel < 8e-3``, ``_close(2e-2, 2e-2)`` at a 0.1 % share).
"""
import math

import pytest
import torch

import gemm_refs as R
from distributed_llms_example_amd.ops import activations
from distributed_llms_example_amd.ops.rng import rowwise_keep_mask

CPU = "cpu"
BF16 = torch.bfloat16


# ------------------------------------------------------------------------------- the whole-tensor numbers used so far
def old_rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def old_close_share(a, b, rtol=2e-2, atol=2e-2):
    a, b = a.float(), b.float()
    return ((a - b).abs() > atol + rtol * b.abs()).float().mean().item()


def old_accepts(got, ref):
    return old_rel(got, ref) < 8e-3 and old_close_share(got, ref) < 1e-3


# ---------------------------------------------------------------------------------------- references vs fp32 composites
def _randn_ops(M=96, K=160, N=72, seed=0):
    g = R.gen(CPU, seed)
    a = torch.randn(M, K, generator=g).to(BF16)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF16)
    bias = (0.5 * torch.randn(N, generator=g)).to(BF16)
    c0 = torch.randn(M, N, generator=g).to(BF16)
    return a, w, bias, c0


def _fp32_close(got64, ref32, scale=None):
    s = ref32.double().abs().max().item() if scale is None else scale
    assert (got64 - ref32.double()).abs().max().item() <= 2e-5 * max(s, 1.0)


@pytest.mark.parametrize("kmajor", [False, True])
def test_gemm_ref_matches_fp32_composite(kmajor):
    a, w, bias, c0 = _randn_ops()
    b = w.t().contiguous() if kmajor else w
    u32 = a.float() @ w.float().t()
    _fp32_close(R.gemm_ref(a, b, kmajor), u32)
    _fp32_close(R.gemm_ref(a, b, kmajor, bias, c0), u32 + bias.float() + c0.float())
    mass = R.gemm_mass(a, b, kmajor, bias, c0)
    assert (mass >= R.gemm_ref(a, b, kmajor, bias, c0).abs() - 1e-12).all()
    # the weight gradient is the same product with token-major operands
    _fp32_close(R.wgrad_ref(a, c0.new_zeros(a.shape[0], 8) + 1, None, False), a.float().t() @ torch.ones(a.shape[0], 8))
    _fp32_close(R.wgrad_ref(a.t().contiguous(), w.t().contiguous(), c0[:a.shape[0], :w.shape[0]], True),
                a.float() @ w.float().t() + c0.float())


@pytest.mark.parametrize("act", ["gelu", "gelu_new"])
def test_activation_pair_matches_package_reference_and_autograd(act):
    u = torch.linspace(-9.0, 9.0, 4001, dtype=torch.float64)
    ud = u.clone().requires_grad_(True)
    y = activations._act_ref(ud, act)
    (dy,) = torch.autograd.grad(y.sum(), ud)
    g, dg = R.phi_pair(u, act)
    assert (g - y.detach()).abs().max().item() < 1e-12
    assert (dg - dy).abs().max().item() < 1e-12
    # fp32 composite of the same thing (what the existing GPU tests compare with)
    y32 = activations._act_ref(u.float(), act)
    assert (g - y32.double()).abs().max().item() < 2e-6


def test_forward_epilogue_refs_match_fp32_composites():
    a, w, bias, _ = _randn_ops(M=64, K=128, N=96, seed=1)
    M, N, p, seed = 64, 96, 0.1, 77
    keep = rowwise_keep_mask(seed, p, M, N, CPU)
    u = R.gemm_ref(a, w, False, bias)
    u32 = a.float() @ w.float().t() + bias.float()
    h, live = R.relu_fwd_ref(u, keep, p)
    _fp32_close(h, torch.relu(u32) * keep / (1 - p))
    assert torch.equal(live, (torch.relu(u32) > 0) & keep)
    for act in ("gelu", "gelu_new"):
        h, G = R.gelu_fwd_ref(u, act, keep, p)
        uf = u32.clone().requires_grad_(True)
        activations._act_ref(uf, act).sum().backward()
        _fp32_close(h, activations._act_ref(u32, act) * keep / (1 - p))
        _fp32_close(G, uf.grad * keep / (1 - p))
    # gated trio against autograd of dropout(gelu_new(gate) * up)
    F = N // 2
    keep = rowwise_keep_mask(seed, p, M, F, CPU)
    gate, up = u[:, :F], u[:, F:]
    h, g1, g2 = R.geglu_fwd_ref(gate, up, keep, p)
    gd, upd = gate.clone().requires_grad_(True), up.clone().requires_grad_(True)
    y = activations._act_ref(gd, "gelu_new") * upd * keep / (1 - p)
    dh = torch.randn(M, F, dtype=torch.float64, generator=R.gen(CPU, 2))
    y.backward(dh)
    assert (h - y.detach()).abs().max().item() < 1e-12
    assert (dh * g1 - gd.grad).abs().max().item() < 1e-12 and (dh * g2 - upd.grad).abs().max().item() < 1e-12
    both = R.dgeglu_ref(dh, g1, g2)
    assert both.shape == (M, 2 * F) and torch.equal(both[:, F:], dh * g2)


def test_backward_epilogue_and_partial_refs():
    g = R.gen(CPU, 3)
    dh = torch.randn(256, 48, dtype=torch.float64, generator=g)
    hs = torch.relu(torch.randn(256, 48, generator=g)).to(BF16)
    du = R.drelu_ref(dh, hs != 0, 0.1)
    _fp32_close(du, dh.float() * (hs.float() != 0) / 0.9)
    G = torch.randn(256, 48, generator=g).to(BF16)
    _fp32_close(R.dgelu_ref(dh, G), dh.float() * G.float())
    part, mass = R.col_partials_ref(du)
    assert part.shape == (2, 48)
    _fp32_close(part, du.float().view(2, 128, 48).sum(1))
    assert R.col_err(part, part, mass) == 0.0
    assert R.COL_BOUND == 1e-5  # the bound of tests/rowwise_refs.py, imported not copied


# --------------------------------------------------------------------------------------------------- exact operands
@pytest.mark.parametrize("K", R.EXACT_KS)
def test_dyadic_operands_are_exact(K):
    g = R.gen(CPU, K)
    M = N = 128
    for density in {R.density_for(K), 1.0}:
        a = R.dyadic((M, K), CPU, generator=g)
        w = R.dyadic((N, K), CPU, density, generator=g)
        bias, c0 = R.dyadic(N, CPU, generator=g), R.dyadic((M, N), CPU, generator=g)
        assert a.dtype == BF16 and torch.equal(a.double() * 8, (a.double() * 8).round()) and a.abs().max() <= 1
        assert torch.equal(a, a.float().to(BF16))  # survives the bf16 cast unchanged
        head = R.exact_headroom(a, w, extra=bias.double().abs() + c0.double().abs())
        assert head <= 64.0 * (K + 2) < R.EXACT_LIMIT, head  # the analytic worst case of any draw
        u64 = R.gemm_ref(a, w, False, bias, c0)
        perm = torch.randperm(K, generator=g)
        u32 = a.float()[:, perm] @ w.float()[:, perm].t() + bias.float() + c0.float()
        assert torch.equal(u32.double(), u64)
        # split-K in fp32, any chunking: the same bits again
        parts = sum(a.float()[:, k:k + 64] @ w.float()[:, k:k + 64].t() for k in range(0, K, 64))
        assert torch.equal((parts + bias.float() + c0.float()).double(), u64)
    if K >= 960:  # the pre-activations sit in GELU's curved region, both signs
        u = R.gemm_ref(a, R.dyadic((N, K), CPU, R.density_for(K), generator=g))
        assert 1.5 < u.std().item() < 2.8 and ((u.abs() < 3).double().mean().item() > 0.75)
        assert (u > 0).any() and (u < 0).any()


def test_exact_and_ulp_metrics():
    x = torch.tensor([1.0, -1.0, 0.0, 3.140625, 1e-3], dtype=torch.float64)
    got = x.float().to(BF16)
    R.assert_exact(got, x)
    assert R.ulp_bf16(got, x) == 0
    up = (got.view(torch.int16) + torch.tensor([1, 0, 0, 0, 0], dtype=torch.int16)).view(BF16)
    assert R.ulp_bf16(up, x) == 1 and R.exact_mismatch(up, x) is not None
    tiny = torch.tensor([2.0 ** -133], dtype=torch.float32).to(BF16)  # smallest subnormal: one ulp from +-0
    assert R.ulp_bf16(tiny, torch.zeros(1)) == 1 and R.ulp_bf16(-tiny, tiny.double()) == 2
    with pytest.raises(AssertionError, match="tile"):
        R.assert_exact(up, x, msg="named region")
    ref = torch.zeros(512, 512, dtype=torch.float64)
    got = ref.clone()
    got[300, 200] = 1.0
    worst, where, err, lim = R.elem_bound(got, ref, torch.full_like(ref, 0.5))
    assert worst == 2.0 and where == {"tile": (1, 0), "quadrant": (0, 3), "row": 300, "col": 200}
    with pytest.raises(AssertionError):
        R.assert_elem_bound(got, ref, torch.full_like(ref, 0.5))
    got[300, 200] = float("nan")
    assert R.elem_bound(got, ref, torch.full_like(ref, 0.5))[0] == math.inf


# ---------------------------------------------------------------------------------------------------- mask decoders
def _encode_w4(live):
    """Scalar encoder from the comment on GemmW4Params::mask (csrc/gemm_params.h), one element at a time."""
    Mp, Np = live.shape
    tm, tn = Mp // 256, Np // 256
    words = [0] * (tm * tn * 2048)
    for row, col in live.nonzero().tolist():
        tr, tc, r_, c_ = row // 256, col // 256, row % 256, col % 256
        wm, i, rl = r_ // 128, (r_ % 128) // 16, r_ % 16
        wn, j, qd, r = c_ // 128, (c_ % 128) // 16, (c_ % 16) // 4, c_ % 4
        tid = 64 * (2 * wm + wn) + 16 * qd + rl
        words[((tr * tn + tc) * 256 + tid) * 8 + i] |= 1 << (2 * j + (r >> 1) + 16 * (r & 1))
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32)


def _encode_pp(live):
    """Scalar encoder from the comment on GemmFusedParams::mask (csrc/gemm_params.h)."""
    M, N = live.shape
    tn = N // 256
    words = [0] * (M * N // 32)
    for row, col in live.nonzero().tolist():
        tr, tc, r_, c_ = row // 256, col // 256, row % 256, col % 256
        wm, i, rl = r_ // 128, (r_ % 128) // 16, r_ % 16
        wn, j, q, r = c_ // 64, (c_ % 64) // 16, (c_ % 16) // 4, c_ % 4
        tid = 64 * (4 * wm + wn) + 16 * q + rl
        words[((tr * tn + tc) * 512 + tid) * 4 + (i >> 1)] |= 1 << (16 * (i & 1) + 4 * j + r)
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32)


def test_mask_decoders_invert_the_documented_layouts():
    g = R.gen(CPU, 5)
    live = torch.rand(512, 768, generator=g) < 0.05
    live[255, 767] = live[256, 0] = live[511, 3] = live[0, 255] = True
    assert torch.equal(R.decode_mask_pp(_encode_pp(live), 512, 768), live)
    assert torch.equal(R.decode_mask_w4(_encode_w4(live), 512, 768), live)
    # ragged: the decoder returns whole tiles, the caller slices
    dec = R.decode_mask_w4(_encode_w4(live), 300, 520)
    assert dec.shape == (512, 768) and torch.equal(dec[:300, :520], live[:300, :520])
    one = torch.zeros(256, 256, dtype=torch.bool)
    # wm 0, i 1, rl 1; wn 0, j 0, qd 1, r 2 -> thread 17, word 1, bit 1 (w4) / word 0, bit 16 + 2 (pp)
    one[17, 6] = True
    w4, pp = _encode_w4(one), _encode_pp(one)
    assert w4[17 * 8 + 1].item() == 1 << 1 and int(w4.ne(0).sum()) == 1
    assert pp[17 * 4 + 0].item() == 1 << 18 and int(pp.ne(0).sum()) == 1


# ------------------------------------------------------------------------------------------------ predicate mirrors
def test_wgrad_split_counts_documented_in_bind():
    """The comment above csrc/bind_gemm.cpp wgrad_splits, on 256 CUs: 378 tiles -> 2, 216 -> 13, 9 / 36 at 512K tokens ->
    28 / 7, 27 -> 28."""
    K = 512 * 1024
    assert R.wgrad_splits(378, 8192, 256) == 2 and R.wgrad_splits(378, K, 256) == 2
    assert R.wgrad_splits(216, K, 256) == 13
    assert R.wgrad_splits(9, K, 256) == 28 and R.wgrad_splits(36, K, 256) == 7 and R.wgrad_splits(27, K, 256) == 28
    # gemm_wgrad on top of it: at most K / 256 splits, chunks of whole 64-row k-tiles, a short last split
    assert R.wgrad_split_plan(960, 264, 256, 264, 256, 256, 0) == (3, 320)
    assert R.wgrad_split_plan(960, 264, 256, 264, 256, 256, 1) == (1, 960)
    assert R.wgrad_split_plan(320, 520, 768, 520, 768, 256, 0) == (1, 320)
    assert R.wgrad_split_plan(8192, 32128, 768, 32128, 768, 256, 0)[0] == 2
    s, kc = R.wgrad_split_plan(960, 8, 256, 8, 256, 256, 2)
    assert (s, kc) == (2, 512) and kc * (s - 1) < 960 < kc * s  # last split 448 rows: short
    assert R.wgrad_segs_plan(32, 64, 264, 256, 264, 256, 256) == (32, 64, 1)
    assert R.wgrad_segs_plan(1, 64, 264, 256, 264, 256, 256) == (1, 64, 1)
    s, kc, ch = R.wgrad_segs_plan(5, 192, 264, 256, 264, 256, 256)
    assert s == 5 * ch and kc * ch >= 192 > kc * (ch - 1)


def test_persistence_predicates():
    cus = R.mirrored_cus(256)
    assert cus == 256 and R.mirrored_cus(304) == 304 and R.mirrored_cus(100) == 96
    assert R.pp_persistent(1, 528, 128, cus) and R.pp_persistent(0, 512, 128, cus)
    assert not R.pp_persistent(1, 511, 128, cus) and not R.pp_persistent(1, 528, 64, cus)
    assert not R.pp_persistent(1, 528, 128, cus, variant=8)
    for epi in (3, 4, 6):  # the epilogues that load aux in the epilogue never run persistent
        assert not R.pp_persistent(epi, 528, 768, cus)
    for epi in (0, 1, 2, 5, 7, 8, 9):
        assert R.pp_persistent(epi, 528, 768, cus)
    assert not R.pp_persistent(1, 10, 768, cus) and not R.pp_persistent(1, 6, 64, cus)  # 512 x 1280, 768 x 512
    assert R.w4_persistent(0, 264, 128, True, cus) and not R.w4_persistent(0, 256, 128, True, cus)
    assert not R.w4_persistent(0, 264, 64, True, cus) and not R.w4_persistent(0, 264, 128, False, cus)
    assert not R.w4_persistent(12, 528, 1024, True, cus) and R.w4_persistent(11, 528, 1024, True, cus)
    assert [R.w4_sched(v) for v in (0, 1, 2, 3, 257, 769, 16, 112)] == [0, 1, 2, 3, 257, 769, 16, 112]
    assert R.w4_sched(16, bias=True) == 0 and R.w4_sched(112, kmajor=True) == 0 and R.w4_sched(513) == 1


# ------------------------------------------------------------------------------------------------------ sensitivity
PM, PN, PK = 8448, 4096, 128  # the persistent ping-pong shape on 256 CUs (528 tiles, 2-3 per workgroup)


@pytest.fixture(scope="module")
def persistent_case():
    """A correct synthetic kernel output at the persistent shape: exact operands, fp32 products (== fp64, see
    test_dyadic_operands_are_exact), bias, ReLU + dropout(0.1), one bf16 store."""
    g = R.gen(CPU, 11)
    a = R.dyadic((PM, PK), CPU, generator=g)
    w = R.dyadic((PN, PK), CPU, R.density_for(PK), generator=g)
    bias = R.dyadic(PN, CPU, generator=g)
    assert 64.0 * (PK + 1) < R.EXACT_LIMIT
    u = a.float() @ w.float().t() + bias.float()  # exact
    return {"a": a, "w": w, "bias": bias, "u": u, "plain": u.to(BF16)}


def _reject_exact(got, ref32):
    return R.exact_mismatch(got, ref32.double()) is not None


def test_sensitivity_one_ulp(persistent_case):
    ref = persistent_case["plain"]
    got = ref.clone()
    r, c = 5000, 3000
    assert ref[r, c] != 0
    got.view(torch.int16)[r, c] += 1
    assert _reject_exact(got, persistent_case["u"])
    assert old_accepts(got, ref.float())


def test_sensitivity_block_missing_one_k_tile(persistent_case):
    """A ring slot refilled one phase early: one 32 x 32 block of one tile lacks one 64-deep k-tile."""
    c = persistent_case
    got = c["plain"].clone()
    r0, c0 = 20 * 256 + 128, 9 * 256 + 64
    miss = c["a"][r0:r0 + 32, 64:128].float() @ c["w"][c0:c0 + 32, 64:128].float().t()
    assert miss.abs().max() > 0
    got[r0:r0 + 32, c0:c0 + 32] = (c["u"][r0:r0 + 32, c0:c0 + 32] - miss).to(BF16)
    bad = R.exact_mismatch(got, c["u"].double())
    assert bad is not None and "'tile': (20, 9)" in bad and "'quadrant': (1, 1)" in bad, bad
    assert old_accepts(got, c["plain"].float())


def test_sensitivity_row_duplicated(persistent_case):
    c = persistent_case
    got = c["plain"].clone()
    got[3 * 256 + 77, 512:768] = got[3 * 256 + 78, 512:768]
    assert _reject_exact(got, c["u"])
    assert old_accepts(got, c["plain"].float())


def test_sensitivity_bias_shifted_in_last_tile_column(persistent_case):
    """One wave (128 x 64 outputs) of the grid's last tile reads its bias 4 columns off.  (The same shift in the whole
    last tile column, 6 % of this output, is the one fault of this list the old share does catch.)"""
    c = persistent_case
    shifted = torch.roll(c["bias"].float()[PN - 64:], 4)
    got = c["plain"].clone()
    r0 = PM - 128
    got[r0:, PN - 64:] = (c["u"][r0:, PN - 64:] - c["bias"].float()[PN - 64:] + shifted).to(BF16)
    bad = R.exact_mismatch(got, c["u"].double())
    assert bad is not None and "'tile': (32, 15)" in bad and "'quadrant': (1, 3)" in bad, bad
    assert old_accepts(got, c["plain"].float())


def test_sensitivity_keep_bit_flipped(persistent_case):
    """ReLU + dropout(p = 0.1): one kept positive element dropped, and one bit of the stored mask flipped."""
    c = persistent_case
    p, seed = 0.1, 5
    keep = rowwise_keep_mask(seed, p, PM, PN, CPU)
    h64, live = R.relu_fwd_ref(c["u"].double(), keep, p)
    scaled = (torch.relu(c["u"]) * torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)).to(BF16)  # fp32 v * fp32 scale
    got = torch.where(keep, scaled, torch.zeros_like(scaled))
    assert torch.equal(got != 0, live) and R.ulp_bf16(got, h64) <= 1
    idx = live.flatten().nonzero()[12345].item()
    flipped = got.clone()
    flipped.view(-1)[idx] = 0
    assert not torch.equal(flipped != 0, live)  # the new check: zero pattern == relu > 0 & keep, exactly
    assert old_accepts(flipped, h64.float())
    tile = live[:256, :256]
    words = _encode_pp(tile)
    words[1000] ^= 1 << 9
    assert not torch.equal(R.decode_mask_pp(words, 256, 256), tile)  # ... and the stored words themselves


def test_sensitivity_partial_over_127_rows():
    """One wave's 64 columns of one 128-row partial miss a row."""
    g = R.gen(CPU, 13)
    M, N = 8448, 1024
    du = torch.randn(M, N, generator=g).to(BF16)
    ref, mass = R.col_partials_ref(du)
    got = ref.float().clone()
    got[40, 256:320] -= du[40 * 128 + 127, 256:320].float()
    assert R.col_err(ref.float(), ref, mass) < R.COL_BOUND
    assert R.col_err(got, ref, mass) > 50 * R.COL_BOUND
    assert old_rel(got, ref) < 1e-2  # the bound test_gemm_fused_gelu_bwd_colsum applies
