"""fp64 references, exact operands, error metrics, mask decoders and launch-predicate mirrors for the GEMM kernels
(csrc/gemm_fused.hip, csrc/gemm_w4.hip and its weight-gradient mode, csrc/colsum.hip).

Plain torch in float64, written from the operations' definitions (not from the kernels): the oracle of
tests/test_gemm_exact_gpu.py, itself validated on the CPU by tests/test_gemm_refs_cpu.py.  Not a conftest: imported by
name, like tests/rowwise_refs.py.

Exact operands.  ``dyadic`` draws k/8 with |k| <= 8.  Every product of two such values is a multiple of 1/64 and every
partial sum of products, in any order and under any split-K or MFMA blocking, is a multiple of 1/64 bounded by the L1
mass sum |a||b|: it is exact in fp32 while 64 * mass < 2^24 (``exact_headroom``).  A GEMM with fp32 accumulation on
such operands therefore has ONE rounding, the final store, which ``tensor.to(dtype)`` reproduces (round to nearest
even): the kernel output must equal the fp64 result cast to the output type bit for bit.
"""
import math

import torch

from rowwise_refs import COL_BOUND, TINY, col_err  # noqa: F401  (re-exported: one definition of the column metric)

BF16 = torch.bfloat16
EXACT_LIMIT = float(2 ** 24)

# Per-element bound of the transcendental epilogues on exact pre-activations u:
#     |got - ref| <= BF16_REL * |ref| + GELU_ABS * (1 + |u|)
# BF16_REL = 2^-8: half a bf16 ulp (8 significand bits) of the stored value, relative to |ref|.
# GELU_ABS = 2^-16: csrc/gelu.h forms Phi(u) from the Abramowitz-Stegun 7.1.26 erf (|error| <= 1.5e-7, i.e. 0.75e-7 on
# Phi) or from tanh = 1 - 2 / (exp2(.) + 1), with v_rcp_f32 and v_exp_f32 at ~1 ulp (2^-23 relative) of quantities
# <= 1, and a handful of fp32 fma roundings of values <= 1: |Phi_kernel - Phi| <= ~8 * 2^-23 ~ 2^-20.  gelu = u Phi and
# gelu' = Phi + u phi(u) (phi <= 0.4; the tanh form's polynomial factor u (1 - th^2) (1 + 0.134 u^2) sqrt(2/pi) / 2 is
# <= 1.2 as well) then carry at most (1 + |u|) * 2^-20 absolute error: 2^-16 (1 + |u|) leaves a factor 16 of room.
# There is no accumulation term: u is exact.
BF16_REL = 2.0 ** -8
GELU_ABS = 2.0 ** -16
# real-valued operands: the standard forward bound of a length-K fp32 dot product, unit roundoff 2^-23 so that a
# truncating accumulator is covered too, on top of the bf16 store
ACC_U = 2.0 ** -23


# --------------------------------------------------------------------------------------------------------- operands
def gen(device, seed):
    return torch.Generator(device=device).manual_seed(int(seed))


def dyadic(shape, device, density=1.0, generator=None):
    """bf16 tensor of k/8, k uniform in [-8, 8], each entry kept with probability ``density`` (else 0)."""
    shape = tuple(shape) if isinstance(shape, (tuple, list, torch.Size)) else (int(shape),)
    k = torch.randint(-8, 9, shape, device=device, generator=generator).to(torch.float32) / 8.0
    if density < 1.0:
        k = k * (torch.rand(shape, device=device, generator=generator) < density)
    return k.to(BF16)


# reduction lengths the GPU tests run exact operands at (tests/test_gemm_refs_cpu.py checks the precondition at each)
EXACT_KS = (64, 128, 192, 256, 320, 512, 960, 1024, 2048)


def density_for(K):
    """~32 non-zero products per output: u has std ~2.1 (0.61^2 * sqrt(32)), the curved region of GELU, both signs."""
    return min(1.0, 32.0 / K)


def exact_headroom(a, b, extra=None):
    """64 * max_mn (sum_k |a[m, k]| |b[n, k]| (+ extra[m, n])): callers assert it is < 2^24 (``EXACT_LIMIT``), the
    precondition of every bit-exact comparison.  a = [M, K], b = [N, K]."""
    mass = a.double().abs() @ b.double().abs().t()
    if extra is not None:
        mass = mass + extra.double().abs()
    return 64.0 * mass.max().item()


# ------------------------------------------------------------------------------------------------------- references
def gemm_ref(a, b, kmajor=False, bias=None, c0=None):
    """fp64 C = A . B (+ bias) (+ c0).  A = [M, K]; B = [N, K] (NT) or [K, N] (``kmajor``, NN)."""
    bd = b.double()
    u = a.double() @ (bd if kmajor else bd.t())
    if bias is not None:
        u = u + bias.double()
    if c0 is not None:
        u = u + c0.double()
    return u


def gemm_mass(a, b, kmajor=False, bias=None, c0=None):
    """L1 mass of the terms of ``gemm_ref``: |A| . |B| (+ |bias|) (+ |c0|)."""
    bd = b.double().abs()
    m = a.double().abs() @ (bd if kmajor else bd.t())
    if bias is not None:
        m = m + bias.double().abs()
    if c0 is not None:
        m = m + c0.double().abs()
    return m


def _scale(keep, p):
    """Dropout multiplier keep / (1 - p) in fp64 (1 where p == 0)."""
    if p > 0.0:
        return keep.double() / (1.0 - p)
    return 1.0


def phi_pair(u, act):
    """(act(u), act'(u)) in fp64 for act = 'gelu' (erf) or 'gelu_new' (tanh), from the definitions."""
    if act == "gelu":
        cdf = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))
        pdf = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
        return u * cdf, cdf + u * pdf
    if act == "gelu_new":
        c = math.sqrt(2.0 / math.pi)
        th = torch.tanh(c * (u + 0.044715 * u ** 3))
        return 0.5 * u * (1.0 + th), 0.5 * (1.0 + th) + 0.5 * u * (1.0 - th * th) * c * (1.0 + 3.0 * 0.044715 * u * u)
    raise ValueError(act)


def relu_fwd_ref(u, keep=None, p=0.0):
    """(h, live): h = dropout(relu(u)); live = relu(u) > 0 and kept (the ReLU derivative bit)."""
    r = torch.relu(u)
    live = r > 0
    if p > 0.0:
        live = live & keep
    return r * _scale(keep, p), live


def gelu_fwd_ref(u, act, keep=None, p=0.0):
    """(h, G): h = s act(u), G = s act'(u), s = keep / (1 - p)."""
    g, dg = phi_pair(u, act)
    s = _scale(keep, p)
    return g * s, dg * s


def geglu_fwd_ref(gate, up, keep=None, p=0.0):
    """Gated tanh-GELU trio: h = s gelu(gate) up, G1 = s gelu'(gate) up, G2 = s gelu(gate)."""
    g, dg = phi_pair(gate, "gelu_new")
    s = _scale(keep, p)
    return g * up * s, dg * up * s, g * s


def drelu_ref(dh, live, p=0.0):
    """dU = dH * live / (1 - p): ``live`` from the saved H (H != 0) or from the mask bits."""
    return dh * live.double() / (1.0 - p)


def dgelu_ref(dh, G):
    """dU = (dY Wo) * G with the stored (bf16) G."""
    return dh * G.double()


def dgeglu_ref(dh, g1, g2):
    """[dH G1 | dH G2] in the stacked [M, 2F] layout."""
    return torch.cat([dh * g1.double(), dh * g2.double()], dim=1)


def wgrad_ref(a, b, c0=None, beta=False):
    """C = A^T B (+ c0): A = [K, M], B = [K, N] token-major."""
    c = a.double().t() @ b.double()
    if beta:
        c = c + c0.double()
    return c


def col_partials_ref(x, rows=128):
    """(partials, mass): per-``rows``-row column sums of x [M, N] (M % rows == 0) in fp64 and their L1 mass."""
    xd = x.double()
    M, N = xd.shape
    v = xd.view(M // rows, rows, N)
    return v.sum(1), v.abs().sum(1)


# ---------------------------------------------------------------------------------------------------------- metrics
def locate(flat_index, ncols, tile=256, quad=(128, 64)):
    """Where an output element lives: 256 x 256 tile, wave quadrant inside it (rows x cols of ``quad``), row, column."""
    r, c = int(flat_index) // ncols, int(flat_index) % ncols
    quadrant = ((r % tile) // quad[0], (c % tile) // quad[1])
    return {"tile": (r // tile, c // tile), "quadrant": quadrant, "row": r, "col": c}


def _ordered(x):
    """bf16 bit patterns as integers ordered like the values (sign-magnitude -> two's complement)."""
    b = x.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    mag = b & 0x7FFF
    return torch.where((b & 0x8000) != 0, -mag, mag)


def ulp_bf16(got, ref):
    """max distance between ``got`` (bf16) and ``ref`` (any dtype, rounded to bf16 first) in bf16 ulps."""
    assert got.dtype == BF16 and got.shape == ref.shape
    r = ref.float().to(BF16) if ref.dtype != BF16 else ref
    return int((_ordered(got) - _ordered(r)).abs().max().item())


def exact_mismatch(got, ref64, dtype=None):
    """None if ``got`` equals ``ref64`` rounded once to ``dtype``, else a description of the first and the number of
    mismatching elements.  The fp64 -> fp32 step is exact for every value an exact-operand test produces."""
    dtype = dtype or got.dtype
    assert got.dtype == dtype, (got.dtype, dtype)
    exp = ref64.to(torch.float32).to(dtype)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    if torch.equal(got, exp):
        return None
    bad = (got != exp) | (got.isnan() != exp.isnan())
    idx = int(bad.flatten().nonzero()[0].item())
    where = locate(idx, got.shape[-1])
    return (f"{int(bad.sum().item())} of {got.numel()} elements differ; first at {where}: got "
            f"{got.flatten()[idx].item()!r} expected {exp.flatten()[idx].item()!r}")


def assert_exact(got, ref64, dtype=None, msg=""):
    bad = exact_mismatch(got, ref64, dtype)
    assert bad is None, f"{msg}: {bad}"


def elem_bound(got, ref, bound):
    """(worst ratio |got - ref| / bound over the elements, where that element lives, its error and bound).  ``bound``
    is a per-element tensor > 0; the check is ratio <= 1 for EVERY element, never a share."""
    err = (got.detach().double() - ref.double()).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = err / bound
    idx = int(ratio.flatten().argmax().item())
    return ratio.flatten()[idx].item(), locate(idx, got.shape[-1]), err.flatten()[idx].item(), \
        bound.flatten()[idx].item()


def assert_elem_bound(got, ref, bound, msg="", u=None):
    worst, where, err, lim = elem_bound(got, ref, bound)
    extra = "" if u is None else f" u={u.flatten()[where['row'] * got.shape[-1] + where['col']].item():.6g}"
    assert worst <= 1.0, f"{msg}: |err| {err:.4g} > bound {lim:.4g} (x{worst:.3g}) at {where}{extra}"
    return worst


def gelu_bound(ref, u):
    """BF16_REL |ref| + GELU_ABS (1 + |u|) per element (see the constants' derivation above).  The same bound serves
    the dropout-scaled outputs (scale <= 2 in the tests) and the gated products (times an exact |up|): both spend the
    factor 16 of room, nothing else."""
    return BF16_REL * ref.double().abs() + GELU_ABS * (1.0 + u.double().abs())


def gelu_abs_use(got, ref, u):
    """Share of the absolute term GELU_ABS (1 + |u|) the worst element uses once the bf16 store's BF16_REL |ref| is
    taken off: the observed error of the transcendental approximation against its allowance (reported, not asserted)."""
    r = ref.double()
    over = ((got.detach().double() - r).abs() - BF16_REL * r.abs()).clamp_min(0.0)
    return (over / (GELU_ABS * (1.0 + u.double().abs()))).max().item()


def real_bound(ref, mass, K):
    """BF16_REL |ref| + K 2^-23 mass per element: real-valued operands, fp32 accumulation of K terms, bf16 store."""
    return BF16_REL * ref.double().abs() + K * ACC_U * mass.double()


# ----------------------------------------------------------------------------------------------------- mask decoders
def _bits(words):
    w = words.contiguous().view(-1, 1).to(torch.int64) & 0xFFFFFFFF
    return ((w >> torch.arange(32, device=words.device)) & 1).to(torch.bool)


def decode_mask_w4(words, M, N):
    """bool [ceil(M/256) 256, ceil(N/256) 256] from csrc/gemm_w4.hip's ReLU bit mask (layout: csrc/gemm_params.h
    GemmW4Params::mask), padded to whole tiles so the caller can look at rows >= M and columns >= N too."""
    tm, tn = (M + 255) // 256, (N + 255) // 256
    assert words.numel() >= tm * tn * 2048
    b = _bits(words.flatten()[:tm * tn * 2048])
    # word index = ((tile_row tn + tile_col) 256 + 64 (2 wm + wn) + 16 qd + rl) 8 + i
    # bit = 16 r0 + 2 j + r1, r = 2 r1 + r0
    b = b.view(tm, tn, 2, 2, 4, 16, 8, 2, 8, 2)  # tm tn wm wn qd rl i r0 j r1
    b = b.permute(0, 2, 6, 5, 1, 3, 8, 4, 9, 7)  # tm wm i rl | tn wn j qd r1 r0
    return b.reshape(tm * 256, tn * 256)


def decode_mask_pp(words, M, N):
    """bool [M, N] from the ping-pong kernel's ReLU bit mask (layout: csrc/gemm_params.h GemmFusedParams::mask)."""
    assert M % 256 == 0 and N % 256 == 0 and words.numel() == M * N // 32
    tm, tn = M // 256, N // 256
    b = _bits(words)
    # word index = ((tile_row tn + tile_col) 512 + 64 (4 wm + wn) + 16 q + rl) 4 + k
    # bit = 16 i0 + 4 j + r, i = 2 k + i0
    b = b.view(tm, tn, 2, 4, 4, 16, 4, 2, 4, 4)  # tm tn wm wn q rl k i0 j r
    b = b.permute(0, 2, 6, 7, 5, 1, 3, 8, 4, 9)  # tm wm k i0 rl | tn wn j q r
    return b.reshape(M, N)


# ------------------------------------------------------------------------------------------ launch-predicate mirrors
PP_LIGHT = (0, 1, 2, 5, 7, 8, 9)  # csrc/gemm_fused.hip launch_pp: epilogues that may run persistent


def mirrored_cus(multi_processor_count):
    """The CU count the launch code uses (whole XCD-octets)."""
    return multi_processor_count // 8 * 8


def pp_persistent(epi, tiles, K, cus, variant=9):
    """csrc/gemm_fused.hip launch_pp: the ping-pong kernel runs one workgroup per CU walking >= 2 tiles."""
    return variant == 9 and epi in PP_LIGHT and cus >= 8 and tiles >= 2 * cus and K >= 128


def w4_persistent(epi, tiles, K, persist, cus):
    """csrc/gemm_w4.hip launch_rs (+ dllm_gemm_w4, which never asks for it on the GELU backward, epilogue 12, and the
    weight gradient, epilogue 10)."""
    return epi not in (10, 12) and bool(persist) and K >= 128 and cus >= 8 and tiles > cus


def wgrad_splits(tiles, K, cus):
    """csrc/bind_gemm.cpp wgrad_splits (``cus``: the device's raw multi-processor count there)."""
    smax = max(1, min(K // 256, 64))
    best, bestc = 1, 1e30
    for s in range(1, smax + 1):
        rounds = float((tiles * s + cus - 1) // cus)
        c = rounds / s + (1.7 * tiles * s / K if s > 1 else 0.0)
        if c < bestc * (1.0 - 1e-6):
            bestc, best = c, s
    return best


def wgrad_split_plan(K, M, N, lda, ldb, cus, splits_req=0):
    """(splits, kchunk) of csrc/bind_gemm.cpp gemm_wgrad for A = [K, M] (row stride lda), B = [K, N] (ldb)."""
    tiles = ((M + 255) // 256) * (N // 256)
    splits = splits_req if splits_req > 0 else wgrad_splits(tiles, K, cus)
    splits = max(1, min(splits, K // 256))
    kchunk = ((K + splits - 1) // splits + 63) // 64 * 64
    ld, wd = max(lda, ldb), max(M, N)
    while kchunk > 64 and ((kchunk - 1) * ld + wd) * 2 >= 0xFFFFFFFF:
        splits += 1
        kchunk = ((K + splits - 1) // splits + 63) // 64 * 64
    return (K + kchunk - 1) // kchunk, kchunk


def wgrad_segs_plan(nseg, rows, M, N, lda, ldb, cus):
    """(splits, kchunk, chunks per segment) of csrc/bind_gemm.cpp gemm_wgrad_segs."""
    tiles = ((M + 255) // 256) * (N // 256)
    want = wgrad_splits(tiles, rows * nseg, cus)
    chunks = max(1, min((want + nseg // 2) // nseg, rows // 64))
    kchunk = ((rows + chunks - 1) // chunks + 63) // 64 * 64
    ld, wd = max(lda, ldb), max(M, N)
    while kchunk > 64 and ((kchunk - 1) * ld + wd) * 2 >= 0xFFFFFFFF:
        kchunk -= 64
    chunks = (rows + kchunk - 1) // kchunk
    return nseg * chunks, kchunk, chunks


W4_SCHED_COMPILED = (0, 1, 2, 3, 257, 769)  # csrc/gemm_w4.hip launch: schedules every plain form is built with
W4_SCHED_ABLATIONS = (16, 32, 64, 112, 128)  # ... and the timing ablations of the plain no-bias NT forward


def w4_sched(rs, kmajor=False, bias=False, acc=False):
    """The kernel template's RS a DLLM_ROUTE w4_sched value selects for the plain epilogue (csrc/gemm_w4.hip launch)."""
    if not kmajor and not bias and not acc and rs in W4_SCHED_ABLATIONS:
        return rs
    if rs & 256:
        return 769 if rs & 512 else 257
    return rs & 3
