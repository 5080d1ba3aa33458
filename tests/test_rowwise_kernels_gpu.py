"""Kernel-level tests of the memory-bound kernels (csrc/norm.hip, act.hip, adamw.hip, ce.hip) beyond one launch wave.

Each kernel against an fp64 reference of the same operation (tests/rowwise_refs.py, validated on the CPU by
tests/test_rowwise_refs_cpu.py) at the row counts, widths and dtypes where the code takes another path: the second row
of a wave in ``norm_bwd_kernel`` (N > 2048), the second trip of the grid-stride loops, partly filled 256-column chunks,
the 4-wide AdamW kernel, the fp32 instantiations, the scalar path of ``ce_bwd_kernel``.

Metrics (rowwise_refs): per-ROW relative error for row-shaped outputs (2e-2 bf16, 1e-5 fp32), error against the
column's L1 mass for fp32 column sums (1e-5), exact equality of dropout zero sets.  One wrong row of 4099 passes a
whole-tensor rel-L2; it does not pass these.  For every fp32 bound the fp32 torch composite of the same operation is
measured against fp64 on the same inputs and must sit under a quarter of the bound (``comp`` below).  Every figure is
printed before a test asserts (run with -s to collect them).
"""
import types

import numpy as np
import pytest
import torch

import rowwise_refs as R
from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops import activations, norms, rng
from distributed_llms_example_amd.ops.optim import FusedAdamW

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF16, "fp32": F32}


class Figures:
    """Collects (name, measured, bound[, composite]) lines, prints each, asserts them all at the end of the test."""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def add(self, name, val, bound, comp=None):
        line = f"[fig] {self.tag} {name}: err {val:.3e} bound {bound:.1e}" + (f" comp {comp:.3e}" if comp is not None else "")
        print(line)
        if not val < bound or (comp is not None and not comp <= bound / 4):
            self.bad.append(line)

    def row(self, name, got, ref, dtype, comp=None):
        """Per-row error; ``comp``: the fp32 composite's tensor, required (and checked) when the bound is the fp32 one."""
        c = R.row_err(comp, ref) if (dtype == F32 and comp is not None) else None
        self.add(name, R.row_err(got, ref), R.ROW_BOUND[dtype], c)

    def col(self, name, got, ref, mass, comp, single_term=False):
        """fp32 column sum against its L1 mass.  ``single_term``: see test_norm_fwd_bwd."""
        c = R.col_err(comp, ref, mass)
        self.add(name, R.col_err(got, ref, mass), max(R.COL_BOUND, 4 * c) if single_term else R.COL_BOUND, c)

    def check(self, name, ok):
        print(f"[fig] {self.tag} {name}: {'ok' if ok else 'FAILED'}")
        if not ok:
            self.bad.append(f"{self.tag} {name}")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(*shape, gen, dtype, scale=1.0):
    return (torch.randn(*shape, device=DEV, generator=gen) * scale).to(dtype)


# ------------------------------------------------------------------------------------------------------------ norm
def _norm_inputs(N, d, kind, dtype, gen):
    x = R.nonzero_randn(N, d, device=DEV, dtype=dtype, generator=gen)
    # |resid| < 4 and |x| >= 0.01: x / (1 - p) exceeds half a bf16 ulp of resid, so s == resid only where x was dropped
    r = torch.randn(N, d, device=DEV, generator=gen).clamp(-3.9, 3.9).to(dtype)
    w = (1 + 0.1 * torch.randn(d, device=DEV, generator=gen)).to(dtype)
    b = (0.1 * torch.randn(d, device=DEV, generator=gen)).to(dtype) if kind == norms.LAYER else None
    return x, r, w, b


def _norm_bwd_composite(s, w, b, g1, g2, eps, p, keep, kind):
    """The fp32 torch composite of the backward from the stored s: autograd through norms._reference in fp32."""
    sl, wl = s.float().clone().requires_grad_(True), w.float().clone().requires_grad_(True)
    bl = b.float().clone().requires_grad_(True) if b is not None else None
    z = torch.zeros_like(sl)
    if g1 is not None:
        out, _ = norms._reference(sl, None, wl, bl, eps, 0.0, 0, kind)
        out.backward(g1.float())
    ds = (sl.grad if sl.grad is not None else z) + (g2.float() if g2 is not None else 0.0)
    dx = ds * keep.float() * (1.0 / (1.0 - p)) if p > 0.0 else ds
    zc = torch.zeros_like(wl)
    return {"dstream": ds, "dx": dx, "dw": wl.grad if wl.grad is not None else zc,
            "db": bl.grad if (bl is not None and bl.grad is not None) else zc, "dxs": dx.sum(0)}


# every width with an N > 2048 and every N with a partly filled last 256-column chunk; d <= 1024 runs two rows per wave:
# 2049 = exactly one wave with a second row, 2051 = three, 4099 = second loop trip without a second row, 6150 = with one;
# d > 1024 (one row per wave): 2051 = second trip for three waves, 4099 = third trip
NORM_SHAPES = [(1, 260), (2, 4), (5, 1020), (2049, 4), (2049, 260), (2051, 8), (2051, 516), (4099, 252), (4099, 772),
               (6150, 1020), (2051, 1028), (4099, 1500), (2051, 2044), (4099, 2048)]


def _norm_options(N, d):
    """(resid, p, grad of out, grad of s).  A 4- or 8-wide row that dropout or the norm's projection (which removes 1-2 of
    its d dimensions) can leave ~empty has no meaningful per-row error, so d <= 8 runs without dropout and, at N > 5, with
    a stream gradient."""
    if d <= 8:
        return [(True, 0.0, True, True), (True, 0.0, False, True)] + ([(False, 0.0, True, False)] if N <= 5 else [])
    return [(False, 0.0, True, False), (True, 0.0, True, True), (True, 0.0, True, False), (True, 0.1, True, True),
            (False, 0.1, True, False), (False, 0.1, False, True), (True, 0.1, False, True)]


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("kind", [norms.RMS, norms.LAYER])
@pytest.mark.parametrize("N,d", NORM_SHAPES)
def test_norm_fwd_bwd(N, d, kind, dt):
    """norms._norm forward + backward (and the same launch through C.norm_bwd for the fp32 dw / db) vs fp64: out, s, dx,
    dresid (= dstream) per row, dw / db per column, dropout zero sets exact.

    LayerNorm dw at N = 1: the column "sum" is the single term dout * (s - mean) * rstd, so the metric degenerates to the
    relative error of s - mean, which cancels wherever an element sits near the row mean.  The fp32 composite itself
    misses the quarter bound 2.5e-6 there (N = 1, d = 260, no residual, p = 0: 2.26e-5 on fp32 inputs, 8.25e-6 on bf16
    ones; the kernel: 1.85e-6 and 8.25e-6), so this case bounds the kernel by max(1e-5, 4 x the composite's error on the
    same inputs), measured and printed by the test: 9.0e-5 and 3.3e-5."""
    dtype = DT[dt]
    C = _ext.native()
    eps, seed = 1e-6, 1234 + N
    for resid, p, gout, gs in _norm_options(N, d):
        F = Figures(f"norm N={N} d={d} kind={kind} {dt} resid={int(resid)} p={p} gout={int(gout)} gs={int(gs)}")
        gen = _gen(N * 7919 + d)
        x, r, w, b = _norm_inputs(N, d, kind, dtype, gen)
        if not resid:
            r = None
        # gradients without zeros (a normal draw of millions of elements does hit 0.0): a zero in dx is a dropped element
        g1 = R.nonzero_randn(N, d, device=DEV, dtype=dtype, generator=gen) if gout else None
        g2 = R.nonzero_randn(N, d, device=DEV, dtype=dtype, generator=gen) if gs else None
        keep = rng.keep_mask(seed, p, (N, d), DEV) if p > 0 else None
        stored = resid or p > 0
        leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (x, r, w, b)]
        out, s = norms._norm(leaves[0], leaves[1], leaves[2], leaves[3], eps, p, seed, kind)
        ref_out, ref_s = R.norm_fwd_ref(x, r, w, b, eps, p, keep, kind)
        comp_out, comp_s = norms._reference(x, r, w, b, eps, p, seed, kind) if dtype == F32 else (None, None)
        F.row("out", out, ref_out, dtype, comp_out)
        if stored:
            F.row("s", s, ref_s, dtype, comp_s)
        if p > 0:
            F.check("fwd zero set == ~keep", torch.equal((s == r) if resid else (s == 0), ~keep))
        loss = (out.float() * g1.float()).sum() if gout else 0.0
        if gs:
            loss = loss + (s.float() * g2.float()).sum()
        loss.backward()
        s_used = s.detach() if stored else x
        ref = R.norm_bwd_ref(s_used, w, g1, g2, eps, p, keep, kind)
        comp = _norm_bwd_composite(s_used, w, b, g1, g2, eps, p, keep, kind)
        F.row("dx", leaves[0].grad, ref["dx"], dtype, comp["dx"])
        if resid:
            F.row("dresid", leaves[1].grad, ref["dstream"], dtype, comp["dstream"])
        if p > 0:
            z = leaves[0].grad == 0
            F.check(f"bwd zero set == ~keep (kept but zero: {int((z & keep).sum())}, dropped but non-zero: "
                    f"{int((~z & ~keep).sum())})", torch.equal(z, ~keep))
        # the same backward through the binding: dw / db before the cast to the parameter dtype
        o2, s2, mean, rstd = C.norm_fwd(x, r, w, b, eps, p, seed, kind, True)
        F.check("direct fwd bit-equal", torch.equal(o2, out) and (not stored or torch.equal(s2, s)))
        dx2, dst2, dw, db, _ = C.norm_bwd(g1, g2, s_used, w, b, mean, rstd, p, seed, kind, resid and p > 0)
        F.check("direct dx bit-equal", torch.equal(dx2, leaves[0].grad))
        if resid and p > 0:
            F.check("direct dstream bit-equal", torch.equal(dst2, leaves[1].grad))
        single = kind == norms.LAYER and N == 1
        F.col("dw", dw, ref["dw"], ref["dw_mass"], comp["dw"], single)
        if b is not None:
            F.col("db", db, ref["db"], ref["db_mass"], comp["db"])
        if gout and dtype == F32:
            F.col("dw(autograd)", leaves[2].grad, ref["dw"], ref["dw_mass"], comp["dw"], single)
            if b is not None:
                F.col("db(autograd)", leaves[3].grad, ref["db"], ref["db_mass"], comp["db"])
        elif gout:  # rounded to the bf16 parameter dtype on return: the bf16 store's bound
            F.add("dw(autograd, bf16)", R.acc_err(leaves[2].grad, ref["dw"]), R.BF16_ACC_BOUND)
            if b is not None:
                F.add("db(autograd, bf16)", R.acc_err(leaves[3].grad, ref["db"]), R.BF16_ACC_BOUND)
        else:
            F.check("no out gradient: dw is zero", leaves[2].grad is None or not leaves[2].grad.any())
        F.done()


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("kind", [norms.RMS, norms.LAYER])
@pytest.mark.parametrize("d", [772, 1028])
def test_norm_bwd_modes(d, kind, dt):
    """C.norm_bwd called directly at N = 4099: partials_only, dw_acc / db_acc (parameter dtype and fp32, accumulating),
    want_colsum, want_stream; every mode returns the plain call's dx bit for bit."""
    dtype, N = DT[dt], 4099
    C = _ext.native()
    eps, seed = 1e-6, 4321
    for p in (0.0, 0.1):
        F = Figures(f"norm_bwd modes N={N} d={d} kind={kind} {dt} p={p}")
        gen = _gen(d + kind)
        x, r, w, b = _norm_inputs(N, d, kind, dtype, gen)
        g1, g2 = (R.nonzero_randn(N, d, device=DEV, dtype=dtype, generator=gen) for _ in range(2))
        keep = rng.keep_mask(seed, p, (N, d), DEV) if p > 0 else None
        _, s, mean, rstd = C.norm_fwd(x, r, w, b, eps, p, seed, kind, True)
        ref = R.norm_bwd_ref(s, w, g1, g2, eps, p, keep, kind)
        comp = _norm_bwd_composite(s, w, b, g1, g2, eps, p, keep, kind)
        args = (g1, g2, s, w, b, mean, rstd, p, seed, kind)
        dx0, _, dw0, db0, _ = C.norm_bwd(*args, False)
        F.row("dx", dx0, ref["dx"], dtype, comp["dx"])
        F.col("dw", dw0, ref["dw"], ref["dw_mass"], comp["dw"])
        # want_stream: dstream is the pre-dropout gradient, dx its dropped version
        dx1, dst, _, _, _ = C.norm_bwd(*args, True)
        F.check("want_stream dx bit-equal", torch.equal(dx1, dx0))
        F.row("dstream", dst, ref["dstream"], dtype, comp["dstream"])
        if p > 0:
            F.check("dx zero set == ~keep", torch.equal(dx1 == 0, ~keep))
            F.check("dstream has no zeros", bool((dst != 0).all()))
        # partials_only: the [G, d] per-workgroup partials, no reduction
        G = min((N + 3) // 4, 512)
        dx2, _, dwp, dbp, _ = C.norm_bwd(*args, False, partials_only=True)
        F.check("partials_only dx bit-equal", torch.equal(dx2, dx0))
        F.check("partials shape [G, d]", tuple(dwp.shape) == (G, d) and (b is None or tuple(dbp.shape) == (G, d)))
        F.col("dw_part.sum", dwp.double().sum(0), ref["dw"], ref["dw_mass"], comp["dw"])
        if b is not None:
            F.col("db_part.sum", dbp.double().sum(0), ref["db"], ref["db_mass"], comp["db"])
        # dw_acc / db_acc: accumulate onto existing contents, parameter dtype and fp32
        for adt in (dtype, F32):
            wb, bb = _randn(d, gen=gen, dtype=adt), (_randn(d, gen=gen, dtype=adt) if b is not None else None)
            wa, ba = wb.clone(), (bb.clone() if bb is not None else None)
            dx3, _, dw3, db3, _ = C.norm_bwd(*args, False, dw_acc=wa, db_acc=ba)
            F.check(f"dw_acc[{adt}] dx bit-equal, no dw returned", torch.equal(dx3, dx0) and dw3 is None and db3 is None)
            if adt == F32:  # base + sum: the base is one more term of the column
                F.col("dw_acc[fp32]", wa, wb.double() + ref["dw"], ref["dw_mass"] + wb.double().abs(),
                      wb.double() + comp["dw"].double())
                if b is not None:
                    F.col("db_acc[fp32]", ba, bb.double() + ref["db"], ref["db_mass"] + bb.double().abs(),
                          bb.double() + comp["db"].double())
            else:
                F.add("dw_acc[bf16]", R.acc_err(wa, wb.double() + ref["dw"]), R.BF16_ACC_BOUND)
                if b is not None:
                    F.add("db_acc[bf16]", R.acc_err(ba, bb.double() + ref["db"]), R.BF16_ACC_BOUND)
        # want_colsum: column sums of dx as per-workgroup partials
        dx4, _, _, _, dxs = C.norm_bwd(*args, False, want_colsum=True)
        F.check("want_colsum dx bit-equal", torch.equal(dx4, dx0))
        F.check("dxs_part shape [G, d]", tuple(dxs.shape) == (G, d))
        F.col("dxs_part.sum", dxs.double().sum(0), ref["dxs"], ref["dxs_mass"], comp["dxs"])
        if p > 0:
            F.check("want_colsum dx zero at dropped", bool((dx4[~keep] == 0).all()))
        F.done()


# ----------------------------------------------------------------------------------------------------- activations
ALL_ACTS = [(a, g) for a in ("relu", "gelu", "gelu_new", "silu") for g in (False, True)]
ACT_CASES = [(a, g, 3, F_) for a, g in ALL_ACTS for F_ in (4, 12, 388)] + \
            [("relu", False, 4100, 2052), ("gelu_new", True, 4100, 2052)]  # 8,413,200 outputs: past the 8192-block cap


def _act_check(F, x, dy, act, gated, p, seed, dtype, keep_seed=None):
    """act_dropout forward + backward on (x, dy) vs fp64 and, for fp32, the fp32 composite; exact zero sets: an output is
    zero iff it was dropped or the activation itself is zero there (relu of a negative input)."""
    N, F_ = dy.shape
    keep_seed = seed if keep_seed is None else keep_seed
    keep = activations.ffn_keep_mask(act, gated, keep_seed, p, (N, F_), DEV) if p > 0 else None
    xl = x.clone().requires_grad_(True)
    y = activations.act_dropout(xl, act, p, seed, gated=gated)
    y.backward(dy)
    ry, rdx, ry0, rdx0 = R.act_ref(x, act, gated, p, keep, dy)
    cy = cdx = None
    if dtype == F32:
        xc = x.clone().requires_grad_(True)
        cy = activations._reference(xc, act, gated, p, keep_seed)
        cy.backward(dy)
        cy, cdx = cy.detach(), xc.grad
    F.row("y", y, ry, dtype, cy)
    F.row("dx", xl.grad, rdx, dtype, cdx)
    if p > 0:
        F.check("fwd zero set", torch.equal(y == 0, ~keep | (ry0 == 0)))
        keep_in = torch.cat([keep, keep], -1) if gated else keep
        F.check("bwd zero set", torch.equal(xl.grad == 0, ~keep_in | (rdx0 == 0)))
    return y.detach()


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("act,gated,N,F_", ACT_CASES)
def test_act_fwd_bwd(act, gated, N, F_, p, dt):
    dtype = DT[dt]
    F = Figures(f"act {act} gated={int(gated)} N={N} F={F_} p={p} {dt}")
    gen = _gen(N + F_)
    # 0.01 <= |x| <= 4: no input zeros, and gelu / silu of it neither underflow nor round 1 + erf(x / sqrt 2) to 0
    x = R.nonzero_randn(N, 2 * F_ if gated else F_, device=DEV, dtype=dtype, generator=gen)
    dy = R.nonzero_randn(N, F_, device=DEV, dtype=dtype, generator=gen)
    _act_check(F, x, dy, act, gated, p, 77, dtype)
    F.done()


# --------------------------------------------------------------------------------------------------------- dropout
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("numel", [4, 8388612])  # 8192 blocks x 256 threads x 4 = 8,388,608: the last 4 are a 2nd trip
def test_dropout_standalone_exact(numel, dt):
    """Standalone dropout forward and backward: zero set == ~keep_mask element for element, kept elements scaled by
    1 / (1 - p) within one rounding of the dtype (2^-8 bf16, 2^-24 fp32) on top of the <= 4 fp32 roundings of the scale
    itself (p to fp32, 1 - p, the reciprocal, the product)."""
    dtype, p, seed = DT[dt], 0.1, 99
    F = Figures(f"dropout numel={numel} {dt}")
    gen = _gen(numel)
    x = R.nonzero_randn(numel, device=DEV, dtype=dtype, generator=gen).requires_grad_(True)
    dy = R.nonzero_randn(numel, device=DEV, dtype=dtype, generator=gen)
    y = activations.dropout(x, p, seed)
    y.backward(dy)
    keep = rng.keep_mask(seed, p, (numel,), DEV)
    bound = (2.0 ** -8 if dtype == BF16 else 2.0 ** -24) + 4 * 2.0 ** -24
    for name, got, src in (("y", y, x), ("dx", x.grad, dy)):
        F.check(f"{name} zero set == ~keep", torch.equal(got == 0, ~keep))
        want = src.detach().double() / (1.0 - p)
        err = ((got.detach().double() - want).abs() / want.abs())[keep].max().item() if keep.any() else 0.0
        F.add(f"{name} scale (elementwise rel)", err, bound)
    F.done()


# ----------------------------------------------------------------------------------------------------------- AdamW
ADAMW_COMBOS = [("bf16", "fp32", True), ("bf16", "fp32", False), ("bf16", "bf16", True), ("bf16", "bf16", False),
                ("fp32", "fp32", True), ("fp32", "fp32", False)]
ADAMW_CASES = [(pd, gd, ms, n) for pd, gd, ms in ADAMW_COMBOS for n in (2052, 2048)] + \
              [("bf16", "fp32", True, 4194308),   # 4-wide kernel, 4096 x 256 x 4 = 4,194,304: second trip
               ("bf16", "fp32", True, 2097160)]   # 8-wide kernel, 1024 x 256 x 8 = 2,097,152: second trip


def _mirror_hyper(lr, bc1, bc2):
    """[lr, lr / bc1, 1 / sqrt(bc2)] exactly as the host path computes them in fp32 (IEEE division and square root)."""
    lr, bc1, bc2 = np.float32(lr), np.float32(bc1), np.float32(bc2)
    return torch.tensor(np.array([lr, lr / bc1, np.float32(1) / np.sqrt(bc2)], dtype=np.float32), device=DEV)


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("pd,gd,use_master,n", ADAMW_CASES)
def test_adamw_step_direct(pd, gd, use_master, n, mask):
    """C.adamw_step, three consecutive steps, against the fp64 AdamW recurrence (scalars as the kernel receives them, in
    fp32): n = 2052 runs the 4-wide kernel, n = 2048 the 8-wide one.  Element bound 1e-5 of |ref| + rms(ref): every
    output is <= 8 fp32 operations on values within ~5 rms, ~8 x 6e-8 x 5 = 2.4e-6 at worst; a wrong element is O(1)."""
    C = _ext.native()
    F = Figures(f"adamw param={pd} grad={gd} master={int(use_master)} n={n} mask={int(mask)}")
    pdt, gdt = DT[pd], DT[gd]
    lr, b1, b2, eps, wd, coef = 1e-2, 0.9, 0.999, 1e-8, 0.5, 0.37
    gen = _gen(n)
    w0 = torch.randn(n, device=DEV, generator=gen)
    param = w0.to(pdt)
    master = param.float().clone() if use_master else None
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    wd_mask = (torch.rand(n, device=DEV, generator=gen) < 0.5).to(torch.uint8) if mask else None
    coef_t = torch.full((), coef, device=DEV)
    rw, rm, rv = param.double(), m.double(), v.double()
    hyper_self = types.SimpleNamespace(betas=(b1, b2))
    for step in (1, 2, 3):
        g = _randn(n, gen=gen, dtype=gdt, scale=1e-2)
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        # the same step through the hyper tensor with deliberately wrong host lr / bc1 / bc2: bit-identical
        cl = [t.clone() if t is not None else None for t in (param, master, m, v)]
        C.adamw_step(cl[0], cl[1], g, cl[2], cl[3], wd_mask, coef_t, 123.0, b1, b2, eps, wd, 0.5, 0.25,
                     _mirror_hyper(lr, bc1, bc2))
        # and through FusedAdamW.device_hyper itself: its 1 - beta^t is computed in fp32 on the device (~2^-23 / bc2
        # relative, 3e-6 measured at step 3), so the moments are bit-identical and the weights within the fp64 bound
        dh = FusedAdamW.device_hyper(hyper_self, torch.full((), float(step), device=DEV), lr)
        cd = [t.clone() if t is not None else None for t in (param, master, m, v)]
        C.adamw_step(cd[0], cd[1], g, cd[2], cd[3], wd_mask, coef_t, 123.0, b1, b2, eps, wd, 0.5, 0.25, dh)
        if not use_master and pdt == BF16:
            rw = param.double()  # bf16 weights without a master: each step starts from the stored (rounded) weights
        C.adamw_step(param, master, g, m, v, wd_mask, coef_t, lr, b1, b2, eps, wd, bc1, bc2)
        same = [torch.equal(a, c) for a, c in zip((param, master, m, v), cl) if a is not None]
        F.check(f"step {step} hyper tensor == host scalars bit for bit (param, master?, m, v: {same})", all(same))
        prev = (rw, rm, rv)
        rw, rm, rv = R.adamw_ref(rw, g, rm, rv, wd_mask, coef, lr, b1, b2, eps, wd, step)
        wgot = master if use_master else param
        slack = 0.0 if (use_master or pdt == F32) else 2.0 ** -8  # bf16 weights, no master: one bf16 rounding on top
        if slack == 0.0:
            F.add(f"step {step} w rel-L2", R.rel_l2(wgot, rw), 1e-6)
        F.add(f"step {step} w elem", R.elem_err(wgot, rw, slack), 1e-5)
        F.add(f"step {step} w elem (device_hyper)", R.elem_err(cd[1] if use_master else cd[0], rw, slack), 1e-5)
        F.check(f"step {step} device_hyper: m, v bit-equal", torch.equal(cd[2], m) and torch.equal(cd[3], v))
        mh = _mirror_hyper(lr, bc1, bc2).double()
        F.add(f"step {step} device_hyper vs host values (rel)", ((dh.double() - mh).abs() / mh).max().item(),
              2.0 ** -23 / bc2 + 2.0 ** -22)
        for name, got, want in (("m", m, rm), ("v", v, rv)):
            F.add(f"step {step} {name} rel-L2", R.rel_l2(got, want), 1e-6)
            F.add(f"step {step} {name} elem", R.elem_err(got, want), 1e-5)
        if use_master and pdt == BF16:
            F.check(f"step {step} param == master.to(bf16)", torch.equal(param, master.to(BF16)))
        if mask:  # wd = 0.5: decay moves an element by lr wd = 5e-3 of itself, 2.5e-3 on this metric at |w| = rms, so a
            # mask byte applied to the wrong element of a group is ~250x the bound (20x even under the bf16 slack)
            off = wd_mask == 0
            w_nd, _, _ = R.adamw_ref(*prev[:1], g, *prev[1:], None, coef, lr, b1, b2, eps, 0.0, step)
            w_all, _, _ = R.adamw_ref(*prev[:1], g, *prev[1:], None, coef, lr, b1, b2, eps, wd, step)
            F.add(f"step {step} masked-out elements: no decay", R.elem_err(wgot[off], w_nd[off], slack), 1e-5)
            F.add(f"step {step} masked-in elements: decayed", R.elem_err(wgot[~off], w_all[~off], slack), 1e-5)
    F.done()


def test_adamw_step_rejects_misaligned_and_strided():
    """The kernels read master / moments as 16-B vectors and the decay mask as 8-B words of one flat array: the binding
    must refuse what they cannot address."""
    C = _ext.native()
    n = 2048
    big = torch.zeros(n + 8, device=DEV)
    param, grad, m, v = (torch.zeros(n, device=DEV) for _ in range(4))
    coef = torch.ones((), device=DEV)
    hp = (coef, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0.1, 0.001)
    mask_buf = torch.ones(n + 8, device=DEV, dtype=torch.uint8)
    C.adamw_step(param, big[:n], grad, m, v, mask_buf[:n], *hp)  # aligned views pass
    with pytest.raises(RuntimeError, match="aligned"):
        C.adamw_step(param, big[1:n + 1], grad, m, v, None, *hp)
    with pytest.raises(RuntimeError, match="aligned"):
        C.adamw_step(param, None, grad, m, v, mask_buf[1:n + 1], *hp)
    with pytest.raises(RuntimeError, match="contiguous"):
        C.adamw_step(param, None, grad, torch.zeros(2 * n, device=DEV)[::2], v, None, *hp)
    with pytest.raises(RuntimeError, match="contiguous"):
        C.adamw_step(param, torch.zeros(2 * n, device=DEV)[::2], grad, m, v, None, *hp)
    with pytest.raises(RuntimeError, match="contiguous"):
        C.adamw_step(param, None, grad, m, v, torch.ones(2 * n, device=DEV, dtype=torch.uint8)[::2], *hp)
    torch.cuda.synchronize()


def test_backward_bindings_reject_what_the_kernels_cannot_address():
    """norm_bwd / act_bwd / ce_bwd walk their operands as dense rows: a strided view, a weight of another width or dtype,
    or row statistics that are not fp32 [N] must raise instead of reading past the data."""
    C = _ext.native()
    N, d = 8, 260
    s = torch.randn(N, d, device=DEV)
    w, rstd, mean = torch.ones(d, device=DEV), torch.ones(N, device=DEV), torch.zeros(N, device=DEV)
    C.norm_bwd(s, None, s, w, None, mean, rstd, 0.0, 0, 1, False)  # well-formed: passes
    for bad_w in (torch.ones(d + 4, device=DEV), torch.ones(2 * d, device=DEV)[::2], w.to(BF16)):
        with pytest.raises(RuntimeError, match="weight"):
            C.norm_bwd(s, None, s, bad_w, None, None, rstd, 0.0, 0, 0, False)
    with pytest.raises(RuntimeError, match="rstd"):
        C.norm_bwd(s, None, s, w, None, None, rstd.double(), 0.0, 0, 0, False)
    with pytest.raises(RuntimeError, match="mean"):
        C.norm_bwd(s, None, s, w, None, mean[:N - 1], rstd, 0.0, 0, 1, False)
    x = torch.randn(N, 2 * d, device=DEV)
    with pytest.raises(RuntimeError, match="contiguous"):
        C.act_bwd(torch.randn(N, d, device=DEV), x[:, ::2], 0, False, 0.0, 0)
    V = 1001
    logits = torch.randn(N, 2 * V, device=DEV)
    labels = torch.zeros(N, dtype=torch.long, device=DEV)
    lse, scale = torch.zeros(N, device=DEV), torch.ones(1, device=DEV)
    with pytest.raises(RuntimeError, match="contiguous"):
        C.ce_bwd(scale, logits[:, :V], labels, lse, None, 0.0, -100, False)
    with pytest.raises(RuntimeError, match="labels"):
        C.ce_bwd(scale, logits[:, :V].contiguous(), labels[:N - 1], lse, None, 0.0, -100, False)
    with pytest.raises(RuntimeError, match="lse"):
        C.ce_bwd(scale, logits[:, :V].contiguous(), labels, lse.double(), None, 0.0, -100, False)
    with pytest.raises(RuntimeError, match="bias"):
        C.ce_bwd(scale, logits[:, :V].contiguous(), labels, lse, torch.zeros(V - 1, device=DEV), 0.0, -100, False)
    torch.cuda.synchronize()


def _rejects_cpu_operands(call, args, slots):
    """The well-formed call passes; with any one of `slots` replaced by its CPU copy it raises.  Zero-row inputs: the
    bindings check everything and return before launching, so a missing check shows as "did not raise" and never as a
    kernel reading a host pointer."""
    call(*args)
    for i in slots:
        bad = list(args)
        bad[i] = args[i].cpu()
        with pytest.raises(RuntimeError):
            call(*bad)
            pytest.fail(f"{call.__name__} accepted a CPU tensor as argument {i}")


def test_rowwise_bindings_reject_cpu_operands():
    """norm_fwd (w, resid, b), norm_bwd (dout, dw_acc) and act_bwd (dy) hand these pointers to their kernels: a tensor
    that is not on the GPU must raise."""
    C = _ext.native()
    d = 8
    x = torch.zeros(0, d, device=DEV)
    w, b, stat = torch.ones(d, device=DEV), torch.zeros(d, device=DEV), torch.zeros(0, device=DEV)
    _rejects_cpu_operands(C.norm_fwd, (x, x.clone(), w, b, 1e-6, 0.0, 0, 1, True), slots=(1, 2, 3))
    _rejects_cpu_operands(C.norm_bwd, (x.clone(), None, x, w, b, stat, stat.clone(), 0.0, 0, 1, False,
                                       torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)), slots=(0, 11))
    _rejects_cpu_operands(C.act_bwd, (x.clone(), x, 0, False, 0.0, 0), slots=(0,))
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------- sq_norm
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("n", [4, 1048580, 3000004])  # 1024 x 256 x 4 = 1,048,576: the next 4 start the second trip
def test_sq_norm(n, dt):
    dtype = DT[dt]
    C = _ext.native()
    F = Figures(f"sq_norm n={n} {dt}")
    g = _randn(n, gen=_gen(n), dtype=dtype)
    a, b = C.sq_norm(g), C.sq_norm(g)
    ref = g.double().pow(2).sum().item()
    F.add("sum of squares rel", abs(a.item() - ref) / ref, 1e-5)
    F.check("two calls return the same bits", torch.equal(a, b))
    F.done()
    buf = torch.zeros(n + 8, device=DEV, dtype=dtype)
    off = 4 if dtype == BF16 else 1  # 8 B / 4 B into the allocation: still numel % 4 == 0, not 16-B aligned
    with pytest.raises(RuntimeError, match="aligned"):
        C.sq_norm(buf[off:off + n])


# ---------------------------------------------------------------------------------------------------------- ce_bwd
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("V", [1001, 50265])
def test_ce_bwd_phase_mismatch_scalar_path(V, dt):
    """Logits as a contiguous [N, V] view one element into a larger buffer: with a freshly allocated output every row's
    input and output differ in 16-B phase (the scalar fallback of ce_bwd_kernel); in place they share it and the vector
    path runs with a non-empty scalar head.  Bounds of test_cross_entropy (loss 2e-3, gradient 2e-2), the gradient per
    row."""
    dtype, N, smooth = DT[dt], 5, 0.1
    C = _ext.native()
    F = Figures(f"ce_bwd V={V} {dt}")
    gen = _gen(V)
    buf = (3 * torch.randn(N * V + 8, device=DEV, generator=gen)).to(dtype)
    logits = buf[1:1 + N * V].view(N, V)
    assert logits.is_contiguous() and logits.data_ptr() % 16 == logits.element_size()
    labels = torch.randint(0, V, (N,), device=DEV, generator=gen)
    labels[2] = -100
    bias = 0.5 * torch.randn(V, device=DEV, generator=gen)
    lref = logits.double().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(lref + bias.double(), labels, ignore_index=-100, label_smoothing=smooth)
    ref.backward()
    loss_rows, lse = C.ce_fwd(logits, labels, bias, smooth, -100)
    count = (labels != -100).sum().float()
    loss = (loss_rows.sum() / count).item()
    F.add("loss", abs(loss - ref.item()), 2e-3 * max(1.0, abs(ref.item())))
    scale = (1.0 / count).reshape(1)
    out = C.ce_bwd(scale, logits, labels, lse, bias, smooth, -100, False)
    assert (out.data_ptr() ^ logits.data_ptr()) & 15  # the phases differ: the scalar path ran
    rows = labels != -100
    F.add("dlogits (scalar path) per row", R.row_err(out[rows], lref.grad[rows]), 2e-2)
    F.check("ignored row: zero gradient", not out[~rows].any())
    work = buf.clone()
    lv = work[1:1 + N * V].view(N, V)
    res = C.ce_bwd(scale, lv, labels, lse, bias, smooth, -100, True)
    F.check("in place: same storage", res.data_ptr() == lv.data_ptr())
    F.add("dlogits (in place, vector path with a head) per row", R.row_err(lv[rows], lref.grad[rows]), 2e-2)
    F.check("in place: ignored row zero, neighbours of the view untouched",
            not lv[~rows].any() and torch.equal(work[:1], buf[:1]) and torch.equal(work[1 + N * V:], buf[1 + N * V:]))
    F.done()


# ---------------------------------------------------------------------------------------------------- step counter
def test_seed_step_norm_act_dropout():
    """With the device step counter set, the norm, activation and standalone-dropout kernels (each translation unit has
    its own pointer) draw the masks of seed mix_host(seed, step): exactly the reference masks at steps 0 and 1, which
    differ from each other."""
    C = _ext.native()
    F = Figures("seed_step")
    seed, p, N, d = 77, 0.1, 33, 264
    gen = _gen(1)
    x = R.nonzero_randn(N, d, device=DEV, dtype=BF16, generator=gen)
    w = torch.ones(d, device=DEV, dtype=BF16)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    zeros = {"norm": [], "act": [], "dropout": []}
    # a step counter an earlier test's engine left enabled (process-wide: kernels' pointer + the registry the reference
    # masks read) is set aside for this test and put back afterwards
    prev = rng._active_step[0]
    rng._active_step[0] = None
    try:
        C.set_seed_step(step)
        for st in (0, 1):
            step.fill_(st)
            es = rng.mix_host(seed, st)
            keep = rng.keep_mask(es, p, (N, d), DEV)
            xl = x.clone().requires_grad_(True)
            _, s = norms._norm(xl, None, w, None, 1e-6, p, seed, norms.RMS)
            s.backward(torch.ones_like(s))
            F.check(f"norm step {st}: fwd and bwd zero sets", torch.equal(s == 0, ~keep) and torch.equal(xl.grad == 0, ~keep))
            zeros["norm"].append(s == 0)
            xl = x.clone().requires_grad_(True)
            y = activations.dropout(xl, p, seed)
            y.backward(torch.ones_like(y))
            F.check(f"dropout step {st}: fwd and bwd zero sets", torch.equal(y == 0, ~keep) and torch.equal(xl.grad == 0, ~keep))
            zeros["dropout"].append(y == 0)
            dy = R.nonzero_randn(N, d // 2, device=DEV, dtype=BF16, generator=gen)  # x = [a | g], 132 columns each
            y = _act_check(F, x, dy, "gelu_new", True, p, seed, BF16, keep_seed=es)
            zeros["act"].append(y == 0)
        torch.cuda.synchronize()
    finally:
        rng._active_step[0] = prev
        C.set_seed_step(prev.t if (prev is not None and prev.enabled and prev.t.is_cuda) else None)
    for k, (z0, z1) in zeros.items():
        F.check(f"{k}: masks of steps 0 and 1 differ", not torch.equal(z0, z1))
    F.done()
