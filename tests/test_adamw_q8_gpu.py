"""csrc/adamw_q8.hip (``adamw_q8_step``) against fp64, three consecutive steps, every element checked.  Each step's
reference is ``adamw_ref`` from the kernel's OWN stored state of the step before, dequantised in fp64 (step 1: zeros,
exact, so also the fp32 ``adamw_step``'s reference).  Bounds: parameter / master and side-store moments as
test_adamw_step_direct (element 1e-5, rel-L2 1e-6); absmax within 2^-21 of the exact block maximum; codes, with e the
exact new moment and d the dequantised stored one, |d - e| <= min_i |T[i] absmax - e| + 2^-20 max(|e|, |d|) — every
rounding on the path (state product, <= 3 in the recurrence, division, dequantising product) is relative to |e| or |d|,
under 8 ulp of 2^-24; the bound allows 16.  Sizes: one block, a partial wave, one grid-stride pass + 320.  Gradients
span four decades per block; block 1 is all zero, block 0's extreme element is negative.  The ``device`` cases pass the
``device_hyper`` layout with the values the host path forms in fp32 (and wrong host scalars), so the same reference
holds: a second moment quantised to zero beside a first moment that is not gives single updates of > 100 lr (inherent
to the method), and ``device_hyper``'s own fp32 1 - beta^t (~3e-5 at step 2, bounded in test_adamw_step_direct) times
such an update is not this kernel's error (1.2e-5 measured on one element of 2M); the train test runs ``device_hyper``
itself through a captured step."""
import numpy as np
import pytest
import torch

import rowwise_refs as R
from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops import q8

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, B1, B2, EPS, WD, COEF = 1e-3, 0.9, 0.999, 1e-8, 0.5, 0.37


def _big():
    wg, cap = _ext.native().adamw_q8_geometry()
    return wg * cap + 320


def _deq64(codes, absmax, signed):
    t = torch.from_numpy(q8.SIGNED if signed else q8.UNSIGNED).to(DEV).double()
    return t[codes.long()] * absmax.double()[:, None]


def _nearest_gap(e, absmax, signed):
    """min_i |T[i] absmax - e| per element in fp64: the nearest entry is one of the two that bracket e / absmax."""
    t = torch.from_numpy(q8.SIGNED if signed else q8.UNSIGNED).to(DEV).double()
    s = absmax.double()[:, None]
    x = torch.where(s > 0, e / s.clamp_min(1e-300), torch.zeros_like(e))
    i = torch.searchsorted(t, x.contiguous()).clamp(1, 255)
    return torch.minimum((t[i - 1] * s - e).abs(), (t[i] * s - e).abs())


@pytest.mark.parametrize("with_slots", [False, True])
@pytest.mark.parametrize("n", [64, 320, "pass+320"])
@pytest.mark.parametrize("hyper", ["host", "device"])
@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("pd", ["bf16", "fp32"])
def test_adamw_q8_step_direct(pd, mask, hyper, n, with_slots):
    C = _ext.native()
    n = _big() if n == "pass+320" else n
    nb = n // 64
    tag = f"adamw_q8 param={pd} mask={int(mask)} hyper={hyper} n={n} slots={int(with_slots)}"
    bad = []

    def fig(name, val, bound):
        print(f"[fig] {tag} {name}: err {val:.3e} bound {bound:.1e}")
        if not val <= bound:
            bad.append(f"{name}: {val:.3e} > {bound:.1e}")

    gen = torch.Generator(device=DEV).manual_seed(n + 7)
    param = torch.randn(n, device=DEV, generator=gen).to(torch.bfloat16 if pd == "bf16" else torch.float32)
    master = param.float().clone() if pd == "bf16" else None
    zs, zu = (q8.quantize(torch.zeros(64), s)[0].to(DEV) for s in (True, False))
    cm, cv = zs.repeat(nb, 1), zu.repeat(nb, 1)
    am, av = torch.zeros(nb, device=DEV), torch.zeros(nb, device=DEV)
    slots = torch.full((nb,), -1, dtype=torch.int32, device=DEV)
    ns = 0
    if with_slots:  # blocks in the middle of the buffer, their places in the side store in reverse order
        b0, ns = nb // 2, max(1, nb // 4)
        slots[b0:b0 + ns] = torch.arange(ns - 1, -1, -1, dtype=torch.int32, device=DEV)
    sm, sv = (torch.zeros(max(ns, 1) * 64, device=DEV) for _ in range(2))
    fp32 = slots >= 0
    idx = slots[fp32].long()
    wd_mask = (torch.rand(n, device=DEV, generator=gen) < 0.5).to(torch.uint8) if mask else None
    coef_t = torch.full((), COEF, device=DEV)
    tab = q8.tables(DEV)
    cm0, am0 = cm.clone(), am.clone()
    for step in (1, 2, 3):
        g = torch.randn(n, device=DEV, generator=gen) * 10.0 ** torch.randint(-4, 0, (n,), device=DEV, generator=gen)
        g = g.view(nb, 64)
        if nb > 1:
            g[1] = 0.0
        g[0, 5] = -50.0
        g = g.view(-1)
        # the state the kernel is about to read, in fp64
        w_prev = (master if master is not None else param).double()
        m_prev, v_prev = _deq64(cm, am, True), _deq64(cv, av, False)
        m_prev[fp32], v_prev[fp32] = sm.view(-1, 64)[idx].double(), sv.view(-1, 64)[idx].double()
        bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
        if hyper == "host":
            sc, hp = (LR, B1, B2, EPS, WD, bc1, bc2), None
        else:  # deliberately wrong host lr / bc1 / bc2: the kernel must read the device tensor
            sc = (123.0, B1, B2, EPS, WD, 0.5, 0.25)
            lr32, c1, c2 = np.float32(LR), np.float32(bc1), np.float32(bc2)
            hp = torch.tensor(np.array([lr32, lr32 / c1, np.float32(1) / np.sqrt(c2)], dtype=np.float32), device=DEV)
        C.adamw_q8_step(param, master, g, cm, cv, am, av, slots, sm, sv, wd_mask, tab, coef_t, *sc, hp)
        w_ref, m_ref, v_ref = R.adamw_ref(w_prev, g, m_prev.view(-1), v_prev.view(-1), wd_mask, COEF, LR, B1, B2, EPS,
                                          WD, step)
        m_ref, v_ref = m_ref.view(nb, 64), v_ref.view(nb, 64)
        wgot = master if master is not None else param
        fig(f"step {step} w rel-L2", R.rel_l2(wgot, w_ref), 1e-6)
        fig(f"step {step} w elem", R.elem_err(wgot, w_ref), 1e-5)
        if master is not None and not torch.equal(param, master.to(torch.bfloat16)):
            bad.append(f"step {step} param != master.to(bf16)")
        q = ~fp32
        for name, signed, codes, absmax, ref, side in (("m", True, cm, am, m_ref, sm), ("v", False, cv, av, v_ref, sv)):
            if q.any():
                e, a = ref[q], absmax[q]
                want = e.abs().amax(-1)
                fig(f"step {step} absmax_{name} rel", ((a.double() - want).abs() / want.clamp_min(1e-300)).max().item(),
                    2.0 ** -21)
                d = _deq64(codes[q], a, signed)
                over = (d - e).abs() - _nearest_gap(e, a, signed) - 2.0 ** -20 * torch.maximum(e.abs(), d.abs())
                fig(f"step {step} code_{name} beyond nearest (count)", float((over > 0).sum().item()), 0.0)
            if fp32.any():
                fig(f"step {step} side_{name} elem", R.elem_err(side.view(-1, 64)[idx], ref[fp32]), 1e-5)
        if nb > 1 and not fp32[1]:  # the all-zero block: zero scales, the codes of 0.0
            if not (am[1] == 0 and av[1] == 0 and torch.equal(cm[1], zs[0]) and torch.equal(cv[1], zu[0])):
                bad.append(f"step {step} zero block")
    if fp32.any() and not (torch.equal(cm[fp32], cm0[fp32]) and torch.equal(am[fp32], am0[fp32])):
        bad.append("codes / scales of side-store blocks were written")
    if not fp32.all():
        t = torch.from_numpy(q8.SIGNED).to(DEV)[cm[~fp32].long()].abs()
        assert t.max() > 10 * t[t > 0].min(), "the gradients were meant to reach several decades of the code book"
    assert not bad, "\n".join(bad)


REJECTED = [("master", "misaligned", "aligned"), ("grad", "strided", "contiguous"), ("code_m", "misaligned", "aligned"),
            ("wd_mask", "misaligned", "aligned"), ("side_m", "misaligned", "aligned"), ("absmax_v", "strided", "contig")]


def test_adamw_q8_step_rejects_misaligned_and_strided():
    C = _ext.native()
    n, nb = 256, 4
    f, u8 = (lambda k: torch.zeros(k, device=DEV)), (lambda k: torch.ones(k, device=DEV, dtype=torch.uint8))
    ops = dict(param=f(n).bfloat16(), master=f(n), grad=f(n), code_m=u8(n), code_v=u8(n), absmax_m=f(nb), absmax_v=f(nb),
               slots=torch.full((nb,), -1, dtype=torch.int32, device=DEV), side_m=f(64), side_v=f(64), wd_mask=u8(n),
               tables=q8.tables(DEV), coef=torch.ones((), device=DEV))
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.01, 0.1, 0.001)
    C.adamw_q8_step(*ops.values(), *hp)  # the operands as they stand pass
    for name, how, match in REJECTED:
        t = ops[name]
        big = torch.zeros(2 * t.numel() + 8, device=DEV, dtype=t.dtype)
        view = big[1:t.numel() + 1] if how == "misaligned" else big[::2][:t.numel()]
        with pytest.raises(RuntimeError, match=match):
            C.adamw_q8_step(*dict(ops, **{name: view}).values(), *hp)
    with pytest.raises(RuntimeError, match="64"):
        C.adamw_q8_step(*dict(ops, param=f(n + 32).bfloat16()).values(), *hp)
