"""The fp64 attention oracle of tests/test_attn_rows_gpu.py (tests/attn_refs.py) and its bounds, checked without a GPU.

* ``attn_ref`` (explicit backward formulas) against the plain composite under fp64 autograd, to 1e-10;
* against the package's fp32 composite ``ops.attention._reference`` within fp32 rounding, on rows with a visible key;
* its empty-row convention (zero output row, LSE = +inf, no gradient) explicitly;
* the bound condition: for every case of the GPU file, 4 x the bf16 model's per-row error against ``attn_ref`` fits
  5e-2, the loosest attention-gradient bound the suite has used at more than one query row: a condition on the cases'
  inputs, not a measurement of any kernel;
* the metric's sensitivity: three local corruptions of the reference output at the t5-base encoder shape exceed the
  per-row bound and pass the whole-tensor rel-L2 bounds of the older attention tests.
"""
import pytest
import torch

import attn_refs as R
from distributed_llms_example_amd.ops import attention as A
from distributed_llms_example_amd.ops.rng import attention_keep_mask

F64 = torch.float64


def _composite64(r, table=None):
    """softmax(q k^T scale + bias, masked) keep / (1 - p) @ v in fp64 with autograd leaves q, k, v, lut (or table)."""
    c = r.case
    q, k, v = (t.double().requires_grad_(True) for t in (r.q, r.k, r.v))
    lut = None
    if r.lut is not None:
        lut = table.index_select(0, r.idx).t() if table is not None else r.lut.double().requires_grad_(True)
    s = torch.matmul(q.permute(0, 2, 1, 3), k.permute(0, 2, 3, 1)) * r.scale
    if lut is not None:
        s = s + lut[:, R._rel_index(c.Sq, c.Sk, "cpu")].unsqueeze(0)
    s = s.masked_fill(~R.visible(c.B, c.Sq, c.Sk, c.causal, r.kpm, "cpu"), float("-inf"))
    pr = torch.softmax(s, -1)
    if c.p > 0.0:
        pr = pr * attention_keep_mask(c.seed, c.p, c.B, c.H, c.Sq, c.Sk, "cpu").double() / (1.0 - c.p)
    o = torch.matmul(pr, v.permute(0, 2, 1, 3)).permute(0, 2, 1, 3)
    lse2 = torch.logsumexp(s, -1) / R.LN2
    return o, lse2, (q, k, v, lut)


def _close(a, b, tol):
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


AUTOGRAD_CASES = [R.case(37, 37, bias=True, kpm="suffix", causal=True, p=0.1),
                  R.case(21, 70, bias=True, causal=True, p=0.1), R.case(50, 33, kpm="suffix", p=0.1),
                  R.case(45, 130, bias=True, kpm="holes"), R.case(64, 64, causal=True),
                  R.case(33, 75, bias=True, kpm="suffix", p=0.1, D=40)]


@pytest.mark.parametrize("c", AUTOGRAD_CASES, ids=R.case_id)
def test_ref_matches_fp64_autograd(c):
    r = R.make_case(c)
    ref = R.attn_ref(r.q, r.k, r.v, r.do, r.scale, r.causal, r.kpm, r.lut, r.p, seed=r.seed)
    assert not ref.row_empty.any()
    o, lse2, (q, k, v, lut) = _composite64(r)
    grads = torch.autograd.grad(o, [t for t in (q, k, v, lut) if t is not None], r.do.double())
    assert _close(ref.o, o.detach(), 1e-10) and _close(ref.lse2, lse2.detach(), 1e-10)
    for name, g in zip(("dq", "dk", "dv", "dlut"), grads):
        assert _close(getattr(ref, name), g, 1e-10), name
    if c.bias:  # contracted to the bucket table: autograd through index_select against per_bucket
        table = torch.randn(32, c.H, dtype=F64).requires_grad_(True)
        r2 = R.make_case(c)
        r2.lut = table.detach().index_select(0, r2.idx).t().contiguous()
        ref2 = R.attn_ref(r2.q, r2.k, r2.v, r2.do, r2.scale, r2.causal, r2.kpm, r2.lut, r2.p, seed=r2.seed)
        o2, _, _ = _composite64(r2, table)
        (dt,) = torch.autograd.grad(o2, table, r2.do.double())
        assert _close(R.per_bucket(ref2.dlut, r2.idx), dt.t(), 1e-10)
    # the column sums are the sums of the gradients
    assert _close(ref.cs_dk, ref.dk.sum((0, 1)).reshape(-1), 1e-12)


@pytest.mark.parametrize("c", AUTOGRAD_CASES + [R.case(60, 60, kpm="empty", p=0.1)], ids=R.case_id)
def test_ref_matches_package_composite(c):
    """fp32 inputs on the CPU: ``A._reference`` (forward, and its autograd gradients) against ``attn_ref`` within the
    suite's fp32-vs-fp64 row bound (rowwise_refs.ROW_BOUND: 1e-5), on the rows that have a visible key (the composite
    gives an empty row the uniform softmax, the kernels' contract a zero row)."""
    r = R.make_case(c)
    q, k, v = (t.float().requires_grad_(True) for t in (r.q, r.k, r.v))
    lut = r.lut.clone().requires_grad_(True) if r.lut is not None else None
    kpm = r.kpm.bool() if r.kpm is not None else None
    o = A._reference(q, k, v, r.scale, r.causal, kpm, lut, r.p, r.seed)
    ref = R.attn_ref(r.q, r.k, r.v, r.do, r.scale, r.causal, r.kpm, r.lut, r.p, seed=r.seed)
    live = ~ref.row_empty.permute(0, 2, 1)  # [B, Sq, H]
    do = r.do.float() * live.unsqueeze(-1)  # an empty row contributes no gradient: keep the composite's out of it
    grads = torch.autograd.grad(o, [t for t in (q, k, v, lut) if t is not None], do)
    assert R.row_err(o.detach()[live], ref.o[live]) < 1e-5
    for name, g in zip(("dq", "dk", "dv"), grads):
        assert R.row_err(g, getattr(ref, name)) < 1e-5, name
    if lut is not None:
        assert R.mass_err(grads[3], ref.dlut, ref.dlut_mass) < 1e-5


@pytest.mark.parametrize("c", [R.case(60, 60, kpm="empty", p=0.1), R.case(70, 130, bias=True, kpm="empty", causal=True),
                               R.case(80, 50, causal=True), R.case(40, 40, kpm="allpad")], ids=R.case_id)
def test_ref_empty_rows(c):
    """A row without a visible key: o = 0, LSE = +inf, dq = 0 and no contribution to dk, dv, dlut — the other rows are
    what the same call without the empty rows gives."""
    r = R.make_case(c)
    ref = R.attn_ref(r.q, r.k, r.v, r.do, r.scale, r.causal, r.kpm, r.lut, r.p, seed=r.seed)
    vis = R.visible(c.B, c.Sq, c.Sk, c.causal, r.kpm, "cpu")
    empty = ~vis.any(-1).expand(c.B, c.H, c.Sq)
    assert empty.any() and torch.equal(ref.row_empty, empty)
    e_bsh = empty.permute(0, 2, 1)
    assert torch.isposinf(ref.lse2[empty]).all() and torch.isfinite(ref.lse2[~empty]).all()
    assert (ref.o[e_bsh] == 0).all() and (ref.dq[e_bsh] == 0).all()
    assert (ref.dk[ref.key_dead] == 0).all() and (ref.dv[ref.key_dead] == 0).all()
    for n in ("o", "dq", "dk", "dv"):
        assert torch.isfinite(getattr(ref, n)).all(), n
    if c.kpm == "allpad":
        assert (ref.dk == 0).all() and (ref.dv == 0).all() and (ref.o == 0).all()
    elif c.kpm == "empty":
        # the live rows and every key-side sum equal a call in which the empty batch row sees one key and gets a zero
        # output gradient: the empty rows contributed nothing
        kpm2 = r.kpm.clone()
        kpm2[1, 0] = 1
        do2 = r.do.double() * (~e_bsh).unsqueeze(-1)
        ref2 = R.attn_ref(r.q, r.k, r.v, do2, r.scale, r.causal, kpm2, r.lut, r.p, seed=r.seed)
        live = ~e_bsh
        assert _close(ref.o[live], ref2.o[live], 1e-12) and _close(ref.dq[live], ref2.dq[live], 1e-12)
        assert _close(ref.dk, ref2.dk, 1e-12) and _close(ref.dv, ref2.dv, 1e-12)
        if c.bias:
            assert _close(ref.dlut, ref2.dlut, 1e-12)
    else:  # causal, Sq > Sk: the first Sq - Sk rows are empty
        assert empty[:, :, :c.Sq - c.Sk].all() and not empty[:, :, c.Sq - c.Sk:].any()


@pytest.mark.parametrize("c", R.all_gpu_cases(256), ids=R.case_id)
def test_bound_condition(c):
    """4 x the model's per-row error of every bf16 output fits ROW_CAP (5e-2) for every case of the GPU file (built by
    the same make_case; the device-sized cases at 256 CUs). A condition on the inputs: a case that misses it gets
    other inputs (attn_refs.make_case says which were chosen and why), never a larger cap."""
    r = R.make_case(c)
    ref, fig = R.ref_and_figures(r)
    print(f"[model] {R.case_id(c)} " + " ".join(f"{n} {v:.2e}" for n, v in fig.items()))
    for n in ("o", "dq", "dk", "dv"):
        assert R.MODEL_FACTOR * fig[n] <= R.ROW_CAP, (n, fig[n])


def test_metric_sensitivity():
    """Three local faults in the output of the t5-base encoder case (2 x 12 heads x 1024 x 1024, bias, key padding,
    dropout 0.1): each exceeds the per-row bound (4 x the model's row error on these inputs) and passes the
    whole-tensor rel-L2 bound of the older attention tests (2e-2 for o; 3e-2 for gradients is looser still) — which
    could not see them.

    1. one query row replaced by its neighbour;
    2. the last valid key of a ragged 64-key tile (batch row 1 ends at key 1024 - 82 = 942) dropped from the 128 rows of
       one query tile of one head;
    3. the dropout bits of one wave's 32-row tile of one head shifted by one key."""
    c = R.case(1024, 1024, B=2, H=12, bias=True, kpm="suffix", p=0.1)
    r = R.make_case(c)
    ref, fig = R.ref_and_figures(r, fwd_only=True)
    ref = ref.o
    bound = R.MODEL_FACTOR * fig["o"]
    assert bound <= R.ROW_CAP
    last = int(r.kpm[1].sum()) - 1
    assert last == 1024 - 82 - 1 and (last + 1) % 64 != 0

    def rows(b, h, q0, q1, kpm_row, keep):
        """o of rows q0..q1 of (b, h) in fp64 with another key mask / keep mask."""
        sl = lambda t: t[b:b + 1, :, h:h + 1]
        return R.attn_ref(r.q[b:b + 1, q0:q1, h:h + 1], sl(r.k), sl(r.v), r.do[b:b + 1, q0:q1, h:h + 1], r.scale, False,
                          kpm_row.view(1, -1), r.lut[h:h + 1, 1023 - q0 - (q1 - q0 - 1):1023 - q0 + 1024], r.p,
                          keep=keep, fwd_only=True).o[0, :, 0]

    keep = attention_keep_mask(r.seed, r.p, c.B, c.H, c.Sq, c.Sk, "cpu")
    # the slicing helper reproduces the reference where nothing is corrupted
    assert _close(rows(1, 3, 256, 384, r.kpm[1], keep[1:2, 3:4, 256:384]), ref[1, 256:384, 3], 1e-12)
    bad1 = ref.clone()
    bad1[0, 517, 5] = ref[0, 518, 5]
    kpm_drop = r.kpm[1].clone()
    kpm_drop[last] = 0
    bad2 = ref.clone()
    bad2[1, 256:384, 3] = rows(1, 3, 256, 384, kpm_drop, keep[1:2, 3:4, 256:384])
    bad3 = ref.clone()
    bad3[0, 640:672, 7] = rows(0, 7, 640, 672, r.kpm[0], torch.roll(keep[0:1, 7:8, 640:672], 1, -1))
    for name, bad in (("row replaced", bad1), ("ragged-tile key dropped", bad2), ("dropout bits shifted", bad3)):
        re, l2 = R.row_err(bad, ref), R.rel_l2(bad, ref)
        print(f"[sens] {name}: row_err {re:.3e} (bound {bound:.2e})  whole-tensor rel-L2 {l2:.3e} (old bound 2e-2)")
        assert re > bound, name
        assert l2 < 2e-2, name
