"""The preference-loss kernels (csrc/pref.hip) and everything above them, on the GPU, against fp64.

``pref_fwd`` / ``pref_pairs`` / ``pref_bwd`` on the stored inputs (tests/loss_refs.py: ``peaked_logits``,
``edge_labels``, ``ce_ref`` with ``eps = 0``, which gives ``-lp``, ``lse`` and the unit gradient), each shape in bf16
and fp32, with and without biases, in place and out of place; the chunk kernels on ops/lm_head.py's chunk table (a
ragged 5-column tail) and through ``lm_head_preference_loss``; bit-identical reruns; the bindings' argument checks;
model level and one graphed step.

Bounds.  ``lp`` and ``lse``: per row ``loss_refs.row_metric <= LOSS_BOUND``.  Everything ``pref_pairs`` forms is a
function of the four sequence sums of a pair, so its bounds are propagated from the per-row bound, in the test:

  b_r      = LOSS_BOUND max(1, |lp_r|) on a valid row (what the per-row check allows), 0 on an invalid one
  b(L_s)   = sum of b_r over the sequence's rows
  b(u)     the bound on the pair's margin variable u: u = h, b(h) = beta (b(L^pi_c) + b(L^pi_r) + b(L^ref_c) +
           b(L^ref_r)) for sigmoid and hinge; u = hbar, b(hbar) = the same sum with every b(L_s) divided by n_s for ipo
  b(l)     = b(u) |dl/du|: l is convex in u, so over [u - b(u), u + b(u)] it leaves l(u) by at most the larger endpoint
           deviation upwards and by |l'(u)| b(u) downwards — the first-order bound with the derivative taken where on
           the interval it is largest, which is what keeps the bound valid where l'(u) = 0 (hinge beyond the margin,
           the minimum of a smoothed sigmoid or of ipo) — plus sft_alpha b(L^pi_c) / n_c for the sft term
  b(c_r)   = |G / P_step| k |l'(u +- b(u)) - l'(u)| (l' is monotone: the endpoints bound it; k = beta, or 1 / n_s for
           ipo); the sft part of c is exact
  rewards  beta (b(L^pi_s) + b(L^ref_s)); logps b(L^pi_s); the logged means: the mean of the pairs' bounds
  every stored fp32 value may also be off by its own rounding, U32 |ref|, added to each of the above.

``dx``: per element ``grad_bound`` with ``ce_abs_term`` scaled by ``|c_r|``, the reference formed from the KERNEL's
``c`` so that ``pref_bwd`` is judged alone; rows with ``c_r == 0`` must be exactly 0.  Every figure is printed before a
test asserts (run with -s to collect them).
"""
import copy
import math

import pytest
import torch

import loss_refs as L
import rowwise_refs as R
from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops import preference as PR
from distributed_llms_example_amd.ops import routing

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF16, "fp32": F32}
IGN = L.IGNORE
BETA, EPS, SFT, G_UP = 0.3, 0.1, 0.5, 0.37
KINDS = PR.KINDS
SHAPES = [(3, 5, 1003), (2, 4, 50265), (4, 8, 32128), (1, 3, 250112), (600, 4, 520)]


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _view(x, off):
    """``x`` [N, V] as a contiguous view ``off`` elements into a larger buffer; (view, buffer)."""
    buf = torch.zeros(x.numel() + 16, device=x.device, dtype=x.dtype)
    buf[off:off + x.numel()] = x.reshape(-1)
    return buf[off:off + x.numel()].view(x.shape), buf


_CACHE = {}


def _inputs(P, T, V, dtype, bias):
    """Stored logits of both models, labels, biases and their fp64 reference — computed once per case, shared by the
    in-place and out-of-place tests and never written to."""
    key = (P, T, V, dtype, bias)
    if key not in _CACHE:
        if len(_CACHE) >= 4:
            _CACHE.clear()
        N = 2 * P * T
        gen = _gen(V + 3 * P + (1 if bias else 0))
        x = L.peaked_logits(N, V, DEV, gen).to(dtype)
        r = (0.7 * x.float() + L.peaked_logits(N, V, DEV, gen, scale=1.0, boost=0.0)).to(dtype)
        labels = L.edge_labels(N, V, DEV, gen)
        if P >= 3:
            labels[2 * T:3 * T] = IGN  # a fully ignored sequence: pair 1's chosen
        bp = L.dyadic_bias(V, DEV, gen) if bias else None
        br = L.dyadic_bias(V, DEV, gen, boost=1.0) if bias else None
        nlp, lse, d = L.ce_ref(x, labels, bp, 0.0, IGN, V)
        nlr, _, _ = L.ce_ref(r, labels, br, 0.0, IGN, V)
        _CACHE[key] = dict(x=x, r=r, labels=labels, bp=bp, br=br, lp=-nlp, lpr=-nlr, lse=lse, d=d,
                           valid=L.valid_rows(labels, IGN, V), term=L.ce_abs_term(x, labels, bp, 0.0, IGN, V))
    return _CACHE[key]


# ------------------------------------------------------------------------------------- fp64 pair math and its bounds
def _ell(kind, u, eps, beta):
    """(l(u), l'(u)) of the pair loss in its margin variable, fp64 tensors."""
    if kind == "sigmoid":
        sp = torch.nn.functional.softplus
        return (1 - eps) * sp(-u) + eps * sp(u), -(1 - eps) * torch.sigmoid(-u) + eps * torch.sigmoid(u)
    if kind == "hinge":
        return (1 - u).clamp_min(0.0), torch.where(u < 1, -torch.ones_like(u), torch.zeros_like(u))
    d = u - 1.0 / (2.0 * beta)
    return d * d, 2.0 * d


def _pairs_ref(lp, lpr, valid, T, kind, g, ip, beta=BETA, eps=EPS, sft=SFT):
    """fp64 reference of pref_pairs and the propagated bounds (module docstring).  Returns (ref, bound): dicts with
    'h', 'l', 'rw_c', 'rw_r', 'lp_c', 'lp_r' [P], 'coef' [N] and 'out' [7]."""
    P = lp.numel() // (2 * T)
    v = valid.view(2 * P, T)
    b_row = torch.where(valid, L.LOSS_BOUND * lp.abs().clamp_min(1.0), torch.zeros_like(lp)).view(2 * P, T)
    b_rowr = torch.where(valid, L.LOSS_BOUND * lpr.abs().clamp_min(1.0), torch.zeros_like(lpr)).view(2 * P, T)
    Lp, Lr = lp.view(2 * P, T).sum(1).view(P, 2), lpr.view(2 * P, T).sum(1).view(P, 2)
    bLp, bLr = b_row.sum(1).view(P, 2), b_rowr.sum(1).view(P, 2)
    n = v.sum(1).clamp_min(1).double().view(P, 2)
    h = beta * ((Lp[:, 0] - Lp[:, 1]) - (Lr[:, 0] - Lr[:, 1]))
    bh = beta * (bLp.sum(1) + bLr.sum(1))
    if kind == "ipo":
        u = (Lp[:, 0] / n[:, 0] - Lp[:, 1] / n[:, 1]) - (Lr[:, 0] / n[:, 0] - Lr[:, 1] / n[:, 1])
        bu = ((bLp + bLr) / n).sum(1)
        k = 1.0 / n
    else:
        u, bu, k = h, bh, torch.full_like(n, beta)
    l, dl = _ell(kind, u, eps, beta)
    (lhi, dhi), (llo, dlo) = _ell(kind, u + bu, eps, beta), _ell(kind, u - bu, eps, beta)
    bl = torch.maximum(torch.maximum((lhi - l).abs(), (llo - l).abs()), dl.abs() * bu) + sft * bLp[:, 0] / n[:, 0]
    bdl = torch.maximum((dhi - dl).abs(), (dlo - dl).abs())
    l = l + sft * (-Lp[:, 0] / n[:, 0])
    dL = torch.stack([dl * k[:, 0] - sft / n[:, 0], -dl * k[:, 1]], 1)  # dl/dL^pi_c, dl/dL^pi_r
    coef_seq = (-g * ip * dL).reshape(2 * P)
    bcoef_seq = (abs(g * ip) * bdl.view(P, 1) * k).reshape(2 * P)
    coef = torch.where(valid, coef_seq.view(-1, 1).expand(2 * P, T).reshape(-1), torch.zeros_like(lp))
    bcoef = bcoef_seq.view(-1, 1).expand(2 * P, T).reshape(-1)
    rc, rr = beta * (Lp[:, 0] - Lr[:, 0]), beta * (Lp[:, 1] - Lr[:, 1])
    brc, brr = beta * (bLp[:, 0] + bLr[:, 0]), beta * (bLp[:, 1] + bLr[:, 1])
    ref = dict(h=h, l=l, rw_c=rc, rw_r=rr, lp_c=Lp[:, 0], lp_r=Lp[:, 1], coef=coef, n_c=n[:, 0], n_r=n[:, 1])
    bound = dict(h=bh, l=bl, rw_c=brc, rw_r=brr, lp_c=bLp[:, 0], lp_r=bLp[:, 1], coef=bcoef)
    sure = (rc - rr).abs() > brc + brr  # pairs whose accuracy bit the bounds decide
    acc_lo = ((rc > rr) & sure).double().sum() / P
    acc_hi = ((rc > rr) | ~sure).double().sum() / P
    # 'out' without rewards/accuracies (a count, not a sum of bounded terms): NO_ACC picks the other six columns
    ref["out"] = torch.stack([l.sum() * ip, rc.mean(), rr.mean(), (rc - rr).mean(), Lp[:, 0].mean(), Lp[:, 1].mean()])
    bound["out"] = torch.stack([bl.sum() * abs(ip), brc.mean(), brr.mean(), (brc + brr).mean(), bLp[:, 0].mean(),
                                bLp[:, 1].mean()])
    ref["acc"] = (acc_lo.item(), acc_hi.item())  # the range the pairs whose margin is inside its bound leave open
    for key in bound:  # the fp32 store of each value
        bound[key] = bound[key] + L.U32 * ref[key].abs()
    return ref, bound


def _worst(got, ref, bound):
    """max |got - ref| / bound; 0 / 0 counts as 0 (an exact value that must be hit exactly), a non-finite got as inf."""
    err = (got.detach().double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return ratio.max().item()


NO_ACC = [0, 1, 2, 3, 5, 6]


def _acc_ok(got, rng):
    return rng[0] - 2 * L.U32 <= float(got) <= rng[1] + 2 * L.U32


PAIR_COLS = dict(l=0, h=1, rw_c=2, rw_r=3, lp_c=4, lp_r=5, n_c=6, n_r=7)


def _check_pairs(F, C, lp_pi, lp_ref, c, T, V):
    """pref_pairs (fed the kernel's own row log-probabilities) for every loss kind against the fp64 pair math on the
    fp64 rows, within the bounds propagated from the per-row bound; returns each kind's coefficients."""
    g = torch.full((1,), G_UP, device=DEV)
    P = lp_pi.numel() // (2 * T)
    ip = torch.full((1,), 1.0 / (P + 2), device=DEV)  # P_step > P: other micro-batches hold two more pairs
    coefs = {}
    for kind in KINDS:
        out, pair_out, coef = C.pref_pairs(lp_pi, lp_ref, c["labels"], g, ip, T, V, IGN, BETA, KINDS.index(kind), EPS,
                                           SFT)
        ref, bound = _pairs_ref(c["lp"], c["lpr"], c["valid"], T, kind, float(g.double()), float(ip.double()))
        for name, col in PAIR_COLS.items():
            if name in ("n_c", "n_r"):
                F.check(f"{kind} {name} exact", torch.equal(pair_out[:, col].double(), ref[name]))
            else:
                F.fold(f"{name}", _worst(pair_out[:, col], ref[name], bound[name]), 1.0, kind)
        F.fold("c", _worst(coef, ref["coef"], bound["coef"]), 1.0, kind)
        F.fold("loss and logged means", _worst(out[NO_ACC], ref["out"], bound["out"]), 1.0, kind)
        F.check(f"{kind} rewards/accuracies {out[4].item():.4f} in {ref['acc']}", _acc_ok(out[4], ref["acc"]))
        F.check(f"{kind} c == 0 on invalid rows", not coef[~c["valid"]].any())
        F.check(f"{kind} finite", bool(torch.isfinite(out).all() and torch.isfinite(coef).all()))
        out1, _, coef1 = C.pref_pairs(lp_pi, lp_ref, c["labels"], None, ip, T, V, IGN, BETA, KINDS.index(kind), EPS,
                                      SFT)
        F.check(f"{kind} G absent is G = 1", torch.equal(out1, out) and
                _worst(coef1 * G_UP, coef.double(), 4 * L.U32 * coef.double().abs() + 1e-300) <= 1.0)
        coefs[kind] = coef
    return coefs


def _check_bwd(F, C, c, xv, xbuf, lse, coef, dtype, inplace, tag):
    N, V = xv.shape
    ref = coef.double().view(-1, 1) * c["d"]  # the kernel's own c: pref_bwd judged alone
    bound = L.grad_bound(ref, c["term"] * coef.double().abs().view(-1, 1), dtype).clamp_min(5e-324)
    before = xbuf.clone()
    out = C.pref_bwd(coef, xv, c["labels"], lse, c["bp"], inplace)
    if inplace:
        F.check(f"{tag} in place: same storage", out.data_ptr() == xv.data_ptr())
        F.check(f"{tag} in place: neighbours of the view untouched",
                torch.equal(xbuf[:1], before[:1]) and torch.equal(xbuf[1 + N * V:], before[1 + N * V:]))
    else:
        F.check(f"{tag} out of place: the policy logits are untouched", torch.equal(xbuf, before))
    worst, where = L.grad_worst(out, ref, bound)
    F.fold("dx per element (x of the bound)", worst, 1.0, f"{tag} at {where}")
    zero = coef == 0
    F.check(f"{tag} c_r == 0 rows are exactly 0 ({int(zero.sum())} rows)", bool(zero.any()) and not out[zero].any())
    F.check(f"{tag} c_r != 0 rows carry a gradient", bool(out[~zero].any()))


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pref_kernels(shape, dt, bias, inplace):
    P, T, V = shape
    dtype = DT[dt]
    C = _ext.native()
    c = _inputs(P, T, V, dtype, bias)
    F = L.Figures(f"pref P={P} T={T} V={V} {dt} bias={bias} inplace={inplace}")
    # the policy one element, the reference two elements past a 16-B boundary: rows of both at their own phases
    xv, xbuf = _view(c["x"], 1)
    rv, _ = _view(c["r"], 2)
    lp_pi, lp_ref, lse = C.pref_fwd(xv, rv, c["labels"], c["bp"], c["br"], IGN)
    F.add("lp_pi per row", L.row_metric(lp_pi, c["lp"]), L.LOSS_BOUND)
    F.add("lp_ref per row", L.row_metric(lp_ref, c["lpr"]), L.LOSS_BOUND)
    F.add("lse_pi per row", L.row_metric(lse, c["lse"]), L.LOSS_BOUND)
    F.check("invalid rows: lp = 0", not lp_pi[~c["valid"]].any() and not lp_ref[~c["valid"]].any())
    a, b, e = C.pref_fwd(xv, None, c["labels"], c["bp"], None, IGN)  # the policy alone
    F.check("policy alone: the same lp_pi and lse, lp_ref = 0", torch.equal(a, lp_pi) and torch.equal(e, lse)
            and not b.any())
    coefs = _check_pairs(F, C, lp_pi, lp_ref, c, T, V)
    kinds = KINDS if not inplace else ("sigmoid",)  # in place consumes the view: one kind (hinge zeroes whole pairs)
    for kind in kinds:
        _check_bwd(F, C, c, xv, xbuf, lse, coefs[kind], dtype, inplace, kind)
    F.done()


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_pairs_h_of_80_is_finite(sign):
    """|h| = 80 in every kind: finite loss and coefficients, equal to fp64."""
    C = _ext.native()
    T, V = 1, 7
    lp_pi = torch.tensor([-1.0, -801.0] if sign > 0 else [-801.0, -1.0], device=DEV)
    lp_ref = torch.zeros(2, device=DEV)
    labels = torch.tensor([1, 2], device=DEV)
    one = torch.ones(1, device=DEV)
    F = L.Figures(f"pref |h| = 80 sign={sign}")
    for kind in KINDS:
        out, pair_out, coef = C.pref_pairs(lp_pi, lp_ref, labels, one, one, T, V, IGN, 0.1, KINDS.index(kind), EPS, 0.0)
        F.check(f"{kind} finite", bool(torch.isfinite(out).all() and torch.isfinite(coef).all()))
        F.add(f"{kind} h", abs(pair_out[0, 1].item() - sign * 80.0), 1e-4)
        l, dl = _ell(kind, torch.tensor(sign * 80.0 if kind != "ipo" else sign * 800.0, dtype=torch.float64), EPS, 0.1)
        F.add(f"{kind} loss", abs(out[0].item() - l.item()), 2 * L.U32 * max(1.0, abs(l.item())))
        k = 0.1 if kind != "ipo" else 1.0
        F.add(f"{kind} c", abs(coef[0].item() + dl.item() * k), 2 * L.U32 * max(1e-30, abs(dl.item() * k)))
    F.done()


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_pref_reruns_bit_identical(dt):
    C = _ext.native()
    P, T, V = 3, 5, 1003
    c = _inputs(P, T, V, DT[dt], True)
    g, ip = torch.full((1,), G_UP, device=DEV), torch.full((1,), 1.0 / P, device=DEV)
    runs = []
    for _ in range(2):
        lp_pi, lp_ref, lse = C.pref_fwd(c["x"], c["r"], c["labels"], c["bp"], c["br"], IGN)
        out, pair_out, coef = C.pref_pairs(lp_pi, lp_ref, c["labels"], g, ip, T, V, IGN, BETA, 0, EPS, SFT)
        dx = C.pref_bwd(coef, c["x"], c["labels"], lse, c["bp"], False)
        runs.append((lp_pi, lp_ref, lse, out, pair_out, coef, dx))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    # the op: loss, statistics and gradient
    got = []
    for _ in range(2):
        x = c["x"].clone().requires_grad_(True)
        loss, stats = PR.preference_loss(x, c["r"], c["labels"], T, bias=c["bp"], ref_bias=c["br"], beta=BETA,
                                         label_smoothing=EPS, sft_alpha=SFT)
        loss.backward()
        got.append([loss.detach(), x.grad] + [stats[k] for k in PR.STAT_NAMES])
    assert all(torch.equal(a, b) for a, b in zip(*got))


# ------------------------------------------------------------------------------------------- vocabulary chunks
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_pref_chunk_kernels(bias):
    """Chunk edges of ops/lm_head.py's table at V = 1029 in 256-column chunks: four full chunks and a ragged tail that
    holds 5 new columns (it re-covers 1021 .. 1023 and skips them).  Labels in the first chunk, the last chunk, the
    re-covered columns and on every chunk edge; the merged state must give what the unchunked kernels give, within
    the same bounds, and the assembled gradient likewise."""
    C = _ext.native()
    P, T, V = 4, 5, 1029
    N = 2 * P * T
    chunks = PR._chunks(V, 256)
    assert chunks[-1] == (1021, 8, 3) and len(chunks) == 5
    gen = _gen(29)
    x = L.peaked_logits(N, V, DEV, gen).to(BF16)
    r = (0.7 * x.float() + L.peaked_logits(N, V, DEV, gen, scale=1.0, boost=0.0)).to(BF16)
    labels = L.edge_labels(N, V, DEV, gen)
    labels[9:20] = torch.tensor([0, 3, 255, 256, 767, 768, 1020, 1021, 1023, 1024, 1028], device=DEV)
    bp = L.dyadic_bias(V, DEV, gen) if bias else None
    br = L.dyadic_bias(V, DEV, gen, boost=1.0) if bias else None
    nlp, lse_r, d = L.ce_ref(x, labels, bp, 0.0, IGN, V)
    nlr, _, _ = L.ce_ref(r, labels, br, 0.0, IGN, V)
    state = torch.empty(N, 6, device=DEV)
    lp_pi, lp_ref, lse = (torch.empty(N, device=DEV) for _ in range(3))
    for j, (c0, n, skip) in enumerate(chunks):
        C.pref_chunk_fwd(x[:, c0:c0 + n].contiguous(), r[:, c0:c0 + n].contiguous(), labels, bp, br, state, lp_pi,
                         lp_ref, lse, c0, V, IGN, j == 0, j + 1 == len(chunks), skip)
    F = L.Figures(f"pref chunks V={V} bias={bias}")
    F.add("lp_pi per row", L.row_metric(lp_pi, -nlp), L.LOSS_BOUND)
    F.add("lp_ref per row", L.row_metric(lp_ref, -nlr), L.LOSS_BOUND)
    F.add("lse_pi per row", L.row_metric(lse, lse_r), L.LOSS_BOUND)
    a, b, e = C.pref_fwd(x, r, labels, bp, br, IGN)  # the unchunked kernels on the same logits
    F.add("lp_pi vs unchunked", L.row_metric(lp_pi, a.double()), L.LOSS_BOUND)
    F.add("lp_ref vs unchunked", L.row_metric(lp_ref, b.double()), L.LOSS_BOUND)
    F.add("lse_pi vs unchunked", L.row_metric(lse, e.double()), L.LOSS_BOUND)
    g, ip = torch.full((1,), G_UP, device=DEV), torch.full((1,), 1.0 / P, device=DEV)
    _, _, coef = C.pref_pairs(lp_pi, lp_ref, labels, g, ip, T, V, IGN, BETA, 0, EPS, SFT)
    dx = torch.full((N, V), float("nan"), device=DEV, dtype=BF16)
    for c0, n, skip in chunks:
        buf = x[:, c0:c0 + n].contiguous()
        C.pref_chunk_bwd(coef, buf, labels, lse, bp, c0, V, skip)
        F.check(f"chunk at {c0}: skipped columns are 0", not buf[:, :skip].any())
        dx[:, c0 + skip:c0 + n] = buf[:, skip:]
    ref = coef.double().view(-1, 1) * d
    term = L.ce_abs_term(x, labels, bp, 0.0, IGN, V) * coef.double().abs().view(-1, 1)
    worst, where = L.grad_worst(dx, ref, L.grad_bound(ref, term, BF16).clamp_min(5e-324))
    F.add(f"dx per element (x of the bound) at {where}", worst, 1.0)
    full = C.pref_bwd(coef, x, labels, e, bp, False)
    worst, where = L.grad_worst(dx, full.double(), (2 * (L.G.BF16_REL * ref.abs() + term)).clamp_min(5e-324))
    F.add(f"dx vs unchunked (x of the bound) at {where}", worst, 1.0)
    zero = coef == 0
    F.check("c_r == 0 rows are exactly 0", bool(zero.any()) and not dx[zero].any())
    F.done()


class _Spy:
    """The native module with the names of the called bindings recorded."""

    def __init__(self, calls, real):
        self.calls, self.real = calls, real

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not callable(fn):
            return fn

        def wrapped(*a, **k):
            self.calls.append(name)
            return fn(*a, **k)
        return wrapped


@pytest.fixture
def calls(monkeypatch):
    out = []
    spy = _Spy(out, _ext.native())
    monkeypatch.setattr(PR._ext, "native", lambda: spy)
    return out


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_lm_head_preference_loss_chunks(bias, calls):
    """The no-materialised-logits op on exact operands (loss_refs.lm_operands: every logit exact in the fp32
    accumulator, so both paths round the same value to bf16) against fp64 of the bf16 logits, and against the
    full-logits op; the reference gets no gradient and its chunk is not recomputed in the backward."""
    P, T, V, d, dr = 3, 6, 1029, 64, 32
    N = 2 * P * T
    gen = _gen(31)
    h, w = L.lm_operands(N, d, V, DEV, gen)
    rh, rw = L.lm_operands(N, dr, V, DEV, gen)
    labels = L.edge_labels(N, V, DEV, gen)
    labels[9:14] = torch.tensor([3, 1020, 1021, 1024, 1028], device=DEV)
    bp = L.dyadic_bias(V, DEV, gen) if bias else None
    br = L.dyadic_bias(V, DEV, gen, boost=1.0) if bias else None
    kw = dict(bias=bp, ref_bias=br, beta=BETA, label_smoothing=EPS, sft_alpha=SFT)
    xl, rl = (h.float() @ w.float().t()).to(BF16), (rh.float() @ rw.float().t()).to(BF16)
    h64, w64 = h.double().requires_grad_(True), w.double().requires_grad_(True)
    x64 = (h64 @ w64.t())
    x64 = x64 + (xl.double() - x64).detach()  # the bf16-rounded logits, differentiable through the exact product
    loss_r, stats_r = PR._reference(x64, rl.double(), labels, T, None if bp is None else bp.double(),
                                    None if br is None else br.double(), BETA, "sigmoid", EPS, SFT)
    loss_r.backward()
    hg, wg = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    rhg, rwg = rh.clone().requires_grad_(True), rw.clone().requires_grad_(True)
    loss, stats = PR.lm_head_preference_loss(hg, wg, rhg, rwg, labels, T, chunk_cols=256, **kw)
    loss.backward()
    n = len(PR._chunks(V, 256))
    assert calls.count("pref_chunk_fwd") == n and calls.count("pref_chunk_bwd") == n and "pref_fwd" not in calls, calls
    F = L.Figures(f"pref lm-head chunks bias={bias}")
    nlp, _, _ = L.ce_ref(xl, labels, bp, 0.0, IGN, V)  # fp64 rows of the bf16 logits both paths hold
    nlr, _, _ = L.ce_ref(rl, labels, br, 0.0, IGN, V)
    ref, bound = _pairs_ref(-nlp, -nlr, L.valid_rows(labels, IGN, V), T, "sigmoid", 1.0, 1.0 / P)
    got = torch.stack([loss.detach()] + [stats[k] for k in PR.STAT_NAMES])
    F.add("loss and logged means (x of the bound)", _worst(got[NO_ACC], ref["out"], bound["out"]), 1.0)
    F.check("rewards/accuracies", _acc_ok(got[4], ref["acc"]))
    F.add("loss vs the composite", abs(loss.item() - loss_r.item()), bound["out"][0].item())
    F.add("dh per row", R.row_err(hg.grad, h64.grad), R.ROW_BOUND[BF16])
    F.add("dW per row", R.row_err(wg.grad, w64.grad), R.ROW_BOUND[BF16])
    F.check("no gradient reaches the reference", rhg.grad is None and rwg.grad is None)
    del calls[:]
    xg = xl.clone().requires_grad_(True)
    full, fstats = PR.preference_loss(xg, rl, labels, T, **kw)
    assert calls == ["pref_fwd", "pref_pairs"], calls
    full.backward()
    assert calls == ["pref_fwd", "pref_pairs", "pref_pairs", "pref_bwd"], calls
    gotf = torch.stack([full.detach()] + [fstats[k] for k in PR.STAT_NAMES])
    F.add("chunked vs full-logits op (x of the bound)", _worst(got[NO_ACC], gotf[NO_ACC].double(), 2 * bound["out"]),
          1.0)
    F.check("chunked vs full-logits op: rewards/accuracies", _acc_ok(gotf[4], ref["acc"]))
    F.done()


def test_routes(calls, monkeypatch):
    P, T, V = 2, 3, 520
    c = _inputs(P, T, V, BF16, False)
    kw = dict(beta=BETA, label_smoothing=EPS)
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(pref="composite"))
    a, _ = PR.preference_loss(c["x"], c["r"], c["labels"], T, **kw)
    assert calls == []
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(pref="fused"))
    b, _ = PR.preference_loss(c["x"], c["r"], c["labels"], T, **kw)
    assert calls == ["pref_fwd", "pref_pairs"]
    assert abs(a.item() - b.item()) < 1e-3 * max(1.0, abs(a.item()))


def test_bindings_reject_malformed_arguments():
    C = _ext.native()
    N, V, T = 12, 520, 3
    x = torch.zeros(N, V, device=DEV)
    labels = torch.zeros(N, dtype=torch.long, device=DEV)
    lp, lpr, lse = C.pref_fwd(x, x, labels, None, None, IGN)
    one = torch.ones(1, device=DEV)
    wide = torch.zeros(N, V + 8, device=DEV)
    with pytest.raises(RuntimeError, match="policy"):
        C.pref_fwd(wide[:, :V], x, labels, None, None, IGN)
    with pytest.raises(RuntimeError, match="reference"):
        C.pref_fwd(x, x.to(BF16), labels, None, None, IGN)
    with pytest.raises(RuntimeError, match="reference"):
        C.pref_fwd(x, x[:N - 1], labels, None, None, IGN)
    with pytest.raises(RuntimeError, match="labels"):
        C.pref_fwd(x, x, labels[:N - 1], None, None, IGN)
    with pytest.raises(RuntimeError, match="bias"):
        C.pref_fwd(x, x, labels, torch.zeros(V - 1, device=DEV), None, IGN)
    with pytest.raises(RuntimeError, match="ref_bias"):
        C.pref_fwd(x, None, labels, None, torch.zeros(V, device=DEV), IGN)
    with pytest.raises(RuntimeError, match="2 P T"):
        C.pref_pairs(lp, lpr, labels, one, one, 5, V, IGN, 0.1, 0, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="beta"):
        C.pref_pairs(lp, lpr, labels, one, one, T, V, IGN, 0.0, 0, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="smoothing"):
        C.pref_pairs(lp, lpr, labels, one, one, T, V, IGN, 0.1, 0, 0.5, 0.0)
    with pytest.raises(RuntimeError, match="kind"):
        C.pref_pairs(lp, lpr, labels, one, one, T, V, IGN, 0.1, 3, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="lp_ref"):
        C.pref_pairs(lp, lpr[:N - 1], labels, one, one, T, V, IGN, 0.1, 0, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="inv_pairs"):
        C.pref_pairs(lp, lpr, labels, one, one.cpu(), T, V, IGN, 0.1, 0, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="coef"):
        C.pref_bwd(lp[:N - 1], x, labels, lse, None, False)
    with pytest.raises(RuntimeError, match="lse"):
        C.pref_bwd(lp, x, labels, lse.double(), None, False)
    cs = torch.zeros(N, 256, device=DEV, dtype=BF16)
    state = torch.zeros(N, 6, device=DEV)
    C.pref_chunk_fwd(cs, cs, labels, None, None, state, lp, lpr, lse, 0, V, IGN, True, False, 0)
    with pytest.raises(RuntimeError, match="policy"):
        C.pref_chunk_fwd(cs.float(), cs, labels, None, None, state, lp, lpr, lse, 0, V, IGN, True, False, 0)
    with pytest.raises(RuntimeError, match="reference"):
        C.pref_chunk_fwd(cs, cs[:, :252], labels, None, None, state, lp, lpr, lse, 0, V, IGN, True, False, 0)
    with pytest.raises(RuntimeError, match="state"):
        C.pref_chunk_fwd(cs, cs, labels, None, None, state[:, :4].contiguous(), lp, lpr, lse, 0, V, IGN, True, False, 0)
    with pytest.raises(RuntimeError, match="vocabulary"):
        C.pref_chunk_fwd(cs, cs, labels, None, None, state, lp, lpr, lse, V - 8, V, IGN, True, False, 0)
    with pytest.raises(RuntimeError, match="skip"):
        C.pref_chunk_fwd(cs, cs, labels, None, None, state, lp, lpr, lse, 0, V, IGN, True, False, 256)
    with pytest.raises(RuntimeError, match="skip"):
        C.pref_chunk_bwd(lp, cs, labels, lse, None, 0, V, 256)
    with pytest.raises(RuntimeError, match="labels"):
        C.pref_chunk_bwd(lp, cs, labels[:N - 1], lse, None, 0, V, 0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- model level
def _grad_report(m_test, m_ref):
    """Per parameter: relative L2 error and cosine of the test model's gradient against the reference's
    (tests/test_model_gpu.py)."""
    rep = []
    for (n, pt), (_, pr) in zip(m_test.named_parameters(), m_ref.named_parameters()):
        if pr.grad is None or pr.grad.norm() == 0:
            continue
        gt, gr = pt.grad.float().flatten(), pr.grad.float().flatten()
        rel = ((gt - gr).norm() / gr.norm()).item()
        cos = torch.nn.functional.cosine_similarity(gt, gr, dim=0).item()
        rep.append((rel, cos, n))
    return rep


def _stepped(policy, ref, batch, seed=5):
    from distributed_llms_example_amd.models import Preference
    from distributed_llms_example_amd.ops.rng import manual_seed
    manual_seed(seed)  # same dropout masks on every path; the reference (eval) draws none
    with torch.no_grad():
        rh, rw, rb = ref.lm_head_operands(**batch)
    out = policy(**batch, preference=Preference(rh, rw, rb, beta=0.5, sft_alpha=0.25))
    out.loss.backward()
    return out


@pytest.mark.parametrize("name", ["dpo-tiny", "bart-tiny"])
def test_model_step_fused_vs_composite(name, calls, monkeypatch):
    """A bf16 policy and reference with ``pref=fused`` against the same models in fp32 with ``pref=composite``, by the
    method and bounds of tests/test_distill_gpu.py::test_model_distill_bf16_vs_fp32_composite: bf16-representable
    weights, the same dropout masks, the loss within 1 %, every parameter's gradient within 1.5x of what the torch
    composite run in bf16 costs on that parameter (floors 3e-2 relative, 1e-3 cosine deficit)."""
    from distributed_llms_example_amd.models import build_model, resolve_config
    cfg = resolve_config(name)
    torch.manual_seed(0)
    r32 = build_model(cfg).to(DEV)
    with torch.no_grad():
        if name.startswith("bart"):
            r32.final_logits_bias.normal_(0.0, 0.5)
        for p in r32.parameters():
            p.copy_(p.to(BF16).float())
        for b in r32.buffers():
            if b.is_floating_point():
                b.copy_(b.to(BF16).float())
    m32 = copy.deepcopy(r32)
    with torch.no_grad():  # a policy that has moved away from its reference
        for p in m32.parameters():
            p.copy_((p + 0.02 * torch.randn_like(p)).to(BF16).float())
    r32.eval().requires_grad_(False)
    m32.train()
    m16, c16 = (copy.deepcopy(m32).to(BF16).train() for _ in range(2))
    r16 = copy.deepcopy(r32).to(BF16).eval()
    P, S, T = 3, 200, 40
    g = torch.Generator().manual_seed(0)
    batch = {"input_ids": torch.randint(3, cfg.vocab_size, (P, S), generator=g).to(DEV),
             "attention_mask": torch.ones(P, S, dtype=torch.long, device=DEV),
             "labels": torch.randint(3, cfg.vocab_size, (2 * P, T), generator=g).to(DEV)}
    batch["attention_mask"][1, -33:] = 0
    batch["labels"][2, -5:] = -100
    batch["labels"][5, -17:] = -100
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(pref="composite"))
    monkeypatch.setenv("DLLM_REFERENCE_OPS", "1")
    ref = _stepped(m32, r32, batch)
    _stepped(c16, r16, batch)
    monkeypatch.delenv("DLLM_REFERENCE_OPS")
    assert not any(n.startswith("pref") for n in calls), calls
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(pref="fused"))
    del calls[:]
    out = _stepped(m16, r16, batch)
    assert all(k in calls for k in ("pref_fwd", "pref_pairs", "pref_bwd")), calls
    assert out.logits is None and not any(p.grad is not None for p in r16.parameters())
    F = L.Figures(f"model {name}")
    F.add("loss", abs(out.loss.item() - ref.loss.item()), 0.01 * abs(ref.loss.item()))
    floor = {n: (rel, cos) for rel, cos, n in _grad_report(c16, m32)}
    rep = _grad_report(m16, m32)
    assert len(rep) >= len(list(m32.parameters())) - 1
    for rel, cos, n in rep:
        frel, fcos = floor[n]
        F.add(f"grad {n} rel", rel, max(3e-2, 1.5 * frel), quiet=True)
        F.add(f"grad {n} 1-cos", 1 - cos, max(1e-3, 1.5 * (1 - fcos)), quiet=True)
    print(f"[fig] model {name}: worst grad rel {max(r[0] for r in rep):.3e}, "
          f"worst 1-cos {max(1 - r[1] for r in rep):.3e}")
    F.done()


@pytest.fixture
def _no_leaked_step_seeds():
    from distributed_llms_example_amd.ops import rng as rng_mod
    yield
    st = rng_mod._active_step[0]
    if st is not None:
        st.disable()
    rng_mod.default_rng().site_mode = False


def test_graphed_step_with_reference_equals_eager(_no_leaked_step_seeds):
    """Preference steps captured as a HIP graph (the reference's forward inside) replay and equal the same steps run
    eagerly: the method and bounds of tests/test_distill_gpu.py::test_graphed_step_with_teacher_equals_eager."""
    from distributed_llms_example_amd.models import build_model, resolve_config
    from distributed_llms_example_amd.ops.rng import manual_seed
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    from distributed_llms_example_amd.train.graph import GraphedStep
    env = init_distributed()
    cfg = resolve_config("t5-base").replace(num_layers=2, num_decoder_layers=2, vocab_size=4096)
    torch.manual_seed(0)
    reference = build_model(cfg)
    policy = copy.deepcopy(reference)
    with torch.no_grad():
        for p in policy.parameters():
            p.add_(0.02 * torch.randn_like(p))
    g = torch.Generator().manual_seed(3)
    steps = 2
    data = [{"input_ids": torch.randint(3, cfg.vocab_size, (4, 256), generator=g).cuda(),
             "attention_mask": torch.ones(4, 256, dtype=torch.long).cuda(),
             "labels": torch.randint(3, cfg.vocab_size, (8, 64), generator=g).cuda()} for _ in range(steps + 2)]

    def engine():
        manual_seed(11)
        eng = TrainEngine(copy.deepcopy(policy), env, lr=1e-3, dtype=BF16, bucket_mb=8.0,
                          reference=copy.deepcopy(reference), dpo_beta=0.5, dpo_sft_alpha=0.25)
        eng.train()
        return eng

    eng_g = engine()
    gs = GraphedStep(eng_g, data[:1], warmup=2)
    losses_g = [float(gs.replay(data[2 + i:3 + i])) for i in range(steps)]
    pg = eng_g.flat.to_canonical(eng_g.flat.param_buf).float().clone()
    eng_g.disable_step_seeds()

    eng_e = engine()
    eng_e.enable_step_seeds()
    t = torch.zeros((), dtype=torch.float32, device="cuda")
    losses_e = []
    for i in range(steps + 2):
        loss = float(eng_e.forward_backward(data[0] if i < 2 else data[i]))
        t.add_(1.0)
        eng_e.step(hyper=eng_e.optimizer.device_hyper(t, eng_e.optimizer.param_groups[0]["lr"]))
        if i >= 2:
            losses_e.append(loss)
    pe = eng_e.flat.to_canonical(eng_e.flat.param_buf).float().clone()
    eng_e.disable_step_seeds()
    assert eng_e.last_pref_stats is not None and all(math.isfinite(float(v)) for v in eng_e.last_pref_stats.values())
    assert losses_g == pytest.approx(losses_e, rel=1e-3), (losses_g, losses_e)
    assert ((pg - pe).norm() / pe.norm()).item() < 1e-3
