"""The distillation-loss kernels (csrc/kd.hip), one by one, on the GPU: ``kd_fwd`` / ``kd_bwd``, ``kd_chunk_fwd`` /
``kd_chunk_bwd`` called directly, and ``lm_head_distill_loss`` end to end.

Every kernel is compared with the fp64 reference of the same operation on the same rounded operands
(tests/loss_refs.py ``kd_ref``, validated on the CPU by tests/test_loss_refs_cpu.py): ``ce`` and ``kl`` per ROW, the
three ``stats`` columns per row, the gradient per ELEMENT.  A mean over rows does not see one wrong row or one dropped
16-B group; these do.

Bounds.  ``stats`` = {lse(s), lse(s/T), lse(t/T)}: |got - ref| / max(1, |ref|) <= LOSS_BOUND = 1e-5 per row.  ``ce`` and
``kl`` are differences of much larger terms, so their bounds are absolute, per row, from the fp32 error model of
``loss_refs.kd_loss_abs_term``.  Gradient elements: BF16_REL |ref| + abs_term for a bf16 store, abs_term alone for an
fp32 store, abs_term from ``loss_refs.kd_abs_term``.  The fp32 torch composite sits at or under a quarter of each, on
exactly these inputs (the CPU test draws them from the same ``loss_refs.kd_case``).  The backward kernels are given the
REFERENCE's stats rounded to fp32 and two different weights, so that a forward error cannot mask a backward one.
Logits are peaked with one row of both models scaled by 20; labels walk the edge cases (``edge_labels``).  -inf logits
follow the contract in tests/loss_refs.py.  Every figure is printed before a test asserts.
"""
import pytest
import torch

import loss_refs as L
import rowwise_refs as R
from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops import distill as D
from distributed_llms_example_amd.ops import routing

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF16, "fp32": F32}
NAN, INF = float("nan"), float("inf")
IGN = L.IGNORE
BIASES = ("none", "student", "both")


def _C():
    return _ext.native()


def _dev(case):
    return {k: v.to(DEV) for k, v in case.items()}


def _weights():
    return torch.full((1,), L.W_CE, device=DEV), torch.full((1,), L.W_KL, device=DEV)


def _view(x, off):
    """``x`` [N, V] as a contiguous view ``off`` elements into a larger NaN buffer; (view, buffer)."""
    buf = torch.full((x.numel() + 16,), NAN, device=x.device, dtype=x.dtype)
    buf[off:off + x.numel()] = x.reshape(-1)
    return buf[off:off + x.numel()].view(x.shape), buf


def _around_intact(buf, off, n):
    return bool(buf[:off].isnan().all()) and bool(buf[off + n:].isnan().all())


def _guard(M, N, ld):
    """(buffer, [M, N] bf16 view with row stride ld, one guard row before and after) filled with NaN."""
    buf = torch.full(((M + 2) * ld,), NAN, device=DEV, dtype=BF16)
    return buf, buf.as_strided((M, N), (ld, 1), ld)


def _guard_intact(buf, view):
    """Every element of ``buf`` outside ``view`` still holds the sentinel's bit pattern."""
    c = buf.clone()
    c.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(NAN)
    return torch.equal(c.view(torch.int16), torch.full_like(buf, NAN).view(torch.int16))


class _Ref:
    """The fp64 reference and the bounds of one (inputs, T, eps, biases) case."""

    def __init__(self, s, t, labels, bs, bt, eps, V, T, dtype, steps):
        self.labels, self.V, self.dtype = labels, V, dtype
        self.ce, self.kl, self.stats, self.ds = L.kd_ref(s, t, labels, bs, bt, eps, IGN, V, T, L.W_CE, L.W_KL)
        self.ce_term, self.kl_term = L.kd_loss_abs_term(s, t, labels, bs, bt, eps, IGN, V, T, steps)
        self.bound = L.grad_bound(self.ds, L.kd_abs_term(s, t, labels, bs, bt, eps, IGN, V, T, L.W_CE, L.W_KL), dtype)
        self.invalid = ~L.valid_rows(labels, IGN, V)
        self.stats32 = self.stats.float().contiguous()

    def forward(self, F, case, ce, kl, stats):
        for j, name in enumerate(("lse(s)", "lse(s/T)", "lse(t/T)")):
            F.fold(f"stats {name} per row", L.row_metric(stats[:, j], self.stats[:, j]), L.LOSS_BOUND, case)
        F.fold("ce per row / its bound", L.abs_worst(ce, self.ce, self.ce_term), 1.0, case)
        unb = torch.isinf(self.kl)  # rows whose kl is +inf by the contract: equality, not a distance
        if bool(unb.any()):
            F.check(f"[{case}] kl == +inf where the student bans a column with p_v > 0", bool((kl[unb] == INF).all()))
        if not bool(unb.all()):
            F.fold("kl per row / its bound", L.abs_worst(kl[~unb], self.kl[~unb], self.kl_term[~unb]), 1.0, case)
        F.check(f"[{case}] rows with an ignored / out-of-range label: ce and kl exactly 0",
                not ce[self.invalid].any() and not kl[self.invalid].any())

    def backward(self, F, name, case, got, cols=None):
        ref, bound = (self.ds, self.bound) if cols is None else (self.ds[:, cols], self.bound[:, cols])
        worst, where = L.grad_worst(got, ref, bound)
        F.fold(name, worst, 1.0, f"{case} {where['row']},{where['col']}")
        F.check(f"[{case}] {name}: rows with an ignored / out-of-range label exactly 0", not got[self.invalid].any())


def _fwd_bwd(F, C, case, s, t, labels, bs, bt, eps, T, dtype, steps):
    """kd_fwd, then kd_bwd out of place and in place with the reference's stats, on views at three 16-B phases."""
    N, V = s.shape
    ref = _Ref(s, t, labels, bs, bt, eps, V, T, dtype, steps)
    sv, sbuf = _view(s, 1)
    tv, tbuf = _view(t, 2)
    es = s.element_size()
    assert sv.data_ptr() % 16 == es and tv.data_ptr() % 16 == 2 * es
    ce, kl, stats = C.kd_fwd(sv, tv, labels, bs, bt, eps, IGN, T)
    ref.forward(F, case, ce, kl, stats)
    w_ce, w_kl = _weights()
    out = C.kd_bwd(w_ce, w_kl, sv, tv, labels, ref.stats32, bs, bt, eps, IGN, T, False)
    assert out.data_ptr() % 16 == 0  # student, teacher and output: three 16-B phases
    ref.backward(F, "ds out of place", case, out)
    res = C.kd_bwd(w_ce, w_kl, sv, tv, labels, ref.stats32, bs, bt, eps, IGN, T, True)
    F.check(f"[{case}] in place: same storage", res.data_ptr() == sv.data_ptr())
    ref.backward(F, "ds in place", case, sv)
    F.check(f"[{case}] the teacher and everything around both views untouched",
            torch.equal(tv, t) and _around_intact(sbuf, 1, N * V) and _around_intact(tbuf, 2, N * V))
    return ref, out


# ================================================================================================ kd_fwd / kd_bwd
@pytest.mark.parametrize("V,dt", [(V, dt) for V in (7, 1001, 1003, 2056) for dt in ("bf16", "fp32")]
                         + [(50265, "bf16")])
def test_kd_fwd_bwd(V, dt):
    """V = 7: all scalar head; 1001 / 1003: every row at another 16-B phase; 2056: one full trip of 256 lanes x 8 plus a
    tail; 50265 (N = 5, bf16 only): BART's, many trips.  N = 1, 5 and 300; T = 1 (the template arm), 2 and 0.7;
    eps 0 and 0.1; no bias, the student's, both.  Labels: column 0, V - 1, inside head and tail, ignored, y = V, -1."""
    C, dtype = _C(), DT[dt]
    F = L.Figures(f"kd V={V} {dt}")
    for N, _ in [nv for nv in L.KD_SHAPES if nv[1] == V]:
        c = _dev(L.kd_case(N, V, dtype))
        for T in L.KD_TEMPS:
            for eps in (0.0, 0.1):
                for bias in BIASES:
                    bs, bt = L.kd_biases(c, bias)
                    _fwd_bwd(F, C, f"N={N} T={T} eps={eps} bias={bias}", c["s"], c["t"], c["labels"], bs, bt, eps, T,
                             dtype, L.kd_steps(V, dtype))
    F.done()


# ======================================================================================================= -inf logits
@pytest.mark.parametrize("via", ["bias-bf16", "bias-fp32", "logits-fp32"])
@pytest.mark.parametrize("V", [7, 1003, 2056])
def test_kd_inf_contract(V, via):
    """-inf on column 0 (scalar head), on all of lane 0's first 16-B group (columns 0..15 cover it at every phase: that
    lane's running maxima are still -inf after a group), on the last column (tail) and on the middle peak; through the
    fp32 biases, and through fp32 logits themselves.  Teacher only and both models on the same columns: every such
    column has p_v = 0 and adds nothing, kl finite and within its bound.  Student only, eps = 0: ce finite, kl == +inf
    (the teacher gives every banned column a weight fp32 can hold).  stats finite, the gradient finite and within its
    bound.  Never -inf on a valid row's label."""
    C = _C()
    dtype = BF16 if via == "bias-bf16" else F32
    F = L.Figures(f"kd -inf V={V} {via}")
    N = 5
    c = _dev(L.kd_case(N, V, dtype, hot_scale=L.INF_HOT_SCALE))
    ban = L.kd_banned_columns(V)
    for who in ("teacher", "both", "student"):
        for base in ("none", "both"):
            b0s, b0t = L.kd_biases(c, base)
            bs, bt, labels = L.kd_ban(c, b0s, b0t, ban, who, V)
            labels = labels.to(DEV)
            s, t = c["s"], c["t"]
            if via == "logits-fp32":
                if base == "both":
                    continue
                s, t = s + bs, t + bt  # exact: the bias is 0 or -inf
                bs = bt = None
            assert not bool(torch.isin(labels[L.valid_rows(labels, IGN, V)], torch.tensor(ban, device=DEV)).any())
            for T in L.KD_TEMPS:
                for eps in ((0.0,) if who != "teacher" else (0.0, 0.1)):
                    case = f"{who} base={base} T={T} eps={eps}"
                    ref, out = _fwd_bwd(F, C, case, s, t, labels, bs, bt, eps, T, dtype, L.kd_steps(V, dtype))
                    valid = ~ref.invalid
                    assert bool(torch.isfinite(ref.stats).all()) and bool(torch.isfinite(ref.ce).all())
                    assert bool(torch.isinf(ref.kl[valid]).all()) == (who == "student")
                    if who == "student":  # unambiguous in fp32: the banned columns' teacher weight does not underflow
                        tb = t.double() if bt is None else t.double() + bt.double()
                        assert torch.softmax(tb / T, 1)[:, ban].max(1).values.min().item() > 1e-30
                    F.check(f"[{case}] gradient finite", bool(torch.isfinite(out).all()))
                    if who == "both" and eps == 0.0:
                        F.check(f"[{case}] gradient exactly 0 on the columns both models ban", not out[:, ban].any())
    F.done()


# ========================================================================= kd_chunk_fwd / kd_chunk_bwd, called directly
TABLES = {"hand": (1032, L.HAND_TABLE), "wide": (2056, L.WIDE_TABLE)}


def _run_chunks(F, C, case, s, t, labels, bs, bt, eps, T, V, chunks):
    """Forward over the chunk table, then backward with the reference's stats.  The chunks are [N, n] views with a row
    stride of n + 8 inside NaN buffers; the re-covered (skipped) columns of BOTH chunk buffers hold NaN, forward and
    backward: the earlier chunk owns them, nothing of the skipping chunk's copy may reach the state, and their
    gradient is 0 whatever they hold."""
    N = s.shape[0]
    ref = _Ref(s, t, labels, bs, bt, eps, V, T, BF16, L.kd_steps(V, BF16, chunks))
    state = torch.full((N, 8), NAN, device=DEV)
    ce, kl, stats = (torch.full(sh, NAN, device=DEV) for sh in ((N,), (N,), (N, 3)))
    views = []
    for j, (c0, n, skip) in enumerate(chunks):
        (sb, vs), (tb, vt) = _guard(N, n, n + 8), _guard(N, n, n + 8)
        vs.copy_(s[:, c0:c0 + n])
        vt.copy_(t[:, c0:c0 + n])
        vs[:, :skip] = NAN
        vt[:, :skip] = NAN
        C.kd_chunk_fwd(vs, vt, labels, bs, bt, state, ce, kl, stats, c0, V, eps, IGN, T, j == 0, j + 1 == len(chunks),
                       skip)
        views.append((sb, vs, tb, vt))
    ref.forward(F, case, ce, kl, stats)
    F.check(f"[{case}] forward: chunks and gaps untouched",
            all(_guard_intact(sb, vs) and _guard_intact(tb, vt) and torch.equal(vs[:, k:], s[:, c0 + k:c0 + n])
                and torch.equal(vt[:, k:], t[:, c0 + k:c0 + n]) and bool(vs[:, :k].isnan().all())
                for (sb, vs, tb, vt), (c0, n, k) in zip(views, chunks)))
    # the state after the last chunk is consistent with stats, and holds the label's logit exactly
    st = state.double()
    for j, (m, z, name) in enumerate(((0, 1, "lse(s)"), (0, 4, "lse(s/T)"), (5, 6, "lse(t/T)"))):
        Tj = 1.0 if j == 0 else T
        if j == 1 and T == 1.0:
            continue  # the T == 1 arm keeps no second student sum
        lse = st[:, m] / Tj + torch.log(st[:, z])
        F.fold(f"state -> {name}", L.row_metric(lse, ref.stats[:, j]), L.LOSS_BOUND, case)
    valid = ~ref.invalid
    sx = s.float() + bs if bs is not None else s.float()
    want = sx.gather(1, labels.clamp(0, V - 1).view(-1, 1)).view(-1)
    F.check(f"[{case}] state holds the label's logit", torch.equal(state[valid, 3], want[valid]))
    # backward, in place over the student chunks
    w_ce, w_kl = _weights()
    d = torch.full((N, V), NAN, device=DEV, dtype=BF16)
    seen = torch.zeros(V, device=DEV, dtype=torch.int32)
    for (sb, vs, tb, vt), (c0, n, skip) in zip(views, chunks):
        C.kd_chunk_bwd(w_ce, w_kl, vs, vt, labels, ref.stats32, bs, bt, c0, V, eps, IGN, T, skip)
        F.check(f"[{case}] backward c0={c0}: gaps and the teacher chunk untouched",
                _guard_intact(sb, vs) and _guard_intact(tb, vt) and torch.equal(vt[:, skip:], t[:, c0 + skip:c0 + n]))
        F.check(f"[{case}] backward c0={c0}: skipped columns exactly 0", not vs[:, :skip].any())
        d[:, c0 + skip:c0 + n] = vs[:, skip:]
        seen[c0 + skip:c0 + n] += 1
    assert bool((seen == 1).all())
    ref.backward(F, "ds in place, re-assembled", case, d)
    return ref, d


@pytest.mark.parametrize("N", L.KD_CHUNK_ROWS)
@pytest.mark.parametrize("table", ["hand", "wide"])
def test_kd_chunk_fwd_bwd(table, N):
    """hand (V = 1032): skip 1, 3, 4 and 7 (partially and wholly skipped 4-groups); wide (V = 2056): 1028 columns, the
    second trip of the 256 x 4 loop.  Labels in the first and last column of every chunk and on both sides of every
    skip boundary.  T = 1, 2, 0.7; eps 0 and 0.1; without and with both biases."""
    C = _C()
    V, chunks = TABLES[table]
    F = L.Figures(f"kd_chunk {table} N={N}")
    c = _dev(L.kd_case(N, V, BF16, labels=lambda n, v, g: L.kd_chunk_labels(n, v, chunks, g)))
    for T in L.KD_TEMPS:
        for eps in (0.0, 0.1):
            for bias in ("none", "both"):
                bs, bt = L.kd_biases(c, bias)
                _run_chunks(F, C, f"T={T} eps={eps} bias={bias}", c["s"], c["t"], c["labels"], bs, bt, eps, T, V,
                            chunks)
    F.done()


@pytest.mark.parametrize("table", ["hand", "wide"])
def test_kd_chunk_inf_contract(table):
    """The -inf patterns through the biases on the chunk kernels: the columns of ``test_kd_inf_contract`` plus the first
    owned column of every 4-group that straddles a skip boundary."""
    C = _C()
    V, chunks = TABLES[table]
    F = L.Figures(f"kd_chunk -inf {table}")
    N = 40
    c = _dev(L.kd_case(N, V, BF16, labels=lambda n, v, g: L.kd_chunk_labels(n, v, chunks, g),
                       hot_scale=L.INF_HOT_SCALE))
    ban = L.kd_banned_columns(V, chunks)
    assert table != "hand" or len(ban) > 18  # the straddling groups' columns are in
    for who in ("teacher", "both", "student"):
        bs, bt, labels = L.kd_ban(c, c["bs"], c["bt"], ban, who, V)
        labels = labels.to(DEV)
        for T in (1.0, 0.7):
            case = f"{who} T={T}"
            ref, d = _run_chunks(F, C, case, c["s"], c["t"], labels, bs, bt, 0.0, T, V, chunks)
            assert bool(torch.isfinite(ref.stats).all()) and bool(torch.isfinite(ref.ce).all())
            assert bool(torch.isinf(ref.kl[~ref.invalid]).all()) == (who == "student")
            if who == "student":
                tb = c["t"].double() + bt.double()
                assert torch.softmax(tb / T, 1)[:, ban].max(1).values.min().item() > 1e-30
            F.check(f"[{case}] gradient finite", bool(torch.isfinite(d).all()))
    F.done()


# ============================================================================================================ reruns
def test_kd_reruns_bit_identical_each_kernel():
    C = _C()
    V, chunks = TABLES["hand"]
    c = _dev(L.kd_case(40, V, BF16))
    s, t, labels, bs, bt = c["s"], c["t"], c["labels"], c["bs"], c["bt"]
    w_ce, w_kl = _weights()
    outs = []
    for _ in range(2):
        ce, kl, stats = C.kd_fwd(s, t, labels, bs, bt, 0.1, IGN, 0.7)
        ds = C.kd_bwd(w_ce, w_kl, s, t, labels, stats, bs, bt, 0.1, IGN, 0.7, False)
        state = torch.full((40, 8), NAN, device=DEV)
        ce2, kl2, stats2 = (torch.full(sh, NAN, device=DEV) for sh in ((40,), (40,), (40, 3)))
        grads = []
        for j, (c0, n, skip) in enumerate(chunks):
            vs, vt = s[:, c0:c0 + n].contiguous(), t[:, c0:c0 + n].contiguous()
            C.kd_chunk_fwd(vs, vt, labels, bs, bt, state, ce2, kl2, stats2, c0, V, 0.1, IGN, 0.7, j == 0,
                           j + 1 == len(chunks), skip)
        for c0, n, skip in chunks:
            vs, vt = s[:, c0:c0 + n].contiguous(), t[:, c0:c0 + n].contiguous()
            C.kd_chunk_bwd(w_ce, w_kl, vs, vt, labels, stats2, bs, bt, c0, V, 0.1, IGN, 0.7, skip)
            grads.append(vs)
        outs.append([ce, kl, stats, ds, state, ce2, kl2, stats2] + grads)
    F = L.Figures("kd reruns")
    names = ["kd_fwd ce", "kd_fwd kl", "kd_fwd stats", "kd_bwd", "kd_chunk_fwd state", "kd_chunk_fwd ce",
             "kd_chunk_fwd kl", "kd_chunk_fwd stats"] + [f"kd_chunk_bwd c0={c0}" for c0, _, _ in chunks]
    for name, a, b in zip(names, *outs):
        it = torch.int16 if a.dtype == BF16 else torch.int32
        F.check(f"{name}: rerun bit-identical", torch.equal(a.view(it), b.view(it)))
    F.done()


# ============================================================================================== lm_head_distill_loss
class _Spy:
    """The native module with every call's name and arguments recorded."""

    def __init__(self, calls, real):
        self.calls, self.real = calls, real

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not callable(fn):
            return fn

        def wrapped(*a, **k):
            self.calls.append((name, a))
            return fn(*a, **k)
        return wrapped


def test_lm_head_distill_loss_rows(monkeypatch):
    """Dyadic operands (``lm_operands``: every logit is exact in the fp32 accumulator, so the bf16 logits the chunk
    kernels read are known exactly) at a ragged V = 1003 in 256-column chunks (the last re-covers 5 columns): ce and kl
    per ROW, read from the chunk kernels' output buffers through a spy, and dW per row of [V, d], dh per row."""
    N, d_s, d_t, V, T, eps, alpha = 37, 64, 128, 1003, 2.0, 0.1, 0.5
    F = L.Figures("lm_head_distill_loss V=1003")
    gen = torch.Generator().manual_seed(77)
    h, w = L.lm_operands(N, d_s, V, "cpu", gen)
    th, tw = L.lm_operands(N, d_t, V, "cpu", gen, peaks=[2, V // 2, V - 3])
    bs, bt = L.dyadic_bias(V, "cpu", gen), L.dyadic_bias(V, "cpu", gen, boost=1.0)
    labels = L.edge_labels(N, V, "cpu", gen)
    labels[9:13] = torch.tensor([762, 763, 767, 768])  # both sides of the ragged chunk's skip boundary
    # the entry counts rows by label != ignore: out-of-range rows are its caller's to exclude
    labels = torch.where(L.valid_rows(labels, IGN, V), labels, torch.full_like(labels, IGN))
    h, w, th, tw, bs, bt, labels = (x.to(DEV) for x in (h, w, th, tw, bs, bt, labels))
    x_s, x_t = h.double() @ w.double().t(), th.double() @ tw.double().t()
    assert 64.0 * (max(x_s.abs().max().item(), x_t.abs().max().item()) + 16.0) < 2 ** 24  # exact accumulators
    s, t = x_s.float().to(BF16), x_t.float().to(BF16)  # the stored logits: one rounding of an exact value
    count = int((labels != IGN).sum().item())
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(lmhead_chunk_mb=0.02))
    calls = []
    spy = _Spy(calls, _ext.native())
    monkeypatch.setattr(D._ext, "native", lambda: spy)
    assert D._chunk_cols(N, V) == 256
    chunks = D._chunks(V, 256)
    assert chunks[-1] == (763, 240, 5)
    hg, wg = h.to(BF16).requires_grad_(True), w.to(BF16).requires_grad_(True)
    loss, ce, kl = D.lm_head_distill_loss(hg, wg, th.to(BF16), tw.to(BF16), labels, bias=bs, teacher_bias=bt,
                                          label_smoothing=eps, alpha=alpha, temperature=T)
    fwd = [a for n, a in calls if n == "kd_chunk_fwd"]
    assert len(fwd) == len(chunks)
    ce_rows, kl_rows, stats = (fwd[-1][i].clone() for i in (6, 7, 8))  # (.., state, ce, kl, stats, ..)
    loss.backward()
    assert sum(n == "kd_chunk_bwd" for n, _ in calls) == len(chunks)
    ce_r, kl_r, stats_r, ds_r = L.kd_ref(s, t, labels, bs, bt, eps, IGN, V, T, (1 - alpha) / count, alpha / count)
    ce_term, kl_term = L.kd_loss_abs_term(s, t, labels, bs, bt, eps, IGN, V, T, L.kd_steps(V, BF16, chunks))
    F.add("ce per row / its bound", L.abs_worst(ce_rows, ce_r, ce_term), 1.0)
    F.add("kl per row / its bound", L.abs_worst(kl_rows, kl_r, kl_term), 1.0)
    F.add("stats per row", L.row_metric(stats, stats_r), L.LOSS_BOUND)
    ref = (1 - alpha) * ce_r.sum().item() / count + alpha * T * T * kl_r.sum().item() / count
    F.add("loss", abs(loss.item() - ref), 2e-3 * max(1.0, abs(ref)))
    F.add("dh per row", R.row_err(hg.grad, ds_r @ w.double()), R.ROW_BOUND[BF16])
    F.add("dW per row of [V, d]", R.row_err(wg.grad, ds_r.t() @ h.double()), R.ROW_BOUND[BF16])
    F.done()
