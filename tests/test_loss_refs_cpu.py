"""The fp64 oracle of the loss-path kernel tests (tests/loss_refs.py), validated without a GPU.

* the references against ``F.cross_entropy`` (label smoothing, ignore_index) and autograd, both in float64, at 1e-12;
* the project's ``comp`` rule for every fp32-level bound the GPU tests apply: the fp32 torch composite of the same
  operation, on inputs from every generator the GPU tests use, sits at or under a QUARTER of the bound (a composite that
  did not fit there would make the kernel bound say nothing);
* the chunk-state merge {max, sum exp, sum x, x_label} over ``_chunks(V, vc)``, emulated in fp64, equals ``ce_ref``:
  the algorithm and the chunk table, apart from the kernel;
* a property test of ``_chunks`` / ``_chunk_cols`` (pure Python) over every V in 1..2100 and three real vocabularies;
* the exactness headroom of the embedding-backward operands;
* the distillation references: ``kd_ref`` against torch's losses and autograd in float64, its ``-inf`` contract against
  hand-computed values at V = 3, ``kd_chunk_merge_ref`` equal to it on both hand-made chunk tables (the ``-inf``
  patterns included), and the comp rule for ``kd_loss_abs_term`` / ``kd_abs_term`` on exactly the inputs of
  tests/test_kd_kernels_gpu.py (``loss_refs.kd_case`` draws them on the CPU for both).
"""
import pytest
import torch
import torch.nn.functional as F

import gemm_refs as G
import loss_refs as L
from distributed_llms_example_amd.ops import lm_head as LM
from distributed_llms_example_amd.ops import routing

CPU = "cpu"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
TIGHT = 1e-12
QUARTER = 0.25


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(got, ref):
    return ((got.double() - ref.double()).abs() / ref.double().abs().clamp_min(1.0)).max().item()


def _torch_labels(labels, V):
    """Labels as F.cross_entropy takes them: what the kernels treat as invalid (negative, >= V) becomes ignore_index."""
    return torch.where(L.valid_rows(labels, L.IGNORE, V), labels, torch.full_like(labels, L.IGNORE))


# --------------------------------------------------------------------------------- references against torch in float64
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("N,V", [(1, 7), (5, 1001), (37, 1003), (12, 2056)])
def test_ce_ref_matches_torch_float64(N, V, eps, bias):
    gen = _gen(N * 31 + V)
    x = L.peaked_logits(N, V, CPU, gen).double().requires_grad_(True)
    b = torch.randn(V, generator=gen).double() if bias else None
    labels = L.edge_labels(N, V, CPU, gen)
    g = 0.37
    loss, lse, d = L.ce_ref(x.detach(), labels, b, eps, L.IGNORE, V, g)
    xb = x + b if bias else x
    tl = F.cross_entropy(xb, _torch_labels(labels, V), reduction="none", label_smoothing=eps, ignore_index=L.IGNORE)
    (g * tl.sum()).backward()
    assert _close(loss, tl.detach()) < TIGHT
    assert _close(lse, torch.logsumexp(xb.detach(), 1)) < TIGHT
    assert _close(d, x.grad) < TIGHT
    invalid = ~L.valid_rows(labels, L.IGNORE, V)
    assert not loss[invalid].any() and not d[invalid].any()
    assert bool(torch.isfinite(lse).all())
    # the gradient of a row sums to g (1 - eps V / V - (1 - eps)) = 0
    assert d.sum(1).abs().max().item() < TIGHT


def test_ce_ref_banned_token_is_finite_without_smoothing():
    """eps = 0 and a -inf bias entry on a column that is no row's label: finite loss (as F.cross_entropy), gradient 0
    at that column."""
    N, V = 9, 1003
    gen = _gen(3)
    x = L.peaked_logits(N, V, CPU, gen).double()
    labels = L.edge_labels(N, V, CPU, gen)
    b = torch.zeros(V, dtype=F64)
    b[17] = float("-inf")
    assert not (labels == 17).any()
    loss, lse, d = L.ce_ref(x, labels, b, 0.0, L.IGNORE, V)
    tl = F.cross_entropy(x + b, _torch_labels(labels, V), reduction="none", ignore_index=L.IGNORE)
    assert bool(torch.isfinite(loss).all()) and _close(loss, tl) < TIGHT
    assert not d[:, 17].any() and bool(torch.isfinite(d).all())
    loss2, lse2 = L.chunk_merge_ref(x, labels, b, 0.0, L.IGNORE, V, LM._chunks(V, 256))
    assert _close(loss2, loss) < TIGHT and _close(lse2, lse) < TIGHT


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_lm_head_ref_matches_autograd_float64(eps, bias):
    N, d, V = 21, 64, 1003
    gen = _gen(11)
    h, w = L.lm_operands(N, d, V, CPU, gen)
    b = L.dyadic_bias(V, CPU, gen) if bias else None
    labels = L.edge_labels(N, V, CPU, gen)
    g = 1.0 / 13
    loss, lse, dl, dh, dw = L.lm_head_ref(h, w, labels, b, eps, L.IGNORE, g)
    h64, w64 = h.double().requires_grad_(True), w.double().requires_grad_(True)
    x = h64 @ w64.t()
    if bias:
        x = x + b.double()
    tl = F.cross_entropy(x, _torch_labels(labels, V), reduction="none", label_smoothing=eps, ignore_index=L.IGNORE)
    (g * tl.sum()).backward()
    assert _close(loss, tl.detach()) < TIGHT
    assert _close(dh, h64.grad) < TIGHT and _close(dw, w64.grad) < TIGHT
    assert G.exact_headroom(h, w, extra=None if b is None else b.view(1, V).expand(N, V)) < G.EXACT_LIMIT


def test_embed_ref_matches_index_add_and_headroom():
    V, d, T = 50, 8, 4099
    gen = _gen(5)
    dy, out0 = L.embed_operands(T, d, V, CPU, gen)
    ids = torch.randint(-1, V + 1, (T,), generator=gen)  # -1 and V: dropped
    pad = 3
    ref = L.embed_bwd_ref(ids, dy, V, pad, out0)
    keep = (ids >= 0) & (ids < V) & (ids != pad)
    exp = out0.double().index_add(0, ids[keep], dy.double()[keep])
    assert torch.equal(ref, exp) and torch.equal(ref[pad], out0[pad].double())
    # one id for all T rows: the largest per-id sum any GPU case forms
    one = torch.full((T,), 7)
    assert L.embed_headroom(one, dy, out0, V) < G.EXACT_LIMIT
    assert 8.0 * (4.0 * 4099 + 4.0) < G.EXACT_LIMIT  # the analytic worst case for any draw of embed_operands
    r1 = L.embed_bwd_ref(one, dy, V, -1, out0)
    assert torch.equal(r1.float().double(), r1)  # exact in fp32


# ------------------------------------------------------------------------------------------------ the composite margin
def _composite(x32, labels, b32, eps, V, g):
    """The fp32 torch composite: logsumexp / F.cross_entropy for lse and loss; for the gradient the definition
    g (exp(x - lse) - eps / V - (1 - eps) [v == y]) evaluated in fp32 from the same fp32-rounded lse the backward
    kernels are given."""
    xb = x32 + b32 if b32 is not None else x32
    lse = torch.logsumexp(xb, 1)
    loss = F.cross_entropy(xb, _torch_labels(labels, V), reduction="none", label_smoothing=eps, ignore_index=L.IGNORE)
    return loss, lse, xb


def _check_margin(x, labels, b, eps, V, g=0.37):
    """x: the logits as a kernel reads them (bf16 values or exact fp32 accumulators), held in fp32."""
    assert x.dtype == F32
    loss_r, lse_r, d_r = L.ce_ref(x, labels, b, eps, L.IGNORE, V, g)
    loss, lse, xb = _composite(x, labels, b, eps, V, g)
    assert L.row_metric(lse, lse_r) <= QUARTER * L.LOSS_BOUND
    assert L.row_metric(loss, loss_r) <= QUARTER * L.LOSS_BOUND
    lse32 = lse_r.float().view(-1, 1)
    hit = torch.zeros_like(x).scatter_(1, labels.clamp(0, V - 1).view(-1, 1), 1.0 - eps)
    valid = L.valid_rows(labels, L.IGNORE, V).view(-1, 1)
    d = torch.tensor(g, dtype=F32) * (torch.exp(xb - lse32) - torch.tensor(eps / V, dtype=F32) - hit) * valid
    bound = L.grad_bound(d_r, L.ce_abs_term(x, labels, b, eps, L.IGNORE, V, g), F32)
    worst, where = L.grad_worst(d, d_r, bound)
    assert worst <= QUARTER, (worst, where)
    return worst


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("N,V", [(5, 7), (300, 1001), (300, 1003), (130, 2056), (37, 50265)])
def test_composite_margin_peaked_logits(N, V, dt, eps, bias):
    """peaked_logits + edge_labels (+ a randn or a dyadic bias): the inputs of the ce_fwd / ce_bwd / ce_chunk tests."""
    gen = _gen(V + N)
    x = L.peaked_logits(N, V, CPU, gen)
    if dt == "bf16":
        x = x.to(BF16).float()
    labels = L.edge_labels(N, V, CPU, gen)
    b = 0.5 * torch.randn(V, generator=gen) if bias else None
    _check_margin(x, labels, b, eps, V)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("N,d,V", [(1, 64, 120), (130, 64, 136), (257, 128, 264), (130, 128, 300), (257, 64, 1003),
                                   (33, 128, 33029)])
def test_composite_margin_lm_operands(N, d, V, eps, bias):
    """lm_operands (+ dyadic_bias): exact logits in fp32, the inputs of the CEF / CEB / lm_head_loss tests."""
    gen = _gen(V + d)
    h, w = L.lm_operands(N, d, V, CPU, gen)
    b = L.dyadic_bias(V, CPU, gen) if bias else None
    x64 = h.double() @ w.double().t()
    x = x64.float()
    assert torch.equal(x.double(), x64)
    labels = L.edge_labels(N, V, CPU, gen)
    _check_margin(x, labels, b, eps, V, g=1.0 / N)
    # the logits are peaked: the boosted columns carry a visible share of most rows' mass
    p = torch.softmax(x64 + (b.double() if bias else 0.0), 1)[:, L.peak_columns(V)].sum(1)
    assert p.median().item() > 0.05


# ------------------------------------------------------------------------------------- chunk-state merge on chunk tables
def _tables():
    return [(1003, LM._chunks(1003, 256)), (2056, LM._chunks(2056, 1024)), (2056, L.WIDE_TABLE), (1032, L.HAND_TABLE),
            (50265, LM._chunks(50265, 12544)), (100, LM._chunks(100, 96))]


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("ti", range(6))
def test_chunk_merge_equals_ce_ref(ti, eps, bias):
    V, chunks = _tables()[ti]
    _assert_table(V, chunks, grid=4)
    gen = _gen(V)
    N = 9
    x = L.peaked_logits(N, V, CPU, gen).to(BF16)
    labels = L.edge_labels(N, V, CPU, gen)
    b = 0.5 * torch.randn(V, generator=gen) if bias else None
    loss_r, lse_r, _ = L.ce_ref(x, labels, b, eps, L.IGNORE, V)
    loss, lse = L.chunk_merge_ref(x, labels, b, eps, L.IGNORE, V, chunks)
    assert _close(loss, loss_r) < TIGHT and _close(lse, lse_r) < TIGHT


def test_tables_have_the_shapes_the_gpu_tests_count_on():
    assert LM._chunks(1003, 256) == [(0, 256, 0), (256, 256, 0), (512, 256, 0), (763, 240, 5)]
    assert LM._chunks(2056, 1024) == [(0, 1024, 0), (1024, 1024, 0), (2048, 8, 0)]
    assert sorted(s for _, _, s in L.HAND_TABLE) == [0, 1, 1, 3, 4, 7]
    assert [n for _, n, _ in L.WIDE_TABLE] == [1028, 1028]


# ------------------------------------------------------------------------------------------ _chunks / _chunk_cols
def _assert_table(V, chunks, grid=8):
    cover = torch.zeros(V, dtype=torch.int32)
    for c0, n, skip in chunks:
        assert c0 >= 0 and n > 0 and c0 + n <= V and 0 <= skip < n, (V, chunks)
        if V >= 8:
            assert n % grid == 0, (V, chunks)
        cover[c0 + skip:c0 + n] += 1
    assert bool((cover == 1).all()), (V, chunks)


def test_chunk_tables_cover_every_column_once(monkeypatch):
    """Every V in 1..2100 and T5's, BART's and M2M100's vocabularies, with every chunk width ``_chunk_cols`` returns
    for N in {1, 64, 1000, 65536} at ``lmhead_chunk_mb`` in {default, 8, the smallest that still gives 256 columns}:
    every column covered exactly once after ``skip``, chunks inside [0, V), 0 <= skip < n, widths on the 8-grid of the
    kernels' 16-B rows, and a ragged vocabulary (V % 8 != 0) never in a single chunk.  V < 8 has no 8-wide chunk to
    re-cover with: it stays one chunk of V columns (the chunk kernels' bindings reject a width off the 4-grid)."""
    Vs = list(range(1, 2101)) + [32128, 50265, 128112]
    widths = {V: set() for V in Vs}
    for N in (1, 64, 1000, 65536):
        for mb in (None, 8.0, 512.0 * N / 2 ** 20):
            if mb is None:
                monkeypatch.delenv("DLLM_ROUTE", raising=False)
                assert routing.get("lmhead_chunk_mb") == routing.DEFAULTS["lmhead_chunk_mb"]
            else:
                monkeypatch.setenv("DLLM_ROUTE", f"lmhead_chunk_mb={mb!r}")
                assert routing.get("lmhead_chunk_mb") == mb
            if mb is not None and mb < 8.0:
                assert LM._chunk_cols(N, 128112) == 256  # the smallest budget that still gives 256 columns
            for V in Vs:
                widths[V].add(LM._chunk_cols(N, V))
    for V in Vs:
        for vc in sorted(widths[V]):
            assert vc > 0 and vc % 8 == 0, (V, vc)
            chunks = LM._chunks(V, vc)
            _assert_table(V, chunks)
            if V < 8:
                assert chunks == [(0, V, 0)], (V, vc, chunks)
                continue
            assert all(n % 8 == 0 for _, n, _ in chunks), (V, vc, chunks)
            if V % 8:
                assert len(chunks) >= 2, (V, vc, chunks)
                assert chunks[-1][2] == 8 - V % 8 and all(s == 0 for _, _, s in chunks[:-1]), (V, vc, chunks)
            else:
                assert all(s == 0 for _, _, s in chunks), (V, vc, chunks)


# ------------------------------------------------------------------------------------------------- distillation (kd)
NINF = float("-inf")


@pytest.mark.parametrize("bias", ["none", "student", "both"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("T", L.KD_TEMPS)
@pytest.mark.parametrize("N,V", [(1, 7), (5, 1001), (37, 1003), (12, 2056)])
def test_kd_ref_matches_autograd_float64(N, V, T, eps, bias):
    """``kd_ref`` against torch's own losses and autograd in fp64: ds is the gradient of w_ce sum ce + w_kl T^2 sum kl
    over the valid rows."""
    case = L.kd_case(N, V, F32)
    bs, bt = L.kd_biases(case, bias)
    labels = case["labels"]
    ce, kl, stats, ds = L.kd_ref(case["s"], case["t"], labels, bs, bt, eps, L.IGNORE, V, T, L.W_CE, L.W_KL)
    s64 = case["s"].double().requires_grad_(True)
    sb = s64 + bs.double() if bs is not None else s64
    tb = case["t"].double() + (bt.double() if bt is not None else 0.0)
    valid = L.valid_rows(labels, L.IGNORE, V)
    ce_t = F.cross_entropy(sb, _torch_labels(labels, V), reduction="none", label_smoothing=eps, ignore_index=L.IGNORE)
    kl_t = F.kl_div(F.log_softmax(sb / T, -1), F.log_softmax(tb / T, -1), reduction="none", log_target=True).sum(-1)
    kl_t = kl_t * valid
    (L.W_CE * ce_t.sum() + L.W_KL * T * T * kl_t.sum()).backward()
    assert _close(ce, ce_t.detach()) < TIGHT and _close(kl, kl_t.detach()) < TIGHT
    assert _close(ds, s64.grad) < TIGHT
    for j, x in enumerate((sb, sb / T, tb / T)):
        assert _close(stats[:, j], torch.logsumexp(x.detach(), 1)) < TIGHT
    assert not ce[~valid].any() and not kl[~valid].any() and not ds[~valid].any()
    assert bool(torch.isfinite(stats).all()) and bool((kl >= -TIGHT).all())
    assert ds.sum(1).abs().max().item() < TIGHT  # both parts of a row's gradient sum to 0


def test_kd_ref_inf_contract_by_hand():
    """V = 3, T = 2, label 0, eps = 0, values chosen so that every softmax is a ratio of small integers."""
    ln = lambda v: torch.log(torch.tensor(float(v), dtype=F64)).item()  # noqa: E731
    lab = torch.tensor([0])
    t = torch.tensor([[2 * ln(3), 0.0, NINF]], dtype=F64)  # p = (3/4, 1/4, 0)
    # both models ban column 2: q = (1/2, 1/2, 0)
    s = torch.tensor([[0.0, 0.0, NINF]], dtype=F64)
    ce, kl, stats, ds = L.kd_ref(s, t, lab, None, None, 0.0, L.IGNORE, 3, 2.0, 0.5, 0.25)
    assert abs(kl.item() - (0.75 * ln(1.5) + 0.25 * ln(0.5))) < TIGHT
    assert abs(ce.item() - ln(2)) < TIGHT
    assert _close(stats, torch.tensor([[ln(2), ln(2), ln(4)]], dtype=F64)) < TIGHT
    want = 0.5 * torch.tensor([[-0.5, 0.5, 0.0]], dtype=F64) \
        + 0.25 * 2.0 * torch.tensor([[-0.25, 0.25, 0.0]], dtype=F64)
    assert _close(ds, want) < TIGHT and ds[0, 2].item() == 0.0
    # the teacher alone bans it: q = (1/4, 1/4, 1/2); the column adds nothing
    s = torch.tensor([[0.0, 0.0, 2 * ln(2)]], dtype=F64)
    ce, kl, stats, ds = L.kd_ref(s, t, lab, None, None, 0.0, L.IGNORE, 3, 2.0, 0.5, 0.25)
    assert abs(kl.item() - 0.75 * ln(3)) < TIGHT
    sm = torch.softmax(s, 1)
    want = 0.5 * (sm - torch.tensor([[1.0, 0.0, 0.0]], dtype=F64)) \
        + 0.25 * 2.0 * torch.tensor([[-0.5, 0.0, 0.5]], dtype=F64)
    assert _close(ds, want) < TIGHT
    # the same -inf delivered by the biases instead
    b = torch.tensor([0.0, 0.0, NINF], dtype=F64)
    out = L.kd_ref(s, torch.tensor([[2 * ln(3), 0.0, 5.0]], dtype=F64), lab, None, b, 0.0, L.IGNORE, 3, 2.0, 0.5, 0.25)
    assert abs(out[1].item() - 0.75 * ln(3)) < TIGHT and _close(out[3], want) < TIGHT
    # the student alone bans it, the teacher gives it mass: p = (3/5, 1/5, 1/5); kl = +inf, everything else finite
    t = torch.tensor([[2 * ln(3), 0.0, 0.0]], dtype=F64)
    s = torch.tensor([[0.0, 0.0, NINF]], dtype=F64)
    ce, kl, stats, ds = L.kd_ref(s, t, lab, None, None, 0.0, L.IGNORE, 3, 2.0, 0.5, 0.25)
    assert kl.item() == float("inf") and abs(ce.item() - ln(2)) < TIGHT
    assert _close(stats, torch.tensor([[ln(2), ln(2), ln(5)]], dtype=F64)) < TIGHT
    want = 0.5 * torch.tensor([[-0.5, 0.5, 0.0]], dtype=F64) \
        + 0.25 * 2.0 * torch.tensor([[0.5 - 0.6, 0.5 - 0.2, -0.2]], dtype=F64)
    assert _close(ds, want) < TIGHT
    # an invalid row stays 0 with -inf present
    ce, kl, stats, ds = L.kd_ref(s, t, torch.tensor([3]), None, None, 0.0, L.IGNORE, 3, 2.0)
    assert ce.item() == 0.0 and kl.item() == 0.0 and not ds.any() and bool(torch.isfinite(stats).all())
    # the chunk algorithm on the same rows: one column per chunk
    for sv, tv, klv in ((torch.tensor([[0.0, 0.0, NINF]], dtype=F64), torch.tensor([[2 * ln(3), 0.0, NINF]], dtype=F64),
                         0.75 * ln(1.5) + 0.25 * ln(0.5)), (s, t, float("inf"))):
        ce2, kl2, stats2, _ = L.kd_chunk_merge_ref(sv, tv, lab, None, None, 0.0, L.IGNORE, 3, 2.0,
                                                   [(0, 1, 0), (1, 1, 0), (2, 1, 0)])
        assert kl2.item() == klv or abs(kl2.item() - klv) < TIGHT
        assert abs(ce2.item() - ln(2)) < TIGHT and bool(torch.isfinite(stats2).all())


@pytest.mark.parametrize("bias", ["none", "both"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("T", L.KD_TEMPS)
@pytest.mark.parametrize("ti", [0, 1])
def test_kd_chunk_merge_equals_kd_ref(ti, T, eps, bias):
    V, chunks = [(1032, L.HAND_TABLE), (2056, L.WIDE_TABLE)][ti]
    _assert_table(V, chunks, grid=4)
    case = L.kd_case(9, V, BF16)
    bs, bt = L.kd_biases(case, bias)
    args = (case["s"], case["t"], case["labels"], bs, bt, eps, L.IGNORE, V, T)
    ce_r, kl_r, stats_r, _ = L.kd_ref(*args)
    ce, kl, stats, state = L.kd_chunk_merge_ref(*args, chunks)
    assert _close(ce, ce_r) < TIGHT and _close(kl, kl_r) < 1e-10 and _close(stats, stats_r) < TIGHT
    # the state after the last chunk is consistent with stats
    assert _close(state[:, 0] + torch.log(state[:, 1]), stats_r[:, 0]) < TIGHT
    assert _close(state[:, 0] / T + torch.log(state[:, 4]), stats_r[:, 1]) < TIGHT
    assert _close(state[:, 5] / T + torch.log(state[:, 6]), stats_r[:, 2]) < TIGHT
    if eps == 0.0:  # the -inf patterns: teacher only, both, student only
        ban = L.kd_banned_columns(V, chunks)
        for who in ("teacher", "both", "student"):
            b_s, b_t, lab = L.kd_ban(case, bs, bt, ban, who, V)
            args = (case["s"], case["t"], lab, b_s, b_t, 0.0, L.IGNORE, V, T)
            ce_r, kl_r, stats_r, _ = L.kd_ref(*args)
            ce, kl, stats, _ = L.kd_chunk_merge_ref(*args, chunks)
            valid = L.valid_rows(lab, L.IGNORE, V)
            assert bool(torch.isfinite(ce_r).all()) and bool(torch.isfinite(stats_r).all())
            assert bool((kl_r[valid] == float("inf")).all()) == (who == "student")
            assert _close(ce, ce_r) < TIGHT and _close(stats, stats_r) < TIGHT
            assert torch.equal(torch.isinf(kl), torch.isinf(kl_r))
            fin = torch.isfinite(kl_r)
            assert _close(kl[fin], kl_r[fin]) < 1e-10


def _kd_fp32(s, t, labels, bs, bt, eps, V, T, stats_r, w_ce, w_kl):
    """The fp32 torch composite of the distillation loss per row (the expressions of ops/distill.py ``_reference``), a
    plain fp32 evaluation of the cancelling form the kernels use, the three lse, and the gradient from the
    fp32-rounded reference stats as the backward kernels get them."""
    sb = s.float() + bs if bs is not None else s.float()
    tb = t.float() + bt if bt is not None else t.float()
    ce = F.cross_entropy(sb, _torch_labels(labels, V), reduction="none", label_smoothing=eps, ignore_index=L.IGNORE)
    logp, logq = F.log_softmax(tb / T, -1), F.log_softmax(sb / T, -1)
    p = logp.exp()
    valid = L.valid_rows(labels, L.IGNORE, V)
    kl = (p * torch.where(p > 0, logp - logq, torch.zeros_like(logp))).sum(-1) * valid
    stats = torch.stack([torch.logsumexp(sb, 1), torch.logsumexp(sb / T, 1), torch.logsumexp(tb / T, 1)], 1)
    klc = ((torch.softmax(tb / T, -1) * (tb - sb)).sum(-1) / T - stats[:, 2] + stats[:, 1]) * valid
    st = stats_r.float()
    hit = torch.zeros_like(sb).scatter_(1, labels.clamp(0, V - 1).view(-1, 1), 1.0 - eps)
    f = lambda v: torch.tensor(v, dtype=F32)  # noqa: E731
    d = f(w_ce) * (torch.exp(sb - st[:, 0:1]) - f(eps / V) - hit) \
        + f(w_kl * T) * (torch.exp(sb / T - st[:, 1:2]) - torch.exp(tb / T - st[:, 2:3]))
    return ce, kl, klc, stats, d * valid.view(-1, 1)


def _kd_margin(case, V, dtype, T, eps, bias, steps):
    bs, bt = L.kd_biases(case, bias)
    s, t, labels = case["s"], case["t"], case["labels"]
    ce_r, kl_r, stats_r, d_r = L.kd_ref(s, t, labels, bs, bt, eps, L.IGNORE, V, T, L.W_CE, L.W_KL)
    ce_term, kl_term = L.kd_loss_abs_term(s, t, labels, bs, bt, eps, L.IGNORE, V, T, steps)
    ce, kl, klc, stats, d = _kd_fp32(s, t, labels, bs, bt, eps, V, T, stats_r, L.W_CE, L.W_KL)
    bound = L.grad_bound(d_r, L.kd_abs_term(s, t, labels, bs, bt, eps, L.IGNORE, V, T, L.W_CE, L.W_KL), F32)
    figs = {"ce": L.abs_worst(ce, ce_r, ce_term), "kl composite": L.abs_worst(kl, kl_r, kl_term),
            "kl cancelling form": L.abs_worst(klc, kl_r, kl_term),
            "stats": L.row_metric(stats, stats_r) / L.LOSS_BOUND, "ds": L.grad_worst(d, d_r, bound)[0]}
    for name, val in figs.items():
        assert val <= QUARTER, (name, val, V, dtype, T, eps, bias)
    return figs


@pytest.mark.parametrize("bias", ["none", "student", "both"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("T", L.KD_TEMPS)
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("N,V", L.KD_SHAPES)
def test_kd_composite_margin(N, V, dt, T, eps, bias):
    """The comp rule on exactly the inputs of tests/test_kd_kernels_gpu.py::test_kd_fwd_bwd: the fp32 composite's ce and
    kl per row, a plain fp32 evaluation of the cancelling form, the three lse and the gradient all sit at or under a
    quarter of the bounds the GPU test applies."""
    dtype = BF16 if dt == "bf16" else F32
    figs = _kd_margin(L.kd_case(N, V, dtype), V, dtype, T, eps, bias, L.kd_steps(V, dtype))
    print(f"[fig] kd margin N={N} V={V} {dt} T={T} eps={eps} bias={bias}: " +
          ", ".join(f"{k} x{v:.3g}" for k, v in figs.items()))


@pytest.mark.parametrize("T", L.KD_TEMPS)
@pytest.mark.parametrize("ti", [0, 1])
def test_kd_composite_margin_chunk_tables(ti, T):
    """The same on the inputs of the direct chunk-kernel test (bf16, both tables, with the tables' step count)."""
    V, chunks = [(1032, L.HAND_TABLE), (2056, L.WIDE_TABLE)][ti]
    for N in L.KD_CHUNK_ROWS:
        case = L.kd_case(N, V, BF16, labels=lambda n, v, g: L.kd_chunk_labels(n, v, chunks, g))
        for eps in (0.0, 0.1):
            for bias in ("none", "both"):
                _kd_margin(case, V, BF16, T, eps, bias, L.kd_steps(V, BF16, chunks))
