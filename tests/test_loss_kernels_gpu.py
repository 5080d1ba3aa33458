"""The kernels that produce the training loss, one by one, on the GPU: ``ce_fwd`` / ``ce_bwd`` and ``ce_chunk_fwd`` /
``ce_chunk_bwd`` (csrc/ce.hip), the LM-head CE epilogues of csrc/gemm_w4.hip (``lmhead_ce_fwd`` = W4_EPI_CEF +
``ce_merge``, ``lmhead_ce_bwd_slice`` = W4_EPI_CEB) and ``lm_head_loss`` end to end on both routes.

Every kernel is compared with the fp64 reference of the same operation on the same rounded operands
(tests/loss_refs.py, validated on the CPU by tests/test_loss_refs_cpu.py): ``loss`` and ``lse`` per row, the gradients
per ELEMENT.  A whole-tensor norm does not see one wrong row of ``[V, d]`` or one dropped vocabulary column; these do.

Bounds.  loss, lse: |got - ref| / max(1, |ref|) <= rowwise_refs.ROW_BOUND[fp32] = 1e-5.  Gradient elements:
BF16_REL |ref| + abs_term for a bf16 store, abs_term alone for an fp32 store; abs_term is derived from the fp32 error
model in ``loss_refs.ce_abs_term``.  The fp32 torch composite sits at or under a quarter of each (CPU test).  The
backward kernels are given the reference's lse rounded to fp32, so that a forward error cannot mask a backward one.
Logits are peaked (boosted columns, labels on and off them): a near-uniform softmax hides dropped columns.  The LM-head
operands are dyadic (gemm_refs.dyadic): every logit is exact in the fp32 accumulator and only exp / log error remains.
Every figure is printed before a test asserts.
"""
import pytest
import torch

import gemm_refs as G
import loss_refs as L
import rowwise_refs as R
from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops import cross_entropy as CE
from distributed_llms_example_amd.ops import lm_head as LM
from distributed_llms_example_amd.ops import routing

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF16, "fp32": F32}
NAN = float("nan")
IGN = L.IGNORE
GS = 0.375  # the gradient scale g: exact in fp32
COMBOS = [(0.0, False), (0.0, True), (0.1, False), (0.1, True)]  # (eps, bias)


def _C():
    return _ext.native()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _scale():
    return torch.full((1,), GS, device=DEV, dtype=F32)


def _view(x, off):
    """``x`` [N, V] as a contiguous view ``off`` elements into a larger NaN buffer; (view, buffer)."""
    buf = torch.full((x.numel() + 16,), NAN, device=x.device, dtype=x.dtype)
    buf[off:off + x.numel()] = x.reshape(-1)
    return buf[off:off + x.numel()].view(x.shape), buf


def _guard(M, N, dtype, ld, off=0):
    """(buffer, [M, N] view with row stride ld, one guard row before and after) filled with NaN."""
    buf = torch.full(((M + 2) * ld,), NAN, device=DEV, dtype=dtype)
    return buf, buf.as_strided((M, N), (ld, 1), ld + off)


def _guard_intact(buf, view):
    """Every element of ``buf`` outside ``view`` still holds the sentinel's bit pattern."""
    it = torch.int16 if buf.dtype == BF16 else torch.int32
    c = buf.clone()
    c.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(NAN)
    return torch.equal(c.view(it), torch.full_like(buf, NAN).view(it))


def _rows(F, case, loss, lse, loss_r, lse_r, labels, V):
    F.fold("lse per row", L.row_metric(lse, lse_r), L.LOSS_BOUND, case)
    F.fold("loss per row", L.row_metric(loss, loss_r), L.LOSS_BOUND, case)
    inv = ~L.valid_rows(labels, IGN, V)
    F.check(f"[{case}] rows with an ignored / out-of-range label: loss exactly 0", not loss[inv].any())


def _grad(F, name, case, got, ref, abs_term, dtype, labels, V):
    worst, where = L.grad_worst(got, ref, L.grad_bound(ref, abs_term, dtype))
    F.fold(name, worst, 1.0, f"{case} {where['row']},{where['col']}")
    inv = ~L.valid_rows(labels, IGN, V)
    F.check(f"[{case}] {name}: rows with an ignored / out-of-range label exactly 0", not got[inv].any())


# ============================================================================================== ce_fwd / ce_bwd
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("V", [7, 1001, 1003, 2056, 50265])
def test_ce_fwd_bwd(V, dt):
    """V = 7: all scalar head; 1001 / 1003: every row at another 16-B phase; 2056: one full trip of 256 lanes x 8 plus a
    tail; 50265: BART's.  The logits sit one element into their buffer, so row 0 has a scalar head at every V.  Labels
    (loss_refs.edge_labels): column 0, column V - 1, inside the scalar head and tail, ignored, y = V, y = -1."""
    C, dtype = _C(), DT[dt]
    F = L.Figures(f"ce V={V} {dt}")
    for N in (1, 5, 300):
        gen = _gen(V * 1000 + N)
        x = L.peaked_logits(N, V, DEV, gen).to(dtype)
        labels = L.edge_labels(N, V, DEV, gen)
        bias_t = 0.5 * torch.randn(V, device=DEV, generator=gen)
        xv, _ = _view(x, 1)
        for eps, bias in COMBOS:
            case = f"N={N} eps={eps} bias={bias}"
            b = bias_t if bias else None
            loss_r, lse_r, d_r = L.ce_ref(x, labels, b, eps, IGN, V, GS)
            abs_term = L.ce_abs_term(x, labels, b, eps, IGN, V, GS)
            loss, lse = C.ce_fwd(xv, labels, b, eps, IGN)
            _rows(F, case, loss, lse, loss_r, lse_r, labels, V)
            lse32 = lse_r.float()
            src = xv if N == 5 else x  # N = 5: input and output at different 16-B phases (the scalar arm)
            out = C.ce_bwd(_scale(), src, labels, lse32, b, eps, IGN, False)
            _grad(F, "dlogits out of place", case, out, d_r, abs_term, dtype, labels, V)
            F.check(f"[{case}] out of place: the logits are untouched", torch.equal(xv, x))
            xi, ibuf = _view(x, 1)
            res = C.ce_bwd(_scale(), xi, labels, lse32, b, eps, IGN, True)
            F.check(f"[{case}] in place: same storage", res.data_ptr() == xi.data_ptr())
            _grad(F, "dlogits in place", case, xi, d_r, abs_term, dtype, labels, V)
            F.check(f"[{case}] in place: nothing written around the view",
                    bool(ibuf[:1].isnan().all()) and bool(ibuf[1 + N * V:].isnan().all()))
    F.done()


# ================================================================================= ce_chunk_fwd / ce_chunk_bwd, direct
def _tables():
    return {"1003x256": (1003, LM._chunks(1003, 256)), "2056x1024": (2056, LM._chunks(2056, 1024)),
            "hand": (1032, L.HAND_TABLE), "wide": (2056, L.WIDE_TABLE)}


def _chunk_labels(N, V, chunks, gen):
    """edge_labels, then per skipping chunk the last re-covered column (owned by the earlier chunk: the skipping one
    must not overwrite x_label), the first column it owns, and column V - 1."""
    labels = L.edge_labels(N, V, DEV, gen)
    special = [V - 1]
    for c0, n, skip in chunks:
        if skip:
            special += [c0 + skip - 1, c0 + skip, c0]
    if N == 1:
        labels[0] = special[1] if len(special) > 1 else V - 1
    else:
        assert N >= 9 + len(special)
        labels[9:9 + len(special)] = torch.tensor(special, device=DEV)
    return labels


def _run_chunks_fwd(C, x, chunks, labels, b, eps, V):
    """The chunks of ``x`` as [N, n] views with a row stride of n + 8 inside NaN buffers -> (loss, lse, views).  The
    skipped (re-covered) columns of a chunk hold NaN too: the earlier chunk owns them, label logit included, and
    nothing of the skipping chunk's copy may reach the state."""
    N = x.shape[0]
    state = torch.full((N, 4), NAN, device=DEV)
    loss, lse = torch.full((N,), NAN, device=DEV), torch.full((N,), NAN, device=DEV)
    views = []
    for j, (c0, n, skip) in enumerate(chunks):
        buf, v = _guard(N, n, BF16, n + 8)
        v.copy_(x[:, c0:c0 + n])
        v[:, :skip] = NAN
        C.ce_chunk_fwd(v, labels, b, state, loss, lse, c0, V, eps, IGN, j == 0, j + 1 == len(chunks), skip)
        views.append((buf, v))
    return loss, lse, views


@pytest.mark.parametrize("N", [1, 130])
@pytest.mark.parametrize("table", ["1003x256", "2056x1024", "hand", "wide"])
def test_ce_chunk_fwd_bwd(table, N):
    """1003x256: four chunks, the last re-covering 5 columns; hand: skip 1, 3, 4 and 7 (a partially and a wholly skipped
    4-group); wide: 1028 columns, the second trip of the 256 x 4 loop.  The chunks are strided views whose gaps hold
    NaN: the forward must not read them, the backward must not touch them; skipped columns come out exactly 0."""
    C = _C()
    V, chunks = _tables()[table]
    F = L.Figures(f"ce_chunk {table} N={N}")
    gen = _gen(V + N)
    x = L.peaked_logits(N, V, DEV, gen).to(BF16)
    labels = _chunk_labels(N, V, chunks, gen)
    bias_t = 0.5 * torch.randn(V, device=DEV, generator=gen)
    for eps, bias in COMBOS:
        case = f"eps={eps} bias={bias}"
        b = bias_t if bias else None
        loss_r, lse_r, d_r = L.ce_ref(x, labels, b, eps, IGN, V, GS)
        abs_term = L.ce_abs_term(x, labels, b, eps, IGN, V, GS)
        loss, lse, views = _run_chunks_fwd(C, x, chunks, labels, b, eps, V)
        _rows(F, case, loss, lse, loss_r, lse_r, labels, V)
        F.check(f"[{case}] forward: chunks and gaps untouched",
                all(_guard_intact(buf, v) and torch.equal(v[:, s:], x[:, c0 + s:c0 + n]) and bool(v[:, :s].isnan().all())
                    for (buf, v), (c0, n, s) in zip(views, chunks)))
        lse32 = lse_r.float()
        d = torch.full((N, V), NAN, device=DEV, dtype=BF16)
        seen = torch.zeros(V, device=DEV, dtype=torch.int32)
        for (buf, v), (c0, n, skip) in zip(views, chunks):
            C.ce_chunk_bwd(_scale(), v, labels, lse32, b, c0, V, eps, IGN, skip)
            F.check(f"[{case}] backward c0={c0}: gaps untouched", _guard_intact(buf, v))
            F.check(f"[{case}] backward c0={c0}: skipped columns exactly 0", not v[:, :skip].any())
            d[:, c0 + skip:c0 + n] = v[:, skip:]
            seen[c0 + skip:c0 + n] += 1
        assert bool((seen == 1).all())
        _grad(F, "dlogits in place, re-assembled", case, d, d_r, abs_term, BF16, labels, V)
    F.done()


# ========================================================================================== lmhead_ce_fwd (CEF + merge)
def _lm_case(N, d, V, seed, extra_labels=()):
    gen = _gen(seed)
    h, w = L.lm_operands(N, d, V, DEV, gen)
    bias_t = L.dyadic_bias(V, DEV, gen)
    labels = L.edge_labels(N, V, DEV, gen)
    extra = [c for c in extra_labels if c < V]
    if N == 1:
        labels[0] = min(V - 1, 127)
    else:
        assert N >= 9 + len(extra)
        labels[9:9 + len(extra)] = torch.tensor(extra, device=DEV, dtype=torch.long)
    x64 = h.double() @ w.double().t()
    assert 64.0 * (x64.abs().max().item() + bias_t.abs().max().item()) < G.EXACT_LIMIT  # exact in fp32, any order
    assert 64.0 * (d + 8) < G.EXACT_LIMIT  # ... and so is every partial sum, for any draw
    return h, w, bias_t, labels, x64


def _check_cef(F, C, case, h, w, labels, b, eps, x64):
    V = w.shape[0]
    loss_r, lse_r, _ = L.ce_ref(x64, labels, b, eps, IGN, V)
    loss, lse = C.lmhead_ce_fwd(h, w, labels, b, eps, IGN)
    _rows(F, case, loss, lse, loss_r, lse_r, labels, V)
    loss2, lse2 = C.lmhead_ce_fwd(h, w, labels, b, eps, IGN)
    F.check(f"[{case}] rerun bit-identical", torch.equal(loss, loss2) and torch.equal(lse, lse2))


@pytest.mark.parametrize("V", [120, 136, 264, 300, 1003])
@pytest.mark.parametrize("d", [64, 128])
def test_lmhead_ce_fwd(d, V):
    """V = 120: a single half tile, the second half wholly past V; 136: 8 columns in the second half; 264: 8 columns in
    the second column tile; 300: ceil(V / 128) odd (a half tile past V must not write the next row's slot); 1003.
    N = 130 crosses the 128-row wave half, N = 257 has one row in the second row tile.  Labels on the half-tile
    boundaries 127, 128, 255, 256."""
    C = _C()
    F = L.Figures(f"lmhead_ce_fwd d={d} V={V}")
    for N in (1, 130, 257):
        h, w, bias_t, labels, x64 = _lm_case(N, d, V, V * 7 + d + N, (127, 128, 255, 256))
        for eps, bias in COMBOS:
            _check_cef(F, C, f"N={N} eps={eps} bias={bias}", h, w, labels, bias_t if bias else None, eps, x64)
    F.done()


def test_lmhead_ce_fwd_persistent():
    """One workgroup per CU walking more than one tile: 2 ceil(V / 256) = CUs + 2 tiles at N = 257, d = 128, with 5
    columns in the last column tile (ceil(V / 128) odd)."""
    C = _C()
    cus = G.mirrored_cus(torch.cuda.get_device_properties(0).multi_processor_count)
    tn = (cus + 2) // 2
    N, d, V = 257, 128, 256 * (tn - 1) + 5
    assert 2 * -(-V // 256) == cus + 2 and G.w4_persistent(8, 2 * tn, d, True, cus)
    F = L.Figures(f"lmhead_ce_fwd persistent V={V}")
    h, w, bias_t, labels, x64 = _lm_case(N, d, V, 99, (127, 128, 255, 256, V - 6, V - 5))
    _check_cef(F, C, "eps=0.1 bias=True", h, w, labels, bias_t, 0.1, x64)
    F.done()


# ============================================================================================ lmhead_ce_bwd_slice (CEB)
@pytest.mark.parametrize("N", [1, 130, 257])
@pytest.mark.parametrize("d", [64, 128])
def test_lmhead_ce_bwd_slice(d, N):
    """The slices of ``_chunks(1003, 256)`` (the last re-covers 5 columns) and one of 520 columns at c0 = 8, whose tile
    columns 255 and 256 carry labels; a label inside the skipped columns of the tail slice; every label lies in another
    slice for most slices.  ``out`` is a strided view inside a NaN guard buffer."""
    C = _C()
    V = 1003
    chunks = LM._chunks(V, 256)
    assert chunks[-1] == (763, 240, 5)
    F = L.Figures(f"lmhead_ce_bwd_slice d={d} N={N}")
    h, w, bias_t, labels, x64 = _lm_case(N, d, V, 13 * d + N, (8 + 255, 8 + 256, 765, 767, 768, 127, 128, 255, 256))
    if N == 1:
        labels[0] = 765
    for eps, bias in COMBOS:
        b = bias_t if bias else None
        _, lse_r, d_r = L.ce_ref(x64, labels, b, eps, IGN, V, GS)
        abs_term = L.ce_abs_term(x64, labels, b, eps, IGN, V, GS)
        lse32 = lse_r.float()
        full = torch.full((N, V), NAN, device=DEV, dtype=BF16)
        for c0, n, skip in chunks + [(8, 520, 0)]:
            case = f"eps={eps} bias={bias} c0={c0}"
            buf, out = _guard(N, n, BF16, n + 8)
            C.lmhead_ce_bwd_slice(h, w[c0:c0 + n], labels, lse32, _scale(), b, out, c0, V, eps, IGN, skip)
            F.check(f"[{case}] guard rows and gaps intact", _guard_intact(buf, out))
            F.check(f"[{case}] skipped columns exactly 0", not out[:, :skip].any())
            ref = d_r[:, c0:c0 + n].clone()
            ref[:, :skip] = 0.0
            at = abs_term[:, c0:c0 + n].clone()
            at[:, :skip] = 5e-324
            _grad(F, "dlogits slice", case, out, ref, at, BF16, labels, V)
            if n != 520:
                full[:, c0 + skip:c0 + n] = out[:, skip:]
        # the softmax gradient sums to zero per row: over all slices the stored values' row sums stay within the sum
        # of their own bounds (a cheap check against a dropped or doubled column)
        rb = L.grad_bound(d_r, abs_term, BF16).sum(1)
        rs = full.double().sum(1).abs()
        F.fold("row sums over all slices / their bound", (rs / rb).max().item(), 1.0, f"eps={eps} bias={bias}")
    F.done()


# ======================================================================================= lm_head_loss, both routes
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


@pytest.mark.parametrize("eps,bias", [(0.0, False), (0.1, True)])
@pytest.mark.parametrize("route", ["fused", "logits"])
def test_lm_head_loss_rows_of_dw(route, eps, bias, monkeypatch):
    """V = 1003, N = 130 in 256-column chunks (four, the last ragged): the loss, dh per row and dW per row of [V, d]
    (one row per vocabulary column: a column that lost its target or was counted twice moves one row by O(1 / N))
    against fp64 of the same bf16 operands, on the GEMM-epilogue route and on the chunked-logits route."""
    N, d, V = 130, 128, 1003
    F = L.Figures(f"lm_head_loss route={route} eps={eps} bias={bias}")
    gen = _gen(41)
    h = torch.randn(N, d, device=DEV, generator=gen).to(BF16)
    w = (torch.randn(V, d, device=DEV, generator=gen) * d ** -0.5).to(BF16)
    b = None
    if bias:
        b = 0.5 * torch.randn(V, device=DEV, generator=gen)
        b[L.peak_columns(V)] += 4.0
    else:
        w[L.peak_columns(V)] *= 4.0
    labels = L.edge_labels(N, V, DEV, gen)
    labels[3], labels[5] = IGN, IGN  # lm_head_loss counts rows by label != ignore_index: out-of-range rows are its caller's
    labels[9:13] = torch.tensor([762, 763, 767, 768], device=DEV)
    count = int((labels != IGN).sum().item())
    loss_r, _, _, dh_r, dw_r = L.lm_head_ref(h, w, labels, b, eps, IGN, 1.0 / count)
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(lmhead_chunk_mb=0.07, lmhead=route))
    assert LM._chunk_cols(N, V) == 256
    chunks = LM._chunks(V, 256)
    assert len(chunks) == 4 and chunks[-1][2] == 5
    calls = []
    spy = _Spy(calls, _ext.native())
    monkeypatch.setattr(LM._ext, "native", lambda: spy)
    outs = []
    for _ in range(2):
        hg, wg = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
        loss = LM.lm_head_loss(hg, wg, labels, bias=b, label_smoothing=eps, ignore_index=IGN)
        loss.backward()
        outs.append((loss.detach(), hg.grad, wg.grad))
    if route == "fused":
        assert calls.count("lmhead_ce_fwd") == 2 and calls.count("lmhead_ce_bwd_slice") == 2 * len(chunks), calls
        assert "ce_chunk_fwd" not in calls and "ce_chunk_bwd" not in calls, calls
    else:
        assert calls.count("ce_chunk_fwd") == 2 * len(chunks) and calls.count("ce_chunk_bwd") == 2 * len(chunks), calls
        assert "lmhead_ce_fwd" not in calls and "lmhead_ce_bwd_slice" not in calls, calls
    loss, dh, dw = outs[0]
    ref = loss_r.sum().item() / count
    F.add("loss", abs(loss.item() - ref), 2e-3 * max(1.0, abs(ref)))
    F.add("dh per row", R.row_err(dh, dh_r), R.ROW_BOUND[BF16])
    F.add("dW per row of [V, d]", R.row_err(dw, dw_r), R.ROW_BOUND[BF16])
    F.check("rerun bit-identical", all(torch.equal(a, c) for a, c in zip(*outs)), quiet=False)
    F.done()


# ==================================================================================================== the -inf case
def test_banned_token_without_smoothing_is_finite_on_every_route():
    """eps = 0 and a bias with one -inf entry (a banned token, BART's final_logits_bias) on a column that is no row's
    label: ``F.cross_entropy`` gives a finite loss, and so must ``ce_fwd``, the chunked forward, the GEMM-epilogue
    forward and ``cross_entropy``; the gradient is exactly 0 at that column and finite everywhere.  (eps * sum(x) / V
    evaluated unconditionally is 0 * -inf = NaN: the smoothing term must be skipped, not multiplied by 0.)"""
    C = _C()
    N, d, V, ban = 37, 64, 1003, 17
    F = L.Figures("banned token eps=0")
    h, w, bias_t, labels, x64 = _lm_case(N, d, V, 5)
    b = bias_t.clone()
    b[ban] = float("-inf")
    labels[labels == ban] = ban + 1
    x = x64.to(BF16)  # the materialised-logits routes see bf16 logits
    chunks = LM._chunks(V, 256)
    loss_m, lse_m, d_m = L.ce_ref(x, labels, b, 0.0, IGN, V, GS)
    loss_f, lse_f, d_f = L.ce_ref(x64, labels, b, 0.0, IGN, V, GS)
    assert bool(torch.isfinite(loss_m).all()) and bool(torch.isfinite(loss_f).all())

    def grad_ok(name, got, ref, xs):
        F.check(f"{name}: gradient finite", bool(torch.isfinite(got).all()), quiet=False)
        F.check(f"{name}: gradient exactly 0 at the banned column", not got[:, ban].any(), quiet=False)
        _grad(F, f"{name} dlogits", name, got, ref, L.ce_abs_term(xs, labels, b, 0.0, IGN, V, GS), BF16, labels, V)

    # ce_fwd / ce_bwd
    loss, lse = C.ce_fwd(x, labels, b, 0.0, IGN)
    F.add("ce_fwd loss per row", L.row_metric(loss, loss_m), L.LOSS_BOUND)
    F.add("ce_fwd lse per row", L.row_metric(lse, lse_m), L.LOSS_BOUND)
    grad_ok("ce_bwd", C.ce_bwd(_scale(), x, labels, lse_m.float(), b, 0.0, IGN, False), d_m, x)
    # chunked
    loss, lse, views = _run_chunks_fwd(C, x, chunks, labels, b, 0.0, V)
    F.add("ce_chunk_fwd loss per row", L.row_metric(loss, loss_m), L.LOSS_BOUND)
    F.add("ce_chunk_fwd lse per row", L.row_metric(lse, lse_m), L.LOSS_BOUND)
    dch = torch.full((N, V), NAN, device=DEV, dtype=BF16)
    for (_, v), (c0, n, skip) in zip(views, chunks):
        C.ce_chunk_bwd(_scale(), v, labels, lse_m.float(), b, c0, V, 0.0, IGN, skip)
        dch[:, c0 + skip:c0 + n] = v[:, skip:]
    grad_ok("ce_chunk_bwd", dch, d_m, x)
    # GEMM epilogues
    loss, lse = C.lmhead_ce_fwd(h, w, labels, b, 0.0, IGN)
    F.add("lmhead_ce_fwd loss per row", L.row_metric(loss, loss_f), L.LOSS_BOUND)
    F.add("lmhead_ce_fwd lse per row", L.row_metric(lse, lse_f), L.LOSS_BOUND)
    dfu = torch.full((N, V), NAN, device=DEV, dtype=BF16)
    for c0, n, skip in chunks:
        out = torch.empty(N, n, device=DEV, dtype=BF16)
        C.lmhead_ce_bwd_slice(h, w[c0:c0 + n], labels, lse_f.float(), _scale(), b, out, c0, V, 0.0, IGN, skip)
        dfu[:, c0 + skip:c0 + n] = out[:, skip:]
    grad_ok("lmhead_ce_bwd_slice", dfu, d_f, x64)
    # ops.cross_entropy (mean over rows with label != ignore_index; out-of-range rows are its caller's to exclude)
    lab = torch.where(L.valid_rows(labels, IGN, V), labels, torch.full_like(labels, IGN))
    count = int((lab != IGN).sum().item())
    xg = x.clone().requires_grad_(True)
    mean = CE.cross_entropy(xg, lab, bias=b, label_smoothing=0.0, ignore_index=IGN)
    (mean * (GS * count)).backward()
    ref = loss_m.sum().item() / count
    val = abs(mean.item() - ref) / max(1.0, abs(ref))
    F.add("cross_entropy mean loss", val if val == val else float("inf"), L.LOSS_BOUND)
    grad_ok("cross_entropy", xg.grad, d_m, x)
    F.done()


# ========================================================================================================= bindings
def test_ce_chunk_bindings_reject_before_launch():
    """ce_chunk_fwd and ce_chunk_bwd raise, rather than launch, on operands the kernels cannot address."""
    C = _C()
    N, V, Vc = 8, 1003, 256
    lg = torch.zeros(N, Vc, device=DEV, dtype=BF16)
    labels = torch.zeros(N, dtype=torch.long, device=DEV)
    state, loss, lse = torch.zeros(N, 4, device=DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    bias = torch.zeros(V, device=DEV)
    sc = _scale()

    def fwd(lg=lg, labels=labels, bias=bias, lse=lse, skip=0):
        C.ce_chunk_fwd(lg, labels, bias, state, loss, lse, 0, V, 0.1, IGN, True, True, skip)

    def bwd(lg=lg, labels=labels, bias=bias, lse=lse, skip=0):
        C.ce_chunk_bwd(sc, lg, labels, lse, bias, 0, V, 0.1, IGN, skip)

    fwd()
    bwd()  # well-formed: both pass
    odd = torch.zeros(N * Vc + 4, device=DEV, dtype=BF16)[1:1 + N * Vc].view(N, Vc)
    assert odd.data_ptr() % 8 == 2 and odd.stride(0) % 4 == 0
    bad = [
        ("labels int32", dict(labels=labels.int())),
        ("labels strided", dict(labels=torch.zeros(2 * N, dtype=torch.long, device=DEV)[::2])),
        ("labels short", dict(labels=labels[:N - 1])),
        ("lse fp64", dict(lse=lse.double())),
        ("lse short", dict(lse=lse[:N - 1])),
        ("bias fp64", dict(bias=bias.double())),
        ("bias short", dict(bias=bias[:V - 1])),
        ("bias strided", dict(bias=torch.zeros(2 * V, device=DEV)[::2])),
        ("logits not 8-byte aligned", dict(lg=odd)),
        ("skip < 0", dict(skip=-1)),
        ("skip = Vc", dict(skip=Vc)),
    ]
    for fn in (fwd, bwd):
        for name, kw in bad:
            with pytest.raises(RuntimeError):
                fn(**kw)
                pytest.fail(f"{fn.__name__} accepted: {name}")
    with pytest.raises(RuntimeError, match="lse"):
        bwd(lse=torch.zeros(2 * N, device=DEV)[::2])
    with pytest.raises(RuntimeError, match="vocabulary"):
        C.ce_chunk_bwd(sc, lg, labels, lse, bias, V - 8, V, 0.1, IGN, 0)
    torch.cuda.synchronize()


def test_ce_bindings_reject_cpu_operands():
    """ce_fwd (labels, bias) and ce_chunk_fwd (labels, state, bias) hand these pointers to their kernels: a tensor
    that is not on the GPU must raise.  Zero-row inputs: the bindings check everything and return before launching, so
    a missing check shows as "did not raise" and never as a kernel reading a host pointer."""
    C = _C()
    V = 8
    labels, rows = torch.zeros(0, dtype=torch.long, device=DEV), torch.zeros(0, device=DEV)
    bias = torch.zeros(V, device=DEV)
    cases = [
        (C.ce_fwd, (torch.zeros(0, V, device=DEV), labels, bias, 0.1, IGN), (1, 2)),
        (C.ce_chunk_fwd, (torch.zeros(0, V, device=DEV, dtype=BF16), labels, bias, torch.zeros(0, 4, device=DEV), rows,
                          rows.clone(), 0, V, 0.1, IGN, True, True, 0), (1, 2, 3)),
    ]
    for call, args, slots in cases:
        call(*args)  # well-formed: passes
        for i in slots:
            bad = list(args)
            bad[i] = args[i].cpu()
            with pytest.raises(RuntimeError):
                call(*bad)
                pytest.fail(f"{call.__name__} accepted a CPU tensor as argument {i}")
    torch.cuda.synchronize()
