"""The distillation-loss kernels (csrc/kd.hip) and everything above them, on the GPU.

``kd_fwd`` / ``kd_bwd`` against the fp64 composite of the definition (ops/distill.py ``_reference`` on the same rounded
inputs, gradient by autograd) at row lengths off the 16-B grid, with the student and the teacher rows at different 16-B
phases from each other and from the output; ``kd_chunk_*`` through ``lm_head_distill_loss`` with a ragged tail chunk;
bit-identical reruns; the bindings' argument checks; model level and one graphed step.

Bounds are the project's own for the cross-entropy kernels: every loss component within ``2e-3 max(1, |ref|)``, the
gradient per row within ``rowwise_refs.ROW_BOUND`` and per element on ``rowwise_refs.elem_err`` (a bf16 store's 2^-8
allowed on top) within ELEM_BOUND.  ELEM_BOUND = 1e-4: every term of the gradient is ``exp(x - lse)`` in fp32 with
|x|, |lse| up to ~100 on the rows scaled by 20, so the exponent carries half an ulp of 128 (3.8e-6) from each of lse
and the temperature product plus the fast exp / log's few ulp: ~2e-5 relative at most, against 1e-4; one misread 16-B
group is O(1) on this metric.  Every figure is printed before a test asserts (run with -s to collect them).
"""
import copy

import pytest
import torch

import rowwise_refs as R
from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops import distill as D
from distributed_llms_example_amd.ops import routing

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF16, "fp32": F32}
ELEM_BOUND = 1e-4
ALPHA = 0.5


class Figures:
    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def add(self, name, val, bound):
        line = f"[fig] {self.tag} {name}: err {val:.3e} bound {bound:.1e}"
        print(line)
        if not val < bound:
            self.bad.append(line)

    def check(self, name, ok):
        print(f"[fig] {self.tag} {name}: {'ok' if ok else 'FAILED'}")
        if not ok:
            self.bad.append(f"{self.tag} {name}")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _view(x, off):
    """``x`` [N, V] as a contiguous view ``off`` elements into a larger buffer; (view, buffer)."""
    buf = torch.zeros(x.numel() + 16, device=x.device, dtype=x.dtype)
    buf[off:off + x.numel()] = x.reshape(-1)
    return buf[off:off + x.numel()].view(x.shape), buf


def _inputs(N, V, dtype, seed, ignored=(2, 17, 36), hot=(1, 5)):
    gen = _gen(seed)
    s = 2.0 * torch.randn(N, V, device=DEV, generator=gen)
    t = 0.6 * s + 1.5 * torch.randn(N, V, device=DEV, generator=gen)
    for r in hot:  # two rows scaled by 20: the running maxima and the rescales matter
        s[r] *= 20.0
        t[r] *= 20.0
    labels = torch.randint(0, V, (N,), device=DEV, generator=gen)
    for r in ignored:
        labels[r] = -100
    bs = 0.5 * torch.randn(V, device=DEV, generator=gen)
    bt = 0.5 * torch.randn(V, device=DEV, generator=gen)
    return s.to(dtype), t.to(dtype), labels, bs, bt


def _ref64(s, t, labels, bs, bt, eps, T, alpha=ALPHA):
    s64 = s.double().requires_grad_(True)
    loss, ce, kl = D._reference(s64, t.double(), labels, None if bs is None else bs.double(),
                                None if bt is None else bt.double(), eps, -100, alpha, T)
    loss.backward()
    return loss.item(), ce.item(), kl.item(), s64.grad


def _check_kernels(F, s, t, labels, bs, bt, eps, T, dtype):
    """kd_fwd / kd_bwd on views at three different 16-B phases, out of place and in place, against fp64."""
    C = _ext.native()
    N, V = s.shape
    loss_r, ce_r, kl_r, g_r = _ref64(s, t, labels, bs, bt, eps, T)
    sv, sbuf = _view(s, 1)
    tv, _ = _view(t, 2)
    es = s.element_size()
    assert sv.is_contiguous() and sv.data_ptr() % 16 == es and tv.data_ptr() % 16 == 2 * es
    ce_rows, kl_rows, stats = C.kd_fwd(sv, tv, labels, bs, bt, eps, -100, T)
    rows = labels != -100
    count = rows.sum().float()
    ce, kl = (ce_rows.sum() / count).item(), (kl_rows.sum() / count).item()
    F.add("ce", abs(ce - ce_r), 2e-3 * max(1.0, abs(ce_r)))
    F.add("kl", abs(kl - kl_r), 2e-3 * max(1.0, abs(kl_r)))
    F.add("loss", abs((1 - ALPHA) * ce + ALPHA * T * T * kl - loss_r), 2e-3 * max(1.0, abs(loss_r)))
    F.check("ignored rows: zero loss terms", not ce_rows[~rows].any() and not kl_rows[~rows].any())
    F.check("stats finite", bool(torch.isfinite(stats).all()))
    w_ce, w_kl = ((1 - ALPHA) / count).reshape(1), (ALPHA / count).reshape(1)
    slack = 2.0 ** -8 if dtype == BF16 else 0.0
    out = C.kd_bwd(w_ce, w_kl, sv, tv, labels, stats, bs, bt, eps, -100, T, False)
    assert out.data_ptr() % 16 == 0  # student, teacher and output: three 16-B phases
    F.add("ds (out of place) per row", R.row_err(out[rows], g_r[rows]), R.ROW_BOUND[dtype])
    F.add("ds (out of place) per element", R.elem_err(out[rows], g_r[rows], slack), ELEM_BOUND)
    F.check("ignored rows: zero gradient", not out[~rows].any())
    F.check("out of place: the student is untouched", torch.equal(sv, s))
    before = sbuf.clone()
    res = C.kd_bwd(w_ce, w_kl, sv, tv, labels, stats, bs, bt, eps, -100, T, True)
    F.check("in place: same storage", res.data_ptr() == sv.data_ptr())
    F.add("ds (in place) per row", R.row_err(sv[rows], g_r[rows]), R.ROW_BOUND[dtype])
    F.add("ds (in place) per element", R.elem_err(sv[rows], g_r[rows], slack), ELEM_BOUND)
    F.check("in place: ignored rows zero, neighbours of the view untouched",
            not sv[~rows].any() and torch.equal(sbuf[:1], before[:1]) and torch.equal(sbuf[1 + N * V:], before[1 + N * V:]))


@pytest.mark.parametrize("bias", ["none", "student", "both"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("T", [1.0, 2.0])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("V", [1000, 1003])
def test_kd_fwd_bwd(V, dt, T, eps, bias):
    dtype = DT[dt]
    F = Figures(f"kd V={V} {dt} T={T} eps={eps} bias={bias}")
    s, t, labels, bs, bt = _inputs(37, V, dtype, seed=V)
    bs = None if bias == "none" else bs
    bt = bt if bias == "both" else None
    _check_kernels(F, s, t, labels, bs, bt, eps, T, dtype)
    F.done()


@pytest.mark.parametrize("V", [32128, 50265])
def test_kd_real_width(V):
    """One real vocabulary each (T5's, 16-B rows; BART's, odd, with both biases): several trips of the vector loop."""
    F = Figures(f"kd V={V} bf16")
    s, t, labels, bs, bt = _inputs(256, V, BF16, seed=V, ignored=(2, 17, 255), hot=(1, 200))
    if V == 32128:
        bs = bt = None
    _check_kernels(F, s, t, labels, bs, bt, 0.1, 2.0, BF16)
    F.done()


# ------------------------------------------------------------------------------------------- vocabulary chunks
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
    monkeypatch.setattr(D._ext, "native", lambda: spy)
    return out


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("V", [1003, 2056])
def test_lm_head_distill_loss_chunks(V, bias, calls, monkeypatch):
    """256-column chunks (>= 4, and at V = 1003 a ragged tail chunk that re-covers 5 columns, skip = 5) of two logits
    GEMMs of different widths against fp64 of the same bf16 operands; the full-logits kernels give the same loss."""
    N, ds, dt_, T, eps = 37, 64, 128, 2.0, 0.1
    F = Figures(f"kd chunks V={V} bias={bias}")
    gen = _gen(V + 7)
    h = torch.randn(N, ds, device=DEV, generator=gen).to(BF16)
    w = (torch.randn(V, ds, device=DEV, generator=gen) * ds ** -0.5).to(BF16)
    th = torch.randn(N, dt_, device=DEV, generator=gen).to(BF16)
    tw = (torch.randn(V, dt_, device=DEV, generator=gen) * dt_ ** -0.5).to(BF16)
    labels = torch.randint(0, V, (N,), device=DEV, generator=gen)
    labels[[2, 17, 36]] = -100
    labels[0], labels[1] = V - 1, V - 7  # in the tail chunk: past and inside the re-covered columns' neighbourhood
    bs = 0.5 * torch.randn(V, device=DEV, generator=gen) if bias else None
    bt = 0.5 * torch.randn(V, device=DEV, generator=gen) if bias else None
    # fp64 of the definition on the same operands
    h64, w64 = h.double().requires_grad_(True), w.double().requires_grad_(True)
    loss_r, ce_r, kl_r = D._reference(h64 @ w64.t(), th.double() @ tw.double().t(), labels,
                                      None if bs is None else bs.double(), None if bt is None else bt.double(), eps,
                                      -100, ALPHA, T)
    loss_r.backward()
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(lmhead_chunk_mb=0.02))
    assert D._chunk_cols(N, V) == 256
    chunks = D._chunks(V, 256)
    assert len(chunks) >= 4 and (chunks[-1][2] > 0) == (V == 1003)
    hg, wg = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    loss, ce, kl = D.lm_head_distill_loss(hg, wg, th, tw, labels, bias=bs, teacher_bias=bt, label_smoothing=eps,
                                          alpha=ALPHA, temperature=T)
    loss.backward()
    assert calls.count("kd_chunk_fwd") == len(chunks) and calls.count("kd_chunk_bwd") == len(chunks), calls
    assert "kd_fwd" not in calls and "ce_chunk_fwd" not in calls and "lmhead_ce_fwd" not in calls, calls
    for name, got, ref in (("loss", loss, loss_r), ("ce", ce, ce_r), ("kl", kl, kl_r)):
        F.add(name, abs(got.item() - ref.item()), 2e-3 * max(1.0, abs(ref.item())))
    F.add("dh per row", R.row_err(hg.grad, h64.grad), R.ROW_BOUND[BF16])
    F.add("dW per row", R.row_err(wg.grad, w64.grad), R.ROW_BOUND[BF16])
    F.check("no gradient reaches the teacher", th.grad is None and tw.grad is None)
    # the full-logits kernels on the same (bf16) logits
    del calls[:]
    full, _, _ = D.distill_loss(h @ w.t(), th @ tw.t(), labels, bias=bs, teacher_bias=bt, label_smoothing=eps,
                                alpha=ALPHA, temperature=T)
    assert calls == ["kd_fwd"], calls
    F.add("full-logits path loss", abs(full.item() - loss_r.item()), 2e-3 * max(1.0, abs(loss_r.item())))
    # rerun: the same bits
    hg2, wg2 = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    loss2, _, _ = D.lm_head_distill_loss(hg2, wg2, th, tw, labels, bias=bs, teacher_bias=bt, label_smoothing=eps,
                                         alpha=ALPHA, temperature=T)
    loss2.backward()
    F.check("rerun bit-identical", torch.equal(loss, loss2) and torch.equal(hg.grad, hg2.grad)
            and torch.equal(wg.grad, wg2.grad))
    F.done()


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_kd_reruns_bit_identical(dt):
    C = _ext.native()
    s, t, labels, bs, bt = _inputs(37, 1003, DT[dt], seed=5)
    w = torch.full((1,), 0.01, device=DEV)
    outs = []
    for _ in range(2):
        ce, kl, stats = C.kd_fwd(s, t, labels, bs, bt, 0.1, -100, 2.0)
        outs.append((ce, kl, stats, C.kd_bwd(w, w, s, t, labels, stats, bs, bt, 0.1, -100, 2.0, False)))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_kd_bindings_reject_what_the_kernels_cannot_address():
    C = _ext.native()
    N, V = 8, 1001
    s, t = torch.randn(N, V, device=DEV), torch.randn(N, V, device=DEV)
    labels = torch.zeros(N, dtype=torch.long, device=DEV)
    C.kd_fwd(s, t, labels, None, None, 0.0, -100, 2.0)  # well-formed: passes
    wide = torch.randn(N, 2 * V, device=DEV)
    with pytest.raises(RuntimeError, match="student"):
        C.kd_fwd(wide[:, :V], t, labels, None, None, 0.0, -100, 2.0)
    with pytest.raises(RuntimeError, match="teacher"):
        C.kd_fwd(s, wide[:, :V], labels, None, None, 0.0, -100, 2.0)
    with pytest.raises(RuntimeError, match="teacher"):
        C.kd_fwd(s, t.to(BF16), labels, None, None, 0.0, -100, 2.0)
    with pytest.raises(RuntimeError, match="teacher"):
        C.kd_fwd(s, t[:, :V - 1].contiguous(), labels, None, None, 0.0, -100, 2.0)
    with pytest.raises(RuntimeError, match="teacher"):
        C.kd_fwd(s, t[:N - 1], labels, None, None, 0.0, -100, 2.0)
    with pytest.raises(RuntimeError, match="teacher"):
        C.kd_fwd(s, t.cpu(), labels, None, None, 0.0, -100, 2.0)
    with pytest.raises(RuntimeError, match="labels"):
        C.kd_fwd(s, t, labels[:N - 1], None, None, 0.0, -100, 2.0)
    with pytest.raises(RuntimeError, match="bias_s"):
        C.kd_fwd(s, t, labels, torch.zeros(V - 1, device=DEV), None, 0.0, -100, 2.0)
    with pytest.raises(RuntimeError, match="bias_t"):
        C.kd_fwd(s, t, labels, None, torch.zeros(V + 1, device=DEV), 0.0, -100, 2.0)
    with pytest.raises(RuntimeError, match="temperature"):
        C.kd_fwd(s, t, labels, None, None, 0.0, -100, 0.0)
    stats, w = torch.zeros(N, 3, device=DEV), torch.ones(1, device=DEV)
    with pytest.raises(RuntimeError, match="stats"):
        C.kd_bwd(w, w, s, t, labels, stats[:, :2].contiguous(), None, None, 0.0, -100, 2.0, False)
    with pytest.raises(RuntimeError, match="w_kl"):
        C.kd_bwd(w, w.double(), s, t, labels, stats, None, None, 0.0, -100, 2.0, False)
    with pytest.raises(RuntimeError, match="w_ce"):
        C.kd_bwd(w.cpu(), w, s, t, labels, stats, None, None, 0.0, -100, 2.0, False)
    with pytest.raises(RuntimeError, match="temperature"):
        C.kd_bwd(w, w, s, t, labels, stats, None, None, 0.0, -100, -1.0, False)
    # chunk forms
    Vc = 256
    cs, ct = torch.zeros(N, Vc, device=DEV, dtype=BF16), torch.zeros(N, Vc, device=DEV, dtype=BF16)
    state, ce, kl = torch.zeros(N, 8, device=DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    C.kd_chunk_fwd(cs, ct, labels, None, None, state, ce, kl, stats, 0, V, 0.0, -100, 2.0, True, False, 0)
    with pytest.raises(RuntimeError, match="student"):
        C.kd_chunk_fwd(cs.float(), ct, labels, None, None, state, ce, kl, stats, 0, V, 0.0, -100, 2.0, True, False, 0)
    with pytest.raises(RuntimeError, match="teacher"):
        C.kd_chunk_fwd(cs, ct[:, :Vc - 4], labels, None, None, state, ce, kl, stats, 0, V, 0.0, -100, 2.0, True, False, 0)
    with pytest.raises(RuntimeError, match="state"):
        C.kd_chunk_fwd(cs, ct, labels, None, None, state[:, :4].contiguous(), ce, kl, stats, 0, V, 0.0, -100, 2.0, True,
                       False, 0)
    with pytest.raises(RuntimeError, match="vocabulary"):
        C.kd_chunk_fwd(cs, ct, labels, None, None, state, ce, kl, stats, V - 8, V, 0.0, -100, 2.0, True, False, 0)
    with pytest.raises(RuntimeError, match="skip"):
        C.kd_chunk_fwd(cs, ct, labels, None, None, state, ce, kl, stats, 0, V, 0.0, -100, 2.0, True, False, Vc)
    with pytest.raises(RuntimeError, match="bias"):
        C.kd_chunk_bwd(w, w, cs, ct, labels, stats, torch.zeros(V - 1, device=DEV), None, 0, V, 0.0, -100, 2.0, 0)
    with pytest.raises(RuntimeError, match="labels"):
        C.kd_chunk_bwd(w, w, cs, ct, labels[:N - 1], stats, None, None, 0, V, 0.0, -100, 2.0, 0)
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


def _distilled(student, teacher, batch, seed=5, alpha=0.5, T=2.0):
    from distributed_llms_example_amd.models.distill import Distill
    from distributed_llms_example_amd.ops.rng import manual_seed
    manual_seed(seed)  # same dropout masks on every path; the teacher (eval) draws none
    with torch.no_grad():
        th, tw, tb = teacher.lm_head_operands(**batch)
    out = student(**batch, label_smoothing=0.1, distill=Distill(th, tw, tb, alpha, T))
    out.loss.backward()
    return out


@pytest.mark.parametrize("name", ["t5-tiny", "bart-tiny"])
def test_model_distill_bf16_vs_fp32_composite(name, calls, monkeypatch):
    """A bf16 student and teacher on the kernels against the same models in fp32 on the torch composite, by the method
    and bounds of tests/test_model_gpu.py::test_native_bf16_matches_fp32_reference: bf16-representable weights, the
    same dropout masks, loss (and here both components) within 1 %, every parameter's gradient within 1.5x of what the
    torch composite run in bf16 costs on that parameter (floors 3e-2 relative, 1e-3 cosine deficit)."""
    from distributed_llms_example_amd.models import build_model, resolve_config
    from distributed_llms_example_amd.models.distill import make_student
    cfg = resolve_config(name)
    torch.manual_seed(0)
    t32 = build_model(cfg).to(DEV)
    with torch.no_grad():
        if name.startswith("bart"):
            t32.final_logits_bias.normal_(0.0, 0.5)
        for p in t32.parameters():
            p.copy_(p.to(BF16).float())
        for b in t32.buffers():
            if b.is_floating_point():
                b.copy_(b.to(BF16).float())
    t32.eval().requires_grad_(False)
    m32 = make_student(t32, 1, 1)
    with torch.no_grad():  # a student that has moved away from the layers it copied
        for p in m32.parameters():
            p.copy_((p + 0.02 * torch.randn_like(p)).to(BF16).float())
    m32.train()
    m16, c16 = (copy.deepcopy(m32).to(BF16).train() for _ in range(2))
    t16 = copy.deepcopy(t32).to(BF16).eval()
    B, S, T = 4, 200, 40
    g = torch.Generator().manual_seed(0)
    batch = {"input_ids": torch.randint(3, cfg.vocab_size, (B, S), generator=g).to(DEV),
             "attention_mask": torch.ones(B, S, dtype=torch.long, device=DEV),
             "labels": torch.randint(3, cfg.vocab_size, (B, T), generator=g).to(DEV)}
    batch["attention_mask"][1, -33:] = 0
    batch["labels"][2, -5:] = -100
    monkeypatch.setenv("DLLM_REFERENCE_OPS", "1")
    ref = _distilled(m32, t32, batch)
    _distilled(c16, t16, batch)
    monkeypatch.delenv("DLLM_REFERENCE_OPS")
    del calls[:]
    out = _distilled(m16, t16, batch)
    assert "kd_fwd" in calls and "kd_bwd" in calls, calls
    assert out.logits is None and not any(p.grad is not None for p in t16.parameters())
    F = Figures(f"model {name}")
    for k in ("loss", "ce_loss", "kd_loss"):
        a, b = getattr(out, k).item(), getattr(ref, k).item()
        F.add(k, abs(a - b), 0.01 * abs(b))
    floor = {n: (rel, cos) for rel, cos, n in _grad_report(c16, m32)}
    rep = _grad_report(m16, m32)
    assert len(rep) >= len(list(m32.parameters())) - 1
    for rel, cos, n in rep:
        frel, fcos = floor[n]
        F.add(f"grad {n} rel", rel, max(3e-2, 1.5 * frel))
        F.add(f"grad {n} 1-cos", 1 - cos, max(1e-3, 1.5 * (1 - fcos)))
    F.done()


@pytest.fixture
def _no_leaked_step_seeds():
    from distributed_llms_example_amd.ops import rng as rng_mod
    yield
    st = rng_mod._active_step[0]
    if st is not None:
        st.disable()
    rng_mod.default_rng().site_mode = False


def test_graphed_step_with_teacher_equals_eager(_no_leaked_step_seeds):
    """Steps with a teacher captured as a HIP graph (the teacher's forward inside) replay and equal the same steps run
    eagerly: the method and bounds of tests/test_graph_gpu.py::test_graphed_steps_match_eager at ga = 1."""
    from distributed_llms_example_amd.models import build_model, resolve_config
    from distributed_llms_example_amd.models.distill import make_student
    from distributed_llms_example_amd.ops.rng import manual_seed
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    from distributed_llms_example_amd.train.graph import GraphedStep
    env = init_distributed()
    cfg = resolve_config("t5-base").replace(num_layers=2, num_decoder_layers=2, vocab_size=4096)
    torch.manual_seed(0)
    teacher = build_model(cfg)
    student = make_student(teacher, 1, 1)
    g = torch.Generator().manual_seed(3)
    steps = 2
    data = [{"input_ids": torch.randint(3, cfg.vocab_size, (4, 256), generator=g).cuda(),
             "attention_mask": torch.ones(4, 256, dtype=torch.long).cuda(),
             "labels": torch.randint(3, cfg.vocab_size, (4, 64), generator=g).cuda()} for _ in range(steps + 2)]

    def engine():
        manual_seed(11)
        eng = TrainEngine(copy.deepcopy(student), env, lr=1e-3, dtype=BF16, bucket_mb=8.0,
                          teacher=copy.deepcopy(teacher), kd_alpha=0.5, kd_temperature=2.0)
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
    assert eng_e.last_kd_loss is not None and float(eng_e.last_kd_loss) > 0
    assert losses_g == pytest.approx(losses_e, rel=1e-3), (losses_g, losses_e)
    assert ((pg - pe).norm() / pe.norm()).item() < 1e-3
