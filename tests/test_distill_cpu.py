"""Knowledge distillation on the CPU: the torch composite of the loss against an independent fp64 statement, the
no-materialised-logits form against the full one, ``make_student``, the engine with a teacher (frozen teacher, same
flat buffers / optimizer state / dropout seeds as a run without one, ``alpha = 0`` is the plain engine, token-count
normalisation, two gloo ranks), the Trainer entry point, and every loud error."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import rowwise_refs as R
from distributed_llms_example_amd.models import build_model, resolve_config
from distributed_llms_example_amd.models.distill import Distill, layer_picks, make_student
from distributed_llms_example_amd.ops import distill as D
from distributed_llms_example_amd.parallel.flat import FlatParams
from test_distributed_cpu import run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the loss
def _statement64(s, t, labels, eps, alpha, T):
    """The definition in fp64 from torch's own losses: F.cross_entropy + F.kl_div(log_target=True)."""
    s = s.double()
    t = t.double()
    valid = labels != -100
    count = max(1, int(valid.sum()))
    ce = F.cross_entropy(s, labels, ignore_index=-100, label_smoothing=eps, reduction="sum") / count
    kl_el = F.kl_div(F.log_softmax(s / T, -1), F.log_softmax(t / T, -1), reduction="none", log_target=True)
    kl = (kl_el.sum(-1) * valid).sum() / count
    return (1 - alpha) * ce + alpha * T * T * kl, ce, kl


def _logits(all_ignored=False):
    g = torch.Generator().manual_seed(0)
    N, V = 7, 1003
    s = torch.randn(N, V, generator=g) * 2
    t = 0.6 * s + torch.randn(N, V, generator=g) * 1.5
    s[1] *= 20
    t[1] *= 20
    s[4] *= 20
    t[4] *= 20
    labels = torch.randint(0, V, (N,), generator=g)
    labels[3] = -100
    if all_ignored:
        labels[:] = -100
    return s, t, labels


@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("T", [1.0, 2.0])
@pytest.mark.parametrize("all_ignored", [False, True])
def test_composite_against_fp64_statement(all_ignored, T, eps, alpha):
    s, t, labels = _logits(all_ignored)
    s64 = s.double().requires_grad_(True)
    ref, ce_r, kl_r = _statement64(s64, t, labels, eps, alpha, T)
    ref.backward()
    sg = s.clone().requires_grad_(True)
    loss, ce, kl = D.distill_loss(sg, t, labels, label_smoothing=eps, alpha=alpha, temperature=T)
    loss.backward()
    assert not ce.requires_grad and not kl.requires_grad
    for got, want in ((loss, ref), (ce, ce_r), (kl, kl_r)):
        torch.testing.assert_close(got.double(), want.detach(), rtol=1e-5, atol=0)
    rows = labels != -100
    if all_ignored:
        assert float(loss) == 0.0 and not sg.grad.any()
    else:
        assert R.row_err(sg.grad[rows], s64.grad[rows]) < R.ROW_BOUND[torch.float32]
        assert not sg.grad[~rows].any()


def test_composite_takes_both_biases():
    s, t, labels = _logits()
    g = torch.Generator().manual_seed(1)
    bs, bt = torch.randn(s.shape[1], generator=g), torch.randn(s.shape[1], generator=g)
    ref, _, _ = _statement64(s + bs, t + bt, labels, 0.1, 0.5, 2.0)
    loss, _, _ = D.distill_loss(s, t, labels, bias=bs, teacher_bias=bt, label_smoothing=0.1, alpha=0.5, temperature=2.0)
    torch.testing.assert_close(loss.double(), ref, rtol=1e-5, atol=0)


@pytest.mark.parametrize("who", ["teacher", "both", "student"])
@pytest.mark.parametrize("T", [1.0, 2.0, 0.7])
def test_composite_obeys_the_inf_contract(who, T):
    """-inf bias entries (banned tokens) on the teacher, on both models (a student made by ``make_student`` carries the
    teacher's bias) and on the student alone, eps = 0: the composite's ce and kl equal the fp64 reference of
    tests/loss_refs.py (kl finite where only p_v = 0 columns are banned, +inf where the student bans a column the
    teacher gives mass), and the autograd gradient is finite and equals the reference's."""
    import loss_refs as L
    N, V, alpha = 7, 1003, 0.5
    case = L.kd_case(N, V, torch.float32, hot_scale=L.INF_HOT_SCALE)
    bs, bt, labels = L.kd_ban(case, case["bs"], case["bt"], L.kd_banned_columns(V), who, V)
    labels = torch.where(L.valid_rows(labels, -100, V), labels, torch.full_like(labels, -100))
    count = int((labels != -100).sum())
    ce_r, kl_r, _, ds_r = L.kd_ref(case["s"], case["t"], labels, bs, bt, 0.0, -100, V, T, (1 - alpha) / count,
                                   alpha / count)
    assert bool(torch.isfinite(ce_r).all()) and bool(torch.isfinite(ds_r).all())
    sg = case["s"].clone().requires_grad_(True)
    loss, ce, kl = D.distill_loss(sg, case["t"], labels, bias=bs, teacher_bias=bt, label_smoothing=0.0, alpha=alpha,
                                  temperature=T)
    loss.backward()
    torch.testing.assert_close(ce.double(), ce_r.sum() / count, rtol=1e-5, atol=0)
    if who == "student":
        assert kl.item() == float("inf") and loss.item() == float("inf")
        assert bool(torch.isinf(kl_r[labels != -100]).all())
    else:
        assert bool(torch.isfinite(kl_r).all())
        torch.testing.assert_close(kl.double(), kl_r.sum() / count, rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(loss.double(), (1 - alpha) * ce_r.sum() / count + alpha * T * T * kl_r.sum() / count,
                                   rtol=1e-5, atol=1e-7)
    assert bool(torch.isfinite(sg.grad).all())
    rows = labels != -100
    assert R.row_err(sg.grad[rows], ds_r[rows]) < R.ROW_BOUND[torch.float32]
    assert not sg.grad[~rows].any()
    # the definition is unchanged on finite inputs: the fp64 composite is the fp64 reference
    s64 = case["s"].double()
    _, ce64, kl64 = D.distill_loss(s64, case["t"].double(), labels, bias=case["bs"].double(),
                                   teacher_bias=case["bt"].double(), label_smoothing=0.1, alpha=alpha, temperature=T)
    ce_f, kl_f, _, _ = L.kd_ref(case["s"], case["t"], labels, case["bs"], case["bt"], 0.1, -100, V, T)
    torch.testing.assert_close(ce64, ce_f.sum() / count, rtol=1e-12, atol=0)
    torch.testing.assert_close(kl64, kl_f.sum() / count, rtol=1e-10, atol=0)


def test_lm_head_distill_loss_composite_equals_full():
    """The no-materialised-logits entry on its composite path (CPU, fp32) against the loss on explicit logits: loss,
    components, dh and dW; the student and the teacher differ in width."""
    g = torch.Generator().manual_seed(2)
    N, V, ds, dt = 7, 1003, 64, 128
    h = torch.randn(2, N, ds, generator=g)
    w = torch.randn(V, ds, generator=g) * ds ** -0.5
    th = torch.randn(2, N, dt, generator=g)
    tw = torch.randn(V, dt, generator=g) * dt ** -0.5
    bs, bt = torch.randn(V, generator=g), torch.randn(V, generator=g)
    labels = torch.randint(0, V, (2, N), generator=g)
    labels[1, 3:] = -100
    scale = ds ** -0.5
    h1, w1 = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    out = D.lm_head_distill_loss(h1, w1, th, tw, labels, scale=scale, bias=bs, teacher_bias=bt, label_smoothing=0.1,
                                 alpha=0.7, temperature=2.0)
    out[0].backward()
    h2, w2 = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    ref = D.distill_loss(F.linear(h2.reshape(-1, ds) * scale, w2), F.linear(th.reshape(-1, dt), tw), labels.reshape(-1),
                         bias=bs, teacher_bias=bt, label_smoothing=0.1, alpha=0.7, temperature=2.0)
    ref[0].backward()
    for a, b in zip(out, ref):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=0)
    torch.testing.assert_close(h1.grad, h2.grad, rtol=1e-5, atol=1e-8)
    torch.testing.assert_close(w1.grad, w2.grad, rtol=1e-5, atol=1e-8)
    th.requires_grad_(True)  # the teacher takes no gradient even when it could
    D.lm_head_distill_loss(h1, w1, th, tw, labels, alpha=0.5, temperature=2.0)[0].backward()
    assert th.grad is None


# ---------------------------------------------------------------------------------------------------------- the student
def test_layer_picks():
    assert layer_picks(12, 6) == [0, 2, 4, 7, 9, 11]
    assert layer_picks(12, 3) == [0, 6, 11]
    assert layer_picks(12, 1) == [0]
    assert layer_picks(6, 6) == list(range(6))
    for L in range(1, 13):
        for k in range(1, L + 1):
            p = layer_picks(L, k)
            assert p[0] == 0 and len(p) == k and p == sorted(set(p)) and (k == 1 or p[-1] == L - 1)
    with pytest.raises(ValueError, match="layers"):
        layer_picks(6, 7)


@pytest.mark.parametrize("name", ["t5-tiny", "bart-tiny", "led-tiny"])
def test_make_student(name, tmp_path):
    import transformers
    from distributed_llms_example_amd.models import save_pretrained
    torch.manual_seed(0)
    cfg = resolve_config(name)
    kw = dict(num_layers=4, num_decoder_layers=4)
    if name == "led-tiny":
        kw["attention_window"] = [4, 8, 12, 16]
    teacher = build_model(cfg.replace(**kw))
    if teacher.logits_bias() is not None:
        with torch.no_grad():
            teacher.final_logits_bias.normal_()
    student = make_student(teacher, 2, 3)
    assert (student.config.num_layers, student.config.num_decoder_layers) == (2, 3)
    assert student.config.vocab_size == teacher.config.vocab_size and student.config.d_model == teacher.config.d_model
    tsd, ssd = teacher.state_dict(), student.state_dict()
    enc, dec = layer_picks(4, 2), layer_picks(4, 3)
    assert enc == [0, 3] and dec == [0, 2, 3]
    pre = ("encoder.block.{}.", "decoder.block.{}.") if name == "t5-tiny" else \
        ("model.encoder.layers.{}.", "model.decoder.layers.{}.")
    seen = 0
    for k, v in ssd.items():
        src = k
        for fmt, picks in zip(pre, (enc, dec)):
            for i, j in enumerate(picks):
                if k.startswith(fmt.format(i)):
                    src = fmt.format(j) + k[len(fmt.format(i)):]
                    seen += 1
        assert torch.equal(v, tsd[src]), k
    assert seen > 10
    if name == "t5-tiny":  # layer 0 kept, and the relative-bias table with it
        assert any("relative_attention_bias" in k and ".block.0." in k for k in ssd)
    else:
        assert torch.equal(student.final_logits_bias, teacher.final_logits_bias) and student.final_logits_bias.any()
    if name == "led-tiny":
        assert student.config.attention_window == [4, 16]
    save_pretrained(student, str(tmp_path))
    hf = transformers.AutoModelForSeq2SeqLM.from_pretrained(str(tmp_path), attn_implementation="eager").eval()
    hc = hf.config
    assert (getattr(hc, "num_layers", None) or hc.encoder_layers) == 2
    assert (getattr(hc, "num_decoder_layers", None) or hc.decoder_layers) == 3
    # the student is the teacher's function family: its own forward equals transformers' on the saved weights
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab_size, (2, 16), generator=g)
    lab = torch.randint(3, cfg.vocab_size, (2, 5), generator=g)
    kw = {}
    if name == "led-tiny":
        gm = torch.zeros_like(ids)
        gm[:, 0] = 1
        kw["global_attention_mask"] = gm
    with torch.no_grad():
        ours = student.eval()(input_ids=ids, attention_mask=torch.ones_like(ids), labels=lab, **kw).loss
        theirs = hf(input_ids=ids, attention_mask=torch.ones_like(ids), labels=lab, **kw).loss
    torch.testing.assert_close(ours, theirs, rtol=1e-4, atol=1e-5)


# ----------------------------------------------------------------------------------------------------------- the engine
def _batch(B=4, S=12, T=6, seed=7, V=500):
    g = torch.Generator().manual_seed(seed)
    b = {"input_ids": torch.randint(3, V, (B, S), generator=g), "attention_mask": torch.ones(B, S, dtype=torch.long),
         "labels": torch.randint(3, V, (B, T), generator=g)}
    b["labels"][0, -2:] = -100
    return b


def _engine(teacher=True, alpha=0.5, name="t5-tiny", train=True, **kw):
    from distributed_llms_example_amd.ops.rng import manual_seed
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    torch.manual_seed(0)
    t = build_model(name)
    m = make_student(t, 1, 1)
    manual_seed(11)
    eng = TrainEngine(m, init_distributed(cpu=True), lr=1e-2, dtype=torch.float32, teacher=t if teacher else None,
                      kd_alpha=alpha, kd_temperature=2.0, **kw)
    eng.train(train)
    return eng


def test_engine_keeps_the_teacher_frozen_and_outside_the_training_state():
    eng, plain = _engine(), _engine(teacher=False)
    before = {k: v.clone() for k, v in eng.teacher.state_dict().items()}
    b = _batch()
    for _ in range(3):
        eng.forward_backward(b)
        eng.step()
        plain.forward_backward(b)
        plain.step()
    assert not eng.teacher.training
    for k, v in eng.teacher.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(p.grad is None and not p.requires_grad for p in eng.teacher.parameters())
    assert eng.flat.numel == plain.flat.numel and eng.flat.param_buf.shape == plain.flat.param_buf.shape
    so, po = eng.optimizer.state_dict(), plain.optimizer.state_dict()
    sizes = lambda sd: sorted(v.numel() for v in sd.values() if torch.is_tensor(v))  # noqa: E731
    assert sizes(so) == sizes(po) and sizes(so)
    ids = {id(p) for p in eng.teacher.parameters()}
    assert not ids & {id(p) for p in eng.model.parameters()}
    assert eng.last_ce_loss is not None and float(eng.last_kd_loss) > 0 and plain.last_kd_loss is None
    assert not torch.equal(eng.flat.param_buf, plain.flat.param_buf)  # it did distil


def test_engine_student_draws_the_same_dropout_seeds(monkeypatch):
    """The teacher (``eval()``) draws nothing from the dropout seed stream: the student's seeds are those of a run
    without a teacher, recorded where ops/rng.py hands them out."""
    from distributed_llms_example_amd.ops import rng as rng_mod
    real = rng_mod.DropoutRNG.next_seed
    rec = []

    def spy(self):
        s = real(self)
        rec.append(s)
        return s
    monkeypatch.setattr(rng_mod.DropoutRNG, "next_seed", spy)
    seeds = {}
    for teacher in (True, False):
        eng = _engine(teacher=teacher)
        assert eng.model.config.dropout_rate > 0
        if teacher:  # the teacher's own draws (a scope of its own) are not the student's
            ops = eng.teacher.lm_head_operands

            def quiet(*a, _ops=ops, **k):
                n = len(rec)
                out = _ops(*a, **k)
                del rec[n:]
                return out
            eng.teacher.lm_head_operands = quiet
        del rec[:]
        for _ in range(2):
            eng.forward_backward(_batch())
            eng.step()
        seeds[teacher] = list(rec)
    assert seeds[True] == seeds[False] and len(seeds[True]) > 4


@pytest.mark.parametrize("name", ["t5-tiny", "bart-tiny"])
def test_engine_alpha_zero_is_the_plain_engine(name):
    a, b = _engine(alpha=0.0, name=name, label_smoothing=0.1), _engine(teacher=False, name=name, label_smoothing=0.1)
    from distributed_llms_example_amd.ops.rng import manual_seed
    batch = _batch()
    manual_seed(5)  # the same dropout masks for both
    la = a.forward_backward(batch)
    manual_seed(5)
    lb = b.forward_backward(batch)
    torch.testing.assert_close(la, lb, atol=1e-6, rtol=0)
    torch.testing.assert_close(a.flat.grad_buf, b.flat.grad_buf, atol=1e-6, rtol=0)
    assert a.flat.grad_buf.abs().sum() > 0


def test_engine_num_items_two_unequal_micro_batches_equal_one_batch():
    big = _batch(B=6)
    big["labels"][4, 1:] = -100  # the two halves hold different token counts
    parts = [{k: v[:2] for k, v in big.items()}, {k: v[2:] for k, v in big.items()}]
    from distributed_llms_example_amd.train.engine import token_count
    n = token_count(big["labels"])
    assert token_count(parts[0]["labels"]) != token_count(parts[1]["labels"])
    one, two = _engine(train=False), _engine(train=False)  # eval mode: no dropout, as the two-rank case
    one.forward_backward(big, num_items=n)
    two.forward_backward(parts[0], grad_accum=2, sync=False, num_items=n)
    two.forward_backward(parts[1], grad_accum=2, sync=True, num_items=n)
    assert one.last_kd_loss is not None and two.last_kd_loss is not None
    torch.testing.assert_close(two.flat.grad_buf, one.flat.grad_buf, atol=1e-6, rtol=1e-5)


def _kd_grad_case(rank, world):
    from distributed_llms_example_amd.parallel.env import DistEnv
    from distributed_llms_example_amd.train.engine import TrainEngine
    torch.manual_seed(0)
    teacher = build_model("t5-tiny")
    model = make_student(teacher, 1, 1)
    env = DistEnv(rank=rank, world_size=world, backend="gloo", device=torch.device("cpu"))
    if rank == 1:  # a different student on rank 1: the broadcast must overwrite it
        with torch.no_grad():
            for p in model.parameters():
                p.add_(1.0)
    os.environ["DLLM_ROUTE"] = "reducer=python"
    eng = TrainEngine(model, env, lr=1e-3, dtype=torch.float32, bucket_mb=0.01, overlap=True, teacher=teacher,
                      kd_alpha=0.5, kd_temperature=2.0)
    eng.train(False)
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(3, 500, (4 * world, 10), generator=g)
    lab = torch.randint(3, 500, (4 * world, 5), generator=g)
    s = slice(rank * 4, rank * 4 + 4)
    eng.forward_backward({"input_ids": ids[s], "attention_mask": torch.ones_like(ids[s]), "labels": lab[s]})
    return (eng.flat.to_canonical(eng.flat.grad_buf).clone(), eng.flat.to_canonical(eng.flat.param_buf).clone(),
            len(eng.reducer.buckets))


def test_two_ranks_with_a_teacher_match_single_process():
    """Method and bounds of tests/test_lora_cpu.py::test_two_ranks_with_adapters_match_single_process."""
    out = run_ranks(_kd_grad_case)
    torch.manual_seed(0)
    teacher = build_model("t5-tiny").eval()
    model = make_student(teacher, 1, 1).eval()
    flat = FlatParams(model)
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(3, 500, (8, 10), generator=g)
    lab = torch.randint(3, 500, (8, 5), generator=g)
    loss = 0
    for r in range(2):
        b = dict(input_ids=ids[r * 4:(r + 1) * 4], attention_mask=torch.ones(4, 10, dtype=torch.long),
                 labels=lab[r * 4:(r + 1) * 4])
        with torch.no_grad():
            th, tw, tb = teacher.lm_head_operands(**b)
        loss = loss + model(**b, distill=Distill(th, tw, tb, 0.5, 2.0)).loss / 2
    loss.backward()
    g0, p0, nb = (torch.as_tensor(x) if not isinstance(x, int) else x for x in out[0])
    g1, p1, _ = (torch.as_tensor(x) if not isinstance(x, int) else x for x in out[1])
    assert nb > 1 and g0.numel() == flat.numel
    torch.testing.assert_close(g0, g1)
    torch.testing.assert_close(p0, p1)
    torch.testing.assert_close(p0, flat.param_buf)
    torch.testing.assert_close(g0, flat.grad_buf, atol=1e-5, rtol=1e-4)


def test_model_forward_with_distill_returns_components_and_logits():
    torch.manual_seed(0)
    for name in ("t5-tiny", "bart-tiny"):
        t = build_model(name).eval()
        m = make_student(t, 1, 1).eval()
        b = _batch()
        plain = m(**b)
        assert plain.ce_loss is None and plain.kd_loss is None
        with torch.no_grad():
            th, tw, tb = t.lm_head_operands(**b)
            full = t(**b, return_logits=True).logits
        assert th.shape == (4, 6, t.config.d_model) and tw.shape[0] == t.config.vocab_size
        tl = F.linear(th, tw) + (tb if tb is not None else 0)
        torch.testing.assert_close(tl, full, rtol=1e-5, atol=1e-5)  # the operands ARE the teacher's logits
        out = m(**b, distill=Distill(th, tw, tb, 0.5, 2.0), return_logits=True)
        torch.testing.assert_close(out.logits, m(**b, return_logits=True).logits)
        torch.testing.assert_close(out.loss, 0.5 * out.ce_loss + 0.5 * 4.0 * out.kd_loss)
        torch.testing.assert_close(out.ce_loss, plain.loss)


# ---------------------------------------------------------------------------------------------------------- entry point
def test_train_torchrun_distils_a_student(tmp_path):
    import transformers
    from safetensors import safe_open
    env = dict(os.environ)
    env.update({"VH_ROOT": str(tmp_path), "DLLM_FORCE_CPU": "1", "OMP_NUM_THREADS": "2", "PYTHONPATH": ROOT})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train-torchrun.py"), "--teacher-ckpt", "t5-tiny",
                        "--student-layers", "1,1", "--output-dir", "out", "--batch-size", "4", "--grad-accum", "2",
                        "--evaluation-steps", "100", "--warmup-steps", "1", "--synthetic", "80",
                        "--max-source-length", "40", "--max-target-length", "10", "--gen-max-length", "8"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    logs = [json.loads(l) for l in r.stdout.splitlines() if l.strip().startswith("{")]
    kd = [x for x in logs if "kd_loss" in x]
    assert kd and all("ce_loss" in x and "loss" in x and x["kd_loss"] > 0 for x in kd)
    out = tmp_path / "outputs" / "out"
    hf = transformers.AutoModelForSeq2SeqLM.from_pretrained(str(out), attn_implementation="eager")
    assert hf.config.num_layers == 1 and hf.config.num_decoder_layers == 1
    with safe_open(str(out / "model.safetensors"), "pt") as f:
        keys = list(f.keys())
    assert keys and not any("teacher" in k for k in keys)
    assert not any(".block.1." in k for k in keys)  # one layer each: nothing of the two-layer teacher
    assert len(keys) == len(hf.state_dict()) - sum(k.endswith("embed_tokens.weight") or k == "lm_head.weight"
                                                   for k in hf.state_dict())  # the student's tensors, no second model


# --------------------------------------------------------------------------------------------------------------- errors
def _args(*argv, **kw):
    from distributed_llms_example_amd.cli import base_parser
    a = base_parser("t").parse_args(list(argv))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_loud_errors():
    from distributed_llms_example_amd.cli import build_models, resolve_distill
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    s, t, labels = _logits()
    for alpha in (-0.1, 1.1):
        with pytest.raises(ValueError, match="alpha"):
            D.distill_loss(s, t, labels, alpha=alpha, temperature=2.0)
    for T in (0.0, -1.0):
        with pytest.raises(ValueError, match="temperature"):
            D.distill_loss(s, t, labels, alpha=0.5, temperature=T)
    with pytest.raises(ValueError, match="vocabulary"):
        D.distill_loss(s, t[:, :-1], labels, alpha=0.5, temperature=2.0)
    env = init_distributed(cpu=True)
    torch.manual_seed(0)
    teacher = build_model("t5-tiny")
    other = build_model(resolve_config("t5-tiny").replace(vocab_size=resolve_config("t5-tiny").vocab_size + 8))
    with pytest.raises(ValueError, match="vocab_size"):
        TrainEngine(other, env, dtype=torch.float32, teacher=teacher)
    with pytest.raises(ValueError, match="alpha"):
        TrainEngine(make_student(teacher, 1, 1), env, dtype=torch.float32, teacher=teacher, kd_alpha=2.0)
    with pytest.raises(ValueError, match="temperature"):
        TrainEngine(make_student(teacher, 1, 1), env, dtype=torch.float32, teacher=teacher, kd_temperature=0.0)
    # a model-level mismatch is caught where the two heads meet, too
    b = _batch()
    with torch.no_grad():
        th, tw, tb = teacher.lm_head_operands(**b)
    with pytest.raises(ValueError, match="vocabulary"):
        other(**b, distill=Distill(th, tw, tb, 0.5, 2.0))
    # command line
    with pytest.raises(ValueError, match="--teacher-ckpt"):
        resolve_distill(_args("--student-layers", "1,1"))
    for spelling in ("--model-ckpt", "--model-c"):  # argparse takes unambiguous prefixes
        with pytest.raises(ValueError, match="both"):
            resolve_distill(_args("--student-layers", "1,1", "--teacher-ckpt", "t5-tiny", spelling, "t5-tiny"))
    with pytest.raises(ValueError, match="both"):
        resolve_distill(_args("--student-layers=1,1", "--teacher-ckpt=t5-tiny", "--model-ckpt=t5-tiny"))
    with pytest.raises(ValueError, match="--model-overrides"):
        resolve_distill(_args("--student-layers", "1,1", "--teacher-ckpt", "t5-tiny", "--model-overrides", "d_ff=64"))
    with pytest.raises(ValueError, match="E,D"):
        resolve_distill(_args("--student-layers", "1", "--teacher-ckpt", "t5-tiny"))
    with pytest.raises(ValueError, match="alpha"):
        resolve_distill(_args(teacher_ckpt="t5-tiny", kd_alpha=1.5))
    with pytest.raises(ValueError, match="temperature"):
        resolve_distill(_args(teacher_ckpt="t5-tiny", kd_temperature=0.0))
    with pytest.raises(NotImplementedError, match="context-parallel"):
        resolve_distill(_args(teacher_ckpt="t5-tiny", context_parallel=2))
    with pytest.raises(ValueError, match="vocab_size"):
        build_models(_args(teacher_ckpt="t5-tiny", model_ckpt="bart-base"), resolve_config("bart-base"))
    # context parallelism enabled on the student model itself
    student = make_student(teacher, 1, 1)
    student.encoder._cp_group = None
    with pytest.raises(NotImplementedError, match="context-parallel"):
        TrainEngine(student, env, dtype=torch.float32, teacher=teacher)


def test_student_layers_resolve_once_or_twice():
    """``model_config`` and ``build_models`` both resolve the flags, on the same ``args``: the second time changes
    nothing, and the config the data is built with is the config of the model that is trained."""
    from distributed_llms_example_amd.cli import build_models, model_config
    a = _args("--teacher-ckpt", "t5-tiny", "--student-layers", "1,1")
    cfg = model_config(a)
    assert a.student_layers == (1, 1) and a.model_ckpt == "t5-tiny"
    assert model_config(a) == cfg and a.student_layers == (1, 1)
    torch.manual_seed(0)
    model, teacher = build_models(a, cfg)
    assert model.config == cfg and (cfg.num_layers, cfg.num_decoder_layers) == (1, 1)
    assert teacher.config.num_layers == resolve_config("t5-tiny").num_layers


def test_flags_default_to_no_teacher():
    a = _args()
    assert a.teacher_ckpt is None and a.student_layers is None and a.kd_alpha == 0.5 and a.kd_temperature == 2.0
    from distributed_llms_example_amd.cli import build_models
    torch.manual_seed(0)
    m, t = build_models(_args(model_ckpt="t5-tiny"), resolve_config("t5-tiny"))
    assert t is None and m.config.num_layers == resolve_config("t5-tiny").num_layers
