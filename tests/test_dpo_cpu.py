"""Preference optimisation (DPO / IPO / hinge) on the CPU: the torch composite of the loss against an independent fp64
statement, the models with one encoder row per prompt against the prompt repeated per target row, the collator's
interleaved layout, pair-count normalisation under gradient accumulation, the Trainer entry point, and every loud
error."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_llms_example_amd.models import Preference, build_model, resolve_config
from distributed_llms_example_amd.ops import preference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ("rewards/chosen", "rewards/rejected", "rewards/margins", "rewards/accuracies", "logps/chosen",
         "logps/rejected")


# ------------------------------------------------------------------------------------------------------------ the loss
def _softplus64(z):
    """log(1 + e^z) for a python float, stable."""
    return max(z, 0.0) + math.log1p(math.exp(-abs(z)))


def _statement64(x, r, labels, T, beta, kind, eps, sft):
    """The definition, pair by pair and row by row, in fp64: torch only for log_softmax (autograd through ``x``)."""
    lpx = torch.log_softmax(x.double(), -1)
    lpr = torch.log_softmax(r.double(), -1)
    V = x.shape[1]
    P = x.shape[0] // (2 * T)
    total = 0.0
    stats = {k: 0.0 for k in STATS}
    for i in range(P):
        L, R, n = [], [], []
        for s in (2 * i, 2 * i + 1):
            a = b = 0.0
            k = 0
            for t in range(s * T, (s + 1) * T):
                y = int(labels[t])
                if y != -100 and 0 <= y < V:
                    a = a + lpx[t, y]
                    b = b + float(lpr[t, y])
                    k += 1
            L.append(a), R.append(b), n.append(max(1, k))
        h = beta * ((L[0] - L[1]) - (R[0] - R[1]))
        if kind == "sigmoid":
            sp = torch.nn.functional.softplus
            l = (1 - eps) * sp(-h) + eps * sp(h) if torch.is_tensor(h) else \
                (1 - eps) * _softplus64(-h) + eps * _softplus64(h)
        elif kind == "hinge":
            l = torch.clamp(1 - h, min=0) if torch.is_tensor(h) else max(0.0, 1 - h)
        else:
            hb = (L[0] / n[0] - L[1] / n[1]) - (R[0] / n[0] - R[1] / n[1])
            l = (hb - 1 / (2 * beta)) ** 2
        l = l + sft * (-L[0] / n[0])
        total = total + l
        Lc, Lr = float(torch.as_tensor(L[0]).detach()), float(torch.as_tensor(L[1]).detach())
        rc, rr = beta * (Lc - R[0]), beta * (Lr - R[1])
        for k, v in zip(STATS, (rc, rr, rc - rr, float(rc > rr), Lc, Lr)):
            stats[k] += v / P
    return total / P, stats


def _case(P=3, T=4, V=37, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2 * P * T, V, generator=g) * 2
    r = x + 0.3 * torch.randn(2 * P * T, V, generator=g)
    labels = torch.randint(0, V, (2 * P * T,), generator=g)
    labels[1] = -100
    labels[5] = V      # out of range: not valid
    labels[2 * T:3 * T] = -100  # a fully ignored sequence (pair 1's chosen)
    return x, r, labels


@pytest.mark.parametrize("sft", [0.0, 0.5])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("kind", ["sigmoid", "hinge", "ipo"])
def test_reference_matches_the_fp64_statement(kind, eps, sft):
    T, beta = 4, 0.7
    x, r, labels = _case(T=T)
    x64 = x.double().requires_grad_(True)
    want, wstats = _statement64(x64, r, labels, T, beta, kind, eps, sft)
    want.backward()
    for dt, rtol in ((torch.float64, 1e-12), (torch.float32, 2e-5)):
        xx = x.to(dt).requires_grad_(True)
        loss, stats = PR._reference(xx, r.to(dt), labels, T, None, None, beta, kind, eps, sft)
        loss.backward()
        torch.testing.assert_close(loss.double(), want.detach(), rtol=rtol, atol=rtol)
        torch.testing.assert_close(xx.grad.double(), x64.grad, rtol=rtol * 10, atol=rtol)
        assert set(stats) == set(STATS)
        for k in STATS:
            assert abs(float(stats[k]) - wstats[k]) <= rtol * 10 * max(1.0, abs(wstats[k])), (k, stats[k], wstats[k])
        assert torch.equal(xx.grad[2 * T:3 * T], torch.zeros_like(xx.grad[2 * T:3 * T]))  # the ignored sequence
        assert torch.equal(xx.grad[1], torch.zeros_like(xx.grad[1])) and not xx.grad[0].eq(0).all()


def test_reference_bias_is_added_to_the_logits():
    T, beta = 4, 0.3
    x, r, labels = _case(T=T)
    g = torch.Generator().manual_seed(3)
    b, rb = torch.randn(x.shape[1], generator=g), torch.randn(x.shape[1], generator=g)
    a, _ = PR._reference(x.double(), r.double(), labels, T, b.double(), rb.double(), beta, "sigmoid", 0.0, 0.0)
    w, _ = _statement64(x.double() + b.double(), r.double() + rb.double(), labels, T, beta, "sigmoid", 0.0, 0.0)
    torch.testing.assert_close(a, torch.as_tensor(w), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("kind", ["sigmoid", "hinge", "ipo"])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_h_of_80_is_finite(sign, kind):
    """|h| = 80: exp(80) overflows an fp32 softplus written naively; loss and gradient stay finite and right.  Two
    one-row sequences over V = 2: lp = -log 2 on one, -(800 + log 2) on the other, beta = 0.1, no reference."""
    T, beta = 1, 0.1
    x = torch.zeros(2, 2)
    x[1 if sign > 0 else 0, 0] = 800.0 + math.log(2.0)
    labels = torch.tensor([1, 1])
    x = x.requires_grad_(True)
    loss, stats = PR._reference(x, None, labels, T, None, None, beta, kind, 0.1, 0.0)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(x.grad).all()
    assert abs(float(stats["rewards/margins"]) - sign * 80.0) < 1e-3, stats
    x64 = x.detach().double().requires_grad_(True)
    # uniform reference logits: equal lp_ref on both rows, which cancels in h, as ``ref_logits=None`` (lp_ref = 0)
    want, _ = _statement64(x64, torch.zeros(2, 2), labels, T, beta, kind, 0.1, 0.0)
    want.backward()
    torch.testing.assert_close(loss.double(), want.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(x.grad.double(), x64.grad, rtol=1e-4, atol=1e-7)


def test_validation():
    x, r, labels = _case()
    kw = dict(beta=0.1, kind="sigmoid", label_smoothing=0.0, sft_alpha=0.0)
    with pytest.raises(ValueError, match="beta"):
        PR.preference_loss(x, r, labels, 4, **{**kw, "beta": 0.0})
    with pytest.raises(ValueError, match="smoothing"):
        PR.preference_loss(x, r, labels, 4, **{**kw, "label_smoothing": 0.5})
    with pytest.raises(ValueError, match="kind"):
        PR.preference_loss(x, r, labels, 4, **{**kw, "kind": "kto"})
    with pytest.raises(ValueError, match="2 P T"):
        PR.preference_loss(x, r, labels, 5, **kw)
    with pytest.raises(ValueError, match="shape"):
        PR.preference_loss(x, r[:, :-1], labels, 4, **kw)


def test_route_key():
    from distributed_llms_example_amd.ops import routing
    assert routing.DEFAULTS["pref"] in ("fused", "composite")
    assert "pref=composite" in routing.merged(pref="composite")


# ---------------------------------------------------------------------------------------------------------- the models
# tests/test_longt5_cpu.py's model tolerances
LOSS_TOL = dict(atol=2e-5, rtol=1e-5)
GRAD_TOL = dict(atol=5e-5, rtol=1e-3)


def _pairs(cfg, P=3, S=11, T=6, seed=1):
    g = torch.Generator().manual_seed(seed)
    V = cfg.vocab_size
    b = {"input_ids": torch.randint(3, V, (P, S), generator=g), "attention_mask": torch.ones(P, S, dtype=torch.long),
         "labels": torch.randint(3, V, (2 * P, T), generator=g)}
    b["attention_mask"][1, -3:] = 0
    b["labels"][0, -2:] = -100
    b["labels"][3, -4:] = -100
    return b


@pytest.mark.parametrize("name", ["dpo-tiny", "bart-tiny"])
@pytest.mark.parametrize("kind", ["sigmoid", "ipo"])
def test_shared_encoder_equals_the_encoder_repeated_per_target(name, kind):
    torch.manual_seed(0)
    policy = build_model(name).eval()
    torch.manual_seed(1)
    ref = build_model(name).eval().requires_grad_(False)
    b = _pairs(policy.config)
    rep = {"input_ids": b["input_ids"].repeat_interleave(2, 0),
           "attention_mask": b["attention_mask"].repeat_interleave(2, 0), "labels": b["labels"]}
    got = {}
    for tag, batch in (("shared", b), ("repeated", rep)):
        policy.zero_grad(set_to_none=True)
        with torch.no_grad():
            rh, rw, rb = ref.lm_head_operands(**batch)
        out = policy(**batch, preference=Preference(rh, rw, rb, beta=0.5, kind=kind, sft_alpha=0.25))
        out.loss.backward()
        got[tag] = (out.loss.detach(), {n: p.grad.clone() for n, p in policy.named_parameters()}, out.pref_stats)
        assert set(out.pref_stats) == set(STATS)
    assert all(p.grad is None for p in ref.parameters())  # the reference gets no gradient
    torch.testing.assert_close(got["shared"][0], got["repeated"][0], **LOSS_TOL)
    assert got["shared"][1].keys() == got["repeated"][1].keys() and got["shared"][1]
    for n, g in got["shared"][1].items():
        torch.testing.assert_close(g, got["repeated"][1][n], msg=n, **GRAD_TOL)
    assert sum(float(g.abs().sum()) for g in got["shared"][1].values()) > 0
    assert got["shared"][1][next(n for n in got["shared"][1] if "encoder" in n)].abs().sum() > 0


def test_chunked_cross_attention_keeps_working(monkeypatch):
    """A long encoder output: cross-attention over key chunks (parallel/context.py, forced here by a small
    ``attn_chunk``) with the ``2P`` decoder rows sharing each prompt's K/V gives the unchunked loss and gradients."""
    from distributed_llms_example_amd.ops import routing
    from distributed_llms_example_amd.parallel import context
    torch.manual_seed(0)
    policy = build_model("dpo-tiny").eval()
    torch.manual_seed(1)
    ref = build_model("dpo-tiny").eval().requires_grad_(False)
    b = _pairs(policy.config, P=2, S=300, T=5)
    got = {}
    for tag in ("single", "chunked"):
        if tag == "chunked":
            monkeypatch.setenv("DLLM_ROUTE", routing.merged(attn_chunk=128, attn_chunk_min=128))
            assert context.long_sequence_chunk(300, cross=True) is not None
        policy.zero_grad(set_to_none=True)
        with torch.no_grad():
            rh, rw, rb = ref.lm_head_operands(**b)
        out = policy(**b, preference=Preference(rh, rw, rb, beta=0.5))
        out.loss.backward()
        got[tag] = (out.loss.detach(), {n: p.grad.clone() for n, p in policy.named_parameters()})
    torch.testing.assert_close(got["chunked"][0], got["single"][0], **LOSS_TOL)
    for n, g in got["single"][1].items():
        torch.testing.assert_close(got["chunked"][1][n], g, msg=n, **GRAD_TOL)


def test_model_loss_is_the_composite_on_its_logits():
    torch.manual_seed(0)
    policy = build_model("dpo-tiny").eval()
    torch.manual_seed(1)
    ref = build_model("dpo-tiny").eval()
    b = _pairs(policy.config)
    with torch.no_grad():
        rh, rw, rb = ref.lm_head_operands(**b)
        out = policy(**b, preference=Preference(rh, rw, rb, beta=0.5))
        rep = {k: (v.repeat_interleave(2, 0) if k != "labels" else v) for k, v in b.items()}
        xl = policy(**rep, return_logits=True).logits
        rl = ref(**rep, return_logits=True).logits
    V = xl.shape[-1]
    want, _ = _statement64(xl.view(-1, V), rl.view(-1, V), b["labels"].reshape(-1), b["labels"].shape[1], 0.5,
                           "sigmoid", 0.0, 0.0)
    torch.testing.assert_close(out.loss.double(), torch.as_tensor(want), atol=2e-5, rtol=1e-5)


# -------------------------------------------------------------------------------------------------------- the collator
def test_collator_interleaves_chosen_and_rejected():
    from distributed_llms_example_amd.data.collator import DataCollatorForSeq2Seq
    feats = [{"input_ids": np.array([5, 6, 7]), "attention_mask": np.array([1, 1, 1]),
              "chosen_labels": np.array([11, 12, -100]), "rejected_labels": np.array([21, -100, -100])},
             {"input_ids": np.array([8, 9]), "attention_mask": np.array([1, 1]),
              "chosen_labels": np.array([13]), "rejected_labels": np.array([23, 24, 25, 26])}]
    b = DataCollatorForSeq2Seq(pad_token_id=0, decoder_start_token_id=2)(feats)
    assert b["input_ids"].tolist() == [[5, 6, 7], [8, 9, 0]] and b["attention_mask"].tolist() == [[1, 1, 1], [1, 1, 0]]
    assert b["labels"].tolist() == [[11, 12, -100, -100], [21, -100, -100, -100], [13, -100, -100, -100],
                                    [23, 24, 25, 26]]
    assert b["decoder_input_ids"].tolist() == [[2, 11, 12, 0], [2, 21, 0, 0], [2, 13, 0, 0], [2, 23, 24, 25]]


def test_pair_features_and_synthetic_records():
    from distributed_llms_example_amd.cli import base_parser, build_data, eval_targets, model_config
    a = base_parser("t").parse_args(["--model-ckpt", "dpo-tiny", "--synthetic", "12", "--dpo-beta", "0.1",
                                     "--max-source-length", "24", "--max-target-length", "24"])
    cfg = model_config(a)
    tok, tr, ev = build_data(a, cfg)
    assert len(tr) == 12 and set(tr[0]) == {"input_ids", "attention_mask", "chosen_labels", "rejected_labels"}
    assert tr.records[0].keys() >= {"id", "dialogue", "chosen", "rejected"}
    assert (tr.chosen_labels != tr.rejected_labels).any() and (tr.chosen_labels == -100).any()
    from distributed_llms_example_amd.data.collator import DataCollatorForSeq2Seq
    b = DataCollatorForSeq2Seq.for_model(cfg)([ev[0], ev[1]])
    assert b["labels"].shape[0] == 4 and b["input_ids"].shape[0] == 2
    assert torch.equal(eval_targets(b), b["labels"][0::2])
    assert torch.equal(b["labels"][0], torch.as_tensor(ev.labels[0], dtype=torch.long))  # ROUGE scores the chosen


# ---------------------------------------------------------------------------------------------------------- the engine
def _engine(name="dpo-tiny", train=False, **kw):
    from distributed_llms_example_amd.ops.rng import manual_seed
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    torch.manual_seed(0)
    m = build_model(name)
    torch.manual_seed(1)
    r = build_model(name)
    manual_seed(11)
    eng = TrainEngine(m, init_distributed(cpu=True), lr=1e-2, dtype=torch.float32, reference=r, dpo_beta=0.5, **kw)
    eng.train(train)
    return eng


def test_engine_two_micro_batches_of_2_and_1_pairs_equal_one_batch_of_3():
    from distributed_llms_example_amd.train.engine import pair_count
    one, two = _engine(), _engine()
    big = _pairs(one.model.config, P=3)
    parts = [{"input_ids": big["input_ids"][a:b], "attention_mask": big["attention_mask"][a:b],
              "labels": big["labels"][2 * a:2 * b]} for a, b in ((0, 2), (2, 3))]
    n = one.item_count(big["labels"])
    assert int(n) == 3 and int(pair_count(parts[0]["labels"])) == 2 and int(pair_count(parts[1]["labels"])) == 1
    one.forward_backward(big, num_items=n)
    two.forward_backward(parts[0], grad_accum=2, sync=False, num_items=n)
    two.forward_backward(parts[1], grad_accum=2, sync=True, num_items=n)
    assert one.flat.grad_buf.abs().sum() > 0
    torch.testing.assert_close(two.flat.grad_buf, one.flat.grad_buf, atol=1e-6, rtol=1e-5)
    assert set(one.last_pref_stats) == set(STATS)


def test_engine_keeps_the_reference_frozen_and_outside_the_training_state():
    eng = _engine(train=True)
    before = {k: v.clone() for k, v in eng.reference.state_dict().items()}
    b = _pairs(eng.model.config)
    p0 = eng.flat.param_buf.clone()
    for _ in range(2):
        eng.forward_backward(b)
        eng.step()
    assert not eng.reference.training and not torch.equal(p0, eng.flat.param_buf)
    for k, v in eng.reference.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(p.grad is None and not p.requires_grad for p in eng.reference.parameters())
    assert not {id(p) for p in eng.reference.parameters()} & {id(p) for p in eng.model.parameters()}
    assert eng.flat.numel == sum(p.numel() for p in eng.model.parameters())


def test_engine_composes_with_lora_and_adafactor():
    from distributed_llms_example_amd.cli import base_parser, build_reference, maybe_apply_lora
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    a = base_parser("t").parse_args(["--model-ckpt", "dpo-tiny", "--dpo-beta", "0.2", "--lora-r", "4"])
    torch.manual_seed(0)
    model = build_model("dpo-tiny")
    ref = build_reference(a, model)
    maybe_apply_lora(model, a)
    assert ref is not model and not any("lora" in n.lower() for n, _ in ref.named_parameters())
    eng = TrainEngine(model, init_distributed(cpu=True), lr=1e-2, dtype=torch.float32, reference=ref, dpo_beta=0.2,
                      optim="adafactor")
    eng.train(False)  # no dropout: the policy's forward is the reference's
    b = _pairs(eng.model.config)
    l0 = float(eng.forward_backward(b))
    assert abs(l0 - math.log(2.0)) < 1e-4  # the reference is the policy's copy and the adapters start at zero: h = 0
    eng.train()
    eng.step()
    assert math.isfinite(float(eng.forward_backward(b)))
    assert all(not p.requires_grad for p in eng.reference.parameters())


# ---------------------------------------------------------------------------------------------------------- entry point
def test_train_torchrun_logs_the_six_statistics(tmp_path):
    env = dict(os.environ)
    env.update({"VH_ROOT": str(tmp_path), "DLLM_FORCE_CPU": "1", "OMP_NUM_THREADS": "2", "PYTHONPATH": ROOT})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train-torchrun.py"), "--model-ckpt", "dpo-tiny",
                        "--dpo-beta", "0.1", "--output-dir", "out", "--batch-size", "4", "--grad-accum", "2",
                        "--evaluation-steps", "10", "--warmup-steps", "1", "--synthetic", "80",
                        "--max-source-length", "40", "--max-target-length", "10", "--gen-max-length", "8"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    logs = [json.loads(l) for l in r.stdout.splitlines() if l.strip().startswith("{")]
    tr = [x for x in logs if "rewards/chosen" in x]
    assert tr and all(all(k in x for k in STATS) and "loss" in x for x in tr)
    ev = [x for x in logs if "eval_loss" in x]
    assert ev and all("eval_rewards/accuracies" in x for x in ev)
    from safetensors import safe_open
    with safe_open(str(tmp_path / "outputs" / "out" / "model.safetensors"), "pt") as f:
        keys = list(f.keys())
    assert keys and not any("reference" in k for k in keys)  # the saved model is the policy alone


# --------------------------------------------------------------------------------------------------------------- errors
def _args(*argv):
    from distributed_llms_example_amd.cli import base_parser
    return base_parser("t").parse_args(["--model-ckpt", "dpo-tiny", *argv])


def test_invalid_combinations_raise():
    from distributed_llms_example_amd.cli import build_reference, resolve_preference
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    with pytest.raises(ValueError, match="--teacher-ckpt"):
        resolve_preference(_args("--dpo-beta", "0.1", "--teacher-ckpt", "t5-tiny"))
    with pytest.raises(NotImplementedError, match="--pack-sequences"):
        resolve_preference(_args("--dpo-beta", "0.1", "--pack-sequences"))
    with pytest.raises(NotImplementedError, match="--context-parallel"):
        resolve_preference(_args("--dpo-beta", "0.1", "--context-parallel", "2"))
    with pytest.raises(ValueError, match="--dpo-beta"):
        resolve_preference(_args("--dpo-beta", "0"))
    with pytest.raises(ValueError, match="--dpo-label-smoothing"):
        resolve_preference(_args("--dpo-beta", "0.1", "--dpo-label-smoothing", "0.5"))
    with pytest.raises(ValueError, match="--dpo-beta"):
        resolve_preference(_args("--ref-ckpt", "t5-tiny"))
    assert resolve_preference(_args()).dpo_beta is None  # off by default
    torch.manual_seed(0)
    model = build_model("dpo-tiny")
    with pytest.raises(ValueError, match="vocab_size"):  # --ref-ckpt with another vocabulary than the policy's
        build_reference(_args("--dpo-beta", "0.1", "--ref-ckpt", "t5-tiny"), build_model(
            resolve_config("dpo-tiny").replace(vocab_size=resolve_config("dpo-tiny").vocab_size + 8)))
    with pytest.raises(ValueError, match="vocab_size"):
        TrainEngine(model, init_distributed(cpu=True), dtype=torch.float32, reference=build_model(
            resolve_config("dpo-tiny").replace(vocab_size=resolve_config("dpo-tiny").vocab_size + 8)))
    env = init_distributed(cpu=True)
    with pytest.raises(ValueError, match="teacher"):
        TrainEngine(build_model("dpo-tiny"), env, dtype=torch.float32, teacher=build_model("dpo-tiny"),
                    reference=build_model("dpo-tiny"))
    with pytest.raises(ValueError, match="of its own"):
        TrainEngine(model, env, dtype=torch.float32, reference=model)
    eng = TrainEngine(build_model("dpo-tiny"), env, dtype=torch.float32, reference=build_model("dpo-tiny"))
    b = _pairs(eng.model.config)
    with pytest.raises(ValueError, match=r"\[2P, T\]"):
        eng.forward({**b, "labels": b["labels"][:5]})
    with pytest.raises(ValueError, match="per prompt"):
        eng.forward({**b, "labels": b["labels"][:4]})
