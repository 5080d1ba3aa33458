"""FusedAdafactor on the CPU: its torch composite (``_reference_step``) against ``transformers.optimization.Adafactor``
on the real parameter structure of our models, the unit rule for fused parameters, state handling and the plumbing
(TrainEngine, Trainer, the command line, LoRA).

Parity bound: ``atol=1e-6, rtol=1e-5`` on every weight, the bound ``test_fused_adamw_reference_matches_torch_with_clip``
uses (both sides are the same fp32 recurrence in another operation order)."""
import copy
import os
import subprocess
import sys

import pytest
import torch

from distributed_llms_example_amd.models import build_model, to_hf_state_dict
from distributed_llms_example_amd.models.hf_io import hf_param_names
from distributed_llms_example_amd.ops.optim import FusedAdafactor, FusedAdamW
from distributed_llms_example_amd.parallel.flat import FlatParams
from hf_oracle import hf_model_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ["t5-tiny", "t5-tiny-gated", "bart-tiny"]
MODES = {
    "trainer": dict(lr=1e-2, scale_parameter=False, relative_step=False),
    "scale_decay": dict(lr=1e-2, scale_parameter=True, relative_step=False, weight_decay=0.1),
    "relative": dict(lr=None, scale_parameter=True, relative_step=True),
    "warmup_init": dict(lr=None, scale_parameter=True, relative_step=True, warmup_init=True),
}
ATOL, RTOL = 1e-6, 1e-5


@pytest.fixture(autouse=True)
def _own_process_env(monkeypatch):
    """Each test starts without a cached process environment, so ``init_distributed(cpu=True)`` builds the CPU one even
    when GPU tests of the same run have cached a cuda one (the fixture of tests/test_training_cpu.py)."""
    from distributed_llms_example_amd.parallel import env as env_mod
    monkeypatch.setattr(env_mod, "_ENV", None)


class _GradView:
    """The gradients of a model under its parameter names: ``to_hf_state_dict`` then splits them like the weights."""

    def __init__(self, m):
        self.config = m.config
        self._m = m

    def state_dict(self):
        return {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in self._m.named_parameters()}


def _batch(vocab, seed, B=3, S=13, T=7):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    am[1, 9:] = 0
    return ids, am, torch.randint(3, vocab, (B, T), generator=g)


def _parts(cfg):
    return lambda n: len(hf_param_names(cfg, n))


def _run_pair(name, mode, steps=4, parts="hf", max_grad_norm=None):
    """``steps`` steps of ours and of transformers' Adafactor on identical gradients (computed by OUR model each step
    and copied into the transformers parameters through the name mapping).  Returns (ours as a transformers state dict,
    the transformers state dict, the two lists of returned gradient norms)."""
    from transformers.optimization import Adafactor
    torch.manual_seed(0)
    ours = build_model(name).train()
    for mod in ours.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    hf = hf_model_for(ours)
    if hasattr(ours, "lm_head") and hf.lm_head.weight is hf.get_input_embeddings().weight:
        # our config unties the LM head; a transformers model that tied it anyway gets its own parameter back (only the
        # parameters are used here, as the containers the transformers optimizer updates)
        hf.lm_head.weight = torch.nn.Parameter(ours.lm_head.weight.detach().clone())
        with torch.no_grad():
            hf.get_input_embeddings().weight.copy_(ours.shared.weight)
    flat = FlatParams(ours)
    kw = dict(MODES[mode])
    opt = FusedAdafactor(flat, parts=_parts(ours.config) if parts == "hf" else parts, **kw)
    ref = Adafactor(hf.parameters(), **kw)
    norms, ref_norms = [], []
    for s in range(steps):
        ids, am, lab = _batch(ours.config.vocab_size, s)
        flat.reset_pending()
        ours(input_ids=ids, attention_mask=am, labels=lab).loss.backward()
        mapped = to_hf_state_dict(_GradView(ours))
        for n, p in hf.named_parameters():
            p.grad = mapped[n].detach().clone().to(p.dtype)
        if max_grad_norm is not None:
            ref_norms.append(torch.nn.utils.clip_grad_norm_(hf.parameters(), max_grad_norm))
        norms.append(opt.step(max_grad_norm=max_grad_norm))
        opt.zero_grad()
        ref.step()
    return to_hf_state_dict(ours), hf.state_dict(), norms, ref_norms


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", MODELS)
def test_matches_transformers_adafactor(name, mode):
    got, ref, _, _ = _run_pair(name, mode)
    assert len(got) > 10
    for k, v in got.items():
        torch.testing.assert_close(v, ref[k], atol=ATOL, rtol=RTOL, msg=lambda m: f"{k}: {m}")


def test_unit_rule_is_load_bearing():
    """With every flat segment as ONE unit, a fused q/k/v shares one clip and one column statistic: the fused weights
    then differ from transformers' beyond the parity bound, while parameters that are not fused still match."""
    got, ref, _, _ = _run_pair("t5-tiny", "trainer", parts=lambda n: 1)
    fused = [k for k in got if ".SelfAttention.q." in k or ".SelfAttention.k." in k or ".SelfAttention.v." in k]
    assert fused
    far = [k for k in fused if not torch.allclose(got[k], ref[k], atol=ATOL, rtol=RTOL)]
    assert far, "stacked q/k/v as one unit still matched transformers"
    plain = [k for k in got if k.endswith(".o.weight") or k.endswith("layer_norm.weight")]
    assert plain
    for k in plain:
        torch.testing.assert_close(got[k], ref[k], atol=ATOL, rtol=RTOL)


def test_clipping_composes_with_the_step():
    got, ref, norms, ref_norms = _run_pair("t5-tiny", "trainer", steps=3, max_grad_norm=0.05)
    for a, b in zip(norms, ref_norms):
        assert float(a) > 0.05  # the clip is active
        assert float(a) == pytest.approx(float(b), rel=1e-5)
    for k, v in got.items():
        torch.testing.assert_close(v, ref[k], atol=ATOL, rtol=RTOL)


def test_beta1_and_option_conflicts_raise():
    flat = FlatParams(build_model("t5-tiny"))
    with pytest.raises(ValueError, match="beta1"):
        FusedAdafactor(flat, lr=1e-3, relative_step=False, beta1=0.9)
    with pytest.raises(ValueError, match="relative_step"):
        FusedAdafactor(flat, lr=1e-3, relative_step=True)
    with pytest.raises(ValueError, match="warmup_init"):
        FusedAdafactor(flat, lr=1e-3, relative_step=False, warmup_init=True)


@pytest.mark.parametrize("name", MODELS)
def test_state_bytes_closed_form(name):
    m = build_model(name)
    flat = FlatParams(m)
    opt = FusedAdafactor(flat, lr=1e-3, relative_step=False, parts=_parts(m.config), master_weights=True)
    want = 0
    for s in flat.segments:
        k = len(hf_param_names(m.config, s.name))
        if len(s.shape) == 2:
            want += k * (s.shape[0] // k + s.shape[1]) * 4
        else:
            want += s.numel * 4
    assert any(len(hf_param_names(m.config, s.name)) > 1 for s in flat.segments)
    assert opt.state_bytes() == want + flat.numel * 4
    adamw = 2 * flat.numel * 4 + flat.numel * 4
    assert opt.state_bytes() < 0.45 * adamw  # no per-parameter moments


def _set_grads(model, seed):
    for i, (n, p) in enumerate(sorted(model.named_parameters())):
        g = torch.Generator().manual_seed(1000 * seed + i)
        p._dllm_gbuf.copy_(torch.randn(p.shape, generator=g) * 1e-2)


def test_state_dict_round_trip_after_relayout():
    torch.manual_seed(0)
    m1 = build_model("t5-tiny-gated")
    m2 = copy.deepcopy(m1)
    f1 = FlatParams(m1)
    o1 = FusedAdafactor(f1, lr=1e-2, relative_step=False, weight_decay=0.1, parts=_parts(m1.config),
                        master_weights=True)
    g = torch.Generator().manual_seed(5)
    f1.relayout(torch.randperm(len(f1.segments), generator=g).tolist())
    assert [s.name for s in f1.segments] != f1.canonical
    for s in range(2):
        _set_grads(m1, s)
        o1.step()  # no global-norm clip: its reduction order follows the layout, the per-unit state does not
    sd = copy.deepcopy(o1.state_dict())
    assert sd["kind"] == "adafactor" and sd["step"] == 2
    m2.load_state_dict(m1.state_dict())
    f2 = FlatParams(m2)
    o2 = FusedAdafactor(f2, lr=1e-2, relative_step=False, weight_decay=0.1, parts=_parts(m2.config),
                        master_weights=True)
    o2.load_state_dict(sd)
    assert o2.step_count == 2
    for o, m in ((o1, m1), (o2, m2)):
        _set_grads(m, 7)
        o.step()
    for (n, a), (_, b) in zip(sorted(m1.named_parameters()), sorted(m2.named_parameters())):
        assert torch.equal(a, b), n
    s1, s2 = o1.state_dict(), o2.state_dict()
    for k in ("R", "C", "V", "master"):
        assert torch.equal(s1[k], s2[k]), k
    bad = dict(sd, layout=sd["layout"][:-1])
    with pytest.raises(ValueError, match="layout"):
        o2.load_state_dict(bad)


def test_state_of_the_other_optimizer_raises():
    flat = FlatParams(build_model("t5-tiny"))
    ada = FusedAdafactor(flat, lr=1e-3, relative_step=False)
    adamw = FusedAdamW(flat, lr=1e-3)
    with pytest.raises(ValueError, match="adamw"):
        ada.load_state_dict(adamw.state_dict())
    with pytest.raises(ValueError, match="adafactor"):
        adamw.load_state_dict(ada.state_dict())


def test_trainer_resume_is_exact_with_adafactor(tmp_path):
    """Train 6 steps straight vs 3 + resume-from-checkpoint + 3 with ``optim="adafactor"``: identical weights (the
    method of test_trainer_resume_is_exact)."""
    from distributed_llms_example_amd.data.collator import DataCollatorForSeq2Seq
    from distributed_llms_example_amd.data.dataset import SyntheticSeq2Seq
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.trainer import Trainer, TrainingArguments
    env = init_distributed(cpu=True)
    ds = SyntheticSeq2Seq(24, 12, 6, 500, seed=1)
    coll = DataCollatorForSeq2Seq(0, 0)

    def make(out, max_steps, save_steps):
        torch.manual_seed(0)
        m = build_model("t5-tiny")
        args = TrainingArguments(output_dir=str(out), max_steps=max_steps, per_device_train_batch_size=4,
                                 learning_rate=1e-3, warmup_steps=2, logging_steps=100, save_steps=save_steps,
                                 bf16=False, seed=3, optim="adafactor")
        return Trainer(m, args, train_dataset=ds, data_collator=coll, env=env)

    t1 = make(tmp_path / "a", 6, 1000)
    assert isinstance(t1.engine.optimizer, FusedAdafactor)
    assert not t1.engine.optimizer.scale_parameter and not t1.engine.optimizer.relative_step
    assert sum(u["name"].endswith("qkv.weight") for u in t1.engine.optimizer.units) % 3 == 0
    t1.train()
    t2 = make(tmp_path / "b", 3, 3)
    t2.train()
    t3 = make(tmp_path / "b", 6, 1000)
    t3.train(resume_from_checkpoint=str(tmp_path / "b" / "checkpoint-3"))
    assert t3.state.global_step == 6
    torch.testing.assert_close(t1.engine.flat.param_buf, t3.engine.flat.param_buf, atol=1e-6, rtol=1e-5)
    with pytest.raises(ValueError, match="optim"):
        TrainingArguments(optim="sgd")


def _cli(tmp, *extra):
    env = dict(os.environ)
    env.update({"VH_ROOT": str(tmp), "DLLM_FORCE_CPU": "1", "OMP_NUM_THREADS": "2", "PYTHONPATH": ROOT})
    return subprocess.run([sys.executable, os.path.join(ROOT, "train-torchrun.py"), "--model-ckpt", "t5-tiny",
                           "--output-dir", "out", "--batch-size", "4", "--grad-accum", "1", "--synthetic", "32",
                           "--max-source-length", "40", "--max-target-length", "10", "--gen-max-length", "8",
                           "--warmup-steps", "1", *extra], env=env, capture_output=True, text=True, timeout=300)


def test_command_line_adafactor(tmp_path):
    import json
    r = _cli(tmp_path, "--optim", "adafactor", "--learning-rate", "1e-2", "--num-epochs", "4", "--evaluation-steps", "8")
    assert r.returncode == 0, r.stderr[-3000:]
    evals = []
    for line in r.stdout.splitlines():
        if line.strip().startswith("{"):
            try:
                d = json.loads(line)
            except json.JSONDecodeError:
                continue
            if "eval_loss" in d:
                evals.append(d["eval_loss"])
    assert len(evals) >= 2 and evals[-1] < evals[0], evals
    bad = _cli(tmp_path, "--optim", "lion")
    assert bad.returncode == 2 and "--optim" in bad.stderr


def test_lora_with_adafactor():
    """Adapters only in the flat buffers: every unit is an adapter matrix, the base stays frozen, the loss falls."""
    from distributed_llms_example_amd.models.lora import LoraConfig, apply_lora
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    torch.manual_seed(0)
    m = build_model("t5-tiny")
    base = {n: p.detach().clone() for n, p in m.named_parameters()}
    apply_lora(m, LoraConfig(r=4, alpha=8, targets=("q", "v", "wi")))
    eng = TrainEngine(m, init_distributed(cpu=True), lr=2e-2, dtype=torch.float32, optim="adafactor")
    opt = eng.optimizer
    assert isinstance(opt, FusedAdafactor) and len(opt.units) == len(eng.flat.segments)
    assert all(u["factored"] for u in opt.units)
    eng.train()
    ids, am, lab = _batch(m.config.vocab_size, 0)
    losses = []
    for _ in range(6):
        losses.append(float(eng.forward_backward({"input_ids": ids, "attention_mask": am, "labels": lab})))
        eng.step()
    assert losses[-1] < losses[0]
    now = dict(m.named_parameters())
    for n, p in base.items():
        if n in now and not now[n].requires_grad:
            assert torch.equal(now[n], p), n


def test_accelerator_maps_transformers_adafactor():
    """``Accelerator.prepare`` turns a transformers Adafactor into FusedAdafactor with its group options and the unit
    rule of the model's config."""
    from transformers.optimization import Adafactor
    from distributed_llms_example_amd.train.accelerator import Accelerator
    acc = Accelerator(cpu=True, mixed_precision="no")
    m = build_model("t5-tiny")
    opt = Adafactor(m.parameters(), lr=None, scale_parameter=True, relative_step=True, warmup_init=True,
                    clip_threshold=0.5, decay_rate=-0.7, weight_decay=0.0)
    pm, po = acc.prepare(m, opt)
    f = po.opt
    assert isinstance(f, FusedAdafactor)
    assert (f.relative_step, f.warmup_init, f.scale_parameter) == (True, True, True)
    assert f.clip_threshold == 0.5 and f.decay_rate == -0.7 and f.eps == (1e-30, 1e-3)
    assert len(f.units) > len(pm.flat.segments)  # fused q/k/v split into their transformers parameters
    adamw = acc.prepare_optimizer(torch.optim.AdamW(m.parameters(), lr=1e-3)).opt
    assert isinstance(adamw, FusedAdamW)
