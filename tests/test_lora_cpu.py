"""LoRA on the CPU (fp32 composite): apply / freeze / merge, adapter gradients against the dense statement, the PEFT
checkpoint layout, exact trainer resume, two gloo ranks against one process, the entry point, the error cases."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

from distributed_llms_example_amd.models import build_model, save_pretrained
from distributed_llms_example_amd.models.hf_io import adapter_keys, load_adapter, save_adapter
from distributed_llms_example_amd.models.lora import (LoraConfig, adapted_layers, apply_lora, merge_lora,
                                                      param_counts)
from distributed_llms_example_amd.ops.linear import Linear
from distributed_llms_example_amd.ops.lora import Adapter, lora_linear
from distributed_llms_example_amd.ops.rng import rowwise_keep_mask
from distributed_llms_example_amd.parallel.flat import FlatParams
from test_distributed_cpu import _native_available, run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("q", "k", "v", "o", "wi", "wo")
TINY = ["t5-tiny", "t5-tiny-gated", "bart-tiny", "led-tiny"]


def _batch(V, B=2, S=16, T=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, V, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    am[1, S - 4:] = 0
    return ids, am, torch.randint(3, V, (B, T), generator=g)


def _randomise_b(m, seed=1, std=0.05):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "lora_B_" in n:
                p.copy_(torch.randn(p.shape, generator=g) * std)


# -------------------------------------------------------------------------------------------------------------- apply
@pytest.mark.parametrize("name", TINY)
def test_apply_freezes_base_and_starts_as_the_base_model(name):
    torch.manual_seed(0)
    m = build_model(name).eval()
    ids, am, lab = _batch(m.config.vocab_size)
    base = m(input_ids=ids, attention_mask=am, labels=lab).loss
    before = {n for n, _ in m.named_parameters()}
    apply_lora(m, LoraConfig(r=4, alpha=8, targets=ALL))
    for n, p in m.named_parameters():
        assert p.requires_grad == ("lora_" in n), n
    assert {n for n, _ in m.named_parameters() if "lora_" not in n} == before
    # B = 0: the adapted model IS the base model
    assert torch.equal(m(input_ids=ids, attention_mask=am, labels=lab).loss, base)
    flat = FlatParams(m)
    assert flat.segments and all("lora_" in s.name for s in flat.segments)
    train, total = param_counts(m)
    assert train == sum(s.numel for s in flat.segments) and 0 < train < total // 5
    m.train()
    m(input_ids=ids, attention_mask=am, labels=lab).loss.backward()
    assert flat.grad_buf.abs().sum() > 0
    assert all(p.grad is None for n, p in m.named_parameters() if "lora_" not in n)


def test_targets_and_slices_on_fused_projections():
    m = build_model("t5-tiny-gated")
    cfg = m.config
    apply_lora(m, LoraConfig(r=2, targets=("q", "v", "wi")))
    layers = dict(adapted_layers(m))
    qkv = layers["encoder.block.0.layer.0.SelfAttention.qkv"]._lora[0]
    inner = cfg.inner_dim
    assert [(a.name, a.c0, a.n) for a in qkv] == [("q", 0, inner), ("v", 2 * inner, inner)]
    kv = layers["decoder.block.0.layer.1.EncDecAttention.kv"]._lora[0]
    assert [(a.name, a.c0, a.n) for a in kv] == [("v", inner, inner)]
    assert [(a.name, a.c0) for a in layers["decoder.block.0.layer.1.EncDecAttention.q"]._lora[0]] == [("q", 0)]
    wi = layers["encoder.block.0.layer.1.DenseReluDense.wi"]._lora[0]
    assert [(a.c0, a.n) for a in wi] == [(0, cfg.d_ff), (cfg.d_ff, cfg.d_ff)]  # a gated wi adapts both halves
    assert not any(n.endswith(".o") or n.endswith(".wo") for n in layers)
    a = qkv[0]
    assert a.A.shape == (2, cfg.d_model) and a.B.shape == (inner, 2) and a.scale == 8.0
    assert a.B.abs().sum() == 0 and a.A.abs().max() <= (1.0 / cfg.d_model) ** 0.5 + 1e-6  # Kaiming-uniform, a = sqrt(5)


def test_led_global_projections_and_heads_are_never_adapted():
    m = build_model("led-tiny")
    apply_lora(m, LoraConfig(r=2, targets=ALL))
    names = [n for n, _ in adapted_layers(m)]
    assert names and not any("q_global" in n or "kv_global" in n or "lm_head" in n for n in names)
    assert not any("lora_" in n for n, _ in m.named_parameters()
                   if "embed" in n or "shared" in n or "norm" in n.lower())
    m2 = build_model("bart-tiny")
    apply_lora(m2, LoraConfig(r=2, targets=("wi", "wo")))
    assert {n.rsplit(".", 1)[-1] for n, _ in adapted_layers(m2)} == {"fc1", "fc2"}


# -------------------------------------------------------------------------------------------------------------- errors
def test_errors():
    with pytest.raises(ValueError, match="unknown LoRA targets.*known: q, k, v, o, wi, wo"):
        LoraConfig(targets=("q", "value"))
    m = build_model("t5-tiny")
    apply_lora(m, LoraConfig(r=2))
    with pytest.raises(RuntimeError, match="already carries adapters"):
        apply_lora(m, LoraConfig(r=2))
    m2 = build_model("t5-tiny")
    FlatParams(m2)
    with pytest.raises(RuntimeError, match="before TrainEngine / FlatParams"):
        apply_lora(m2, LoraConfig(r=2))
    with pytest.raises(RuntimeError, match="no adapters"):
        merge_lora(build_model("t5-tiny"))
    with pytest.raises(RuntimeError, match="no adapters"):
        save_adapter(build_model("t5-tiny"), "unused")
    lin = Linear(8, 8)
    ad = Adapter("q", 0, 8, torch.nn.Parameter(torch.zeros(2, 8)), torch.nn.Parameter(torch.zeros(8, 2)), 1.0)
    with pytest.raises(NotImplementedError, match="frozen base"):
        lora_linear(torch.zeros(3, 8), lin, [ad])


# ----------------------------------------------------------------------------------------------------------- gradients
def _dense(x, W, bias, ads, keep, p):
    """The dense statement: y = x Wᵀ + b, plus scale · (keep ⊙ x / (1 - p)) Aᵀ Bᵀ on each adapter's column slice."""
    y = x @ W.t() + (bias if bias is not None else 0)
    xd = x if keep is None else x * keep / (1.0 - p)
    parts = []
    for c0 in range(0, W.shape[0], ads[0][2]):
        hit = [a for a in ads if a[1] == c0]
        ys = y[:, c0:c0 + ads[0][2]]
        for A, _, n, B, s in hit:
            ys = ys + s * (xd @ A.t()) @ B.t()
        parts.append(ys)
    return torch.cat(parts, 1)


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("case", ["qkv_slices_0_2", "kv_slice_1", "gated_wi", "biased_full"])
def test_adapter_gradients_match_the_dense_statement(case, p):
    """Through the op (fp64: the comparison measures the formulas, not rounding): p = 0 against autograd on
    x (W + s · B_slice A)ᵀ, p > 0 against the same with the explicit ``rowwise_keep_mask``."""
    torch.manual_seed(0)
    K, n, r, N = 24, 16, 3, 10
    nsl, which = {"qkv_slices_0_2": (3, (0, 2)), "kv_slice_1": (2, (1,)), "gated_wi": (2, (0, 1)),
                  "biased_full": (1, (0,))}[case]
    lin = Linear(K, nsl * n, bias=case == "biased_full").double()
    for q in lin.parameters():
        q.requires_grad_(False)
    ads = []
    for i in which:
        A = torch.nn.Parameter(torch.randn(r, K, dtype=torch.float64))
        B = torch.nn.Parameter(torch.randn(n, r, dtype=torch.float64))
        ads.append(Adapter("x", i * n, n, A, B, 0.5 + i))
    x = torch.randn(2, N // 2, K, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(2, N // 2, nsl * n, dtype=torch.float64)
    seed = 4242
    y = lora_linear(x, lin, ads, p, seed)
    got = torch.autograd.grad(y, [x] + [q for a in ads for q in (a.A, a.B)], gy)
    keep = rowwise_keep_mask(seed, p, N, K, "cpu").double() if p > 0 else None
    x2 = x.detach().reshape(N, K).requires_grad_(True)
    ref_y = _dense(x2, lin.weight, lin.bias, [(a.A, a.c0, a.n, a.B, a.scale) for a in ads], keep, p)
    ref = torch.autograd.grad(ref_y, [x2] + [q for a in ads for q in (a.A, a.B)], gy.reshape(N, -1))
    torch.testing.assert_close(y.reshape(N, -1), ref_y, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(got[0].reshape(N, K), ref[0], atol=1e-12, rtol=1e-12)
    for g, e in zip(got[1:], ref[1:]):
        torch.testing.assert_close(g, e, atol=1e-12, rtol=1e-12)
    if p == 0.0:  # the merged weight: x (W + s · B A)ᵀ
        W = lin.weight.detach().clone()
        for a in ads:
            W[a.c0:a.c0 + a.n] += a.scale * (a.B.detach() @ a.A.detach())
        torch.testing.assert_close(y.reshape(N, -1), x2.detach() @ W.t() + (lin.bias if lin.bias is not None else 0),
                                   atol=1e-12, rtol=1e-12)


def test_flat_buffer_accumulation_equals_autograd():
    """With FlatParams the adapter gradients accumulate into the flat buffer (``_use`` / ``_fire``), over two
    micro-batches, and equal what plain autograd gives without it; the reducer-style post hooks fire once each."""
    res = []
    for flat_on in (True, False):
        torch.manual_seed(0)
        m = build_model("bart-tiny").train()
        apply_lora(m, LoraConfig(r=4, dropout=0.1, targets=ALL))
        _randomise_b(m)
        flat = FlatParams(m) if flat_on else None
        fired = []
        if flat_on:
            for q in flat.params:
                q._dllm_post_hooks = [lambda t, fired=fired: fired.append(id(t))]
        from distributed_llms_example_amd.ops.rng import manual_seed
        manual_seed(3)
        for s in (0, 1):
            ids, am, lab = _batch(m.config.vocab_size, seed=s)
            m(input_ids=ids, attention_mask=am, labels=lab).loss.backward()
        if flat_on:
            assert sorted(fired) == sorted(2 * [id(q) for q in flat.params])
            res.append({s.name: flat.grad_view(i).clone() for i, s in enumerate(flat.segments)})
        else:
            res.append({n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None})
    assert res[0].keys() == res[1].keys()
    for k in res[0]:
        torch.testing.assert_close(res[0][k], res[1][k], atol=1e-6, rtol=1e-5, msg=k)


def test_activation_checkpointing_with_adapters():
    """Recomputed blocks (forward inside backward) do not count as fused uses: same gradients with and without."""
    from distributed_llms_example_amd.ops.rng import manual_seed
    grads = []
    for ckpt in (False, True):
        torch.manual_seed(0)
        m = build_model("t5-tiny").train()
        apply_lora(m, LoraConfig(r=4, dropout=0.1, targets=ALL))
        _randomise_b(m)
        m.gradient_checkpointing_enable(ckpt)
        flat = FlatParams(m)
        manual_seed(9)
        ids, am, lab = _batch(m.config.vocab_size)
        m(input_ids=ids, attention_mask=am, labels=lab).loss.backward()
        grads.append(flat.grad_buf.clone())
        assert all(q._dllm_pending == 0 for q in flat.params)
    torch.testing.assert_close(grads[0], grads[1], atol=1e-7, rtol=1e-5)


# --------------------------------------------------------------------------------------------------------------- merge
def _trained(name, tmp_path=None, steps=4):
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    torch.manual_seed(0)
    m = build_model(name)
    if hasattr(m, "lm_head"):
        with torch.no_grad():
            m.lm_head.weight.copy_(m.shared.weight)
    apply_lora(m, LoraConfig(r=4, alpha=8, targets=ALL))
    eng = TrainEngine(m, init_distributed(cpu=True), lr=2e-2, dtype=torch.float32)
    eng.train()
    for s in range(steps):
        ids, am, lab = _batch(m.config.vocab_size, seed=s)
        eng.forward_backward({"input_ids": ids, "attention_mask": am, "labels": lab})
        eng.step()
    assert all(a.B.abs().sum() > 0 for _, l in adapted_layers(m) for a in l._lora[0])
    return m.eval()


@pytest.mark.parametrize("name", ["t5-tiny", "t5-tiny-gated", "bart-tiny"])
def test_merge_reproduces_the_adapted_model(name, tmp_path):
    """A few AdamW steps in fp32, then ``merge_lora``: the merged model's logits match the adapted model's.

    Margin: x (W + s·B A)ᵀ and x Wᵀ + s·(x Aᵀ) Bᵀ differ by reassociation.  The composite's own reassociation error
    is measured as the distance between its fp32 logits and the same adapted model evaluated in fp64 (same weights);
    the merged model gets one order of magnitude over that.  Measured here: composite fp32-vs-fp64 error 1.41e-6
    (t5-tiny), 1.71e-5 (t5-tiny-gated), 2.7e-7 (bart-tiny); merged-vs-adapted distance 1.79e-6, 2.1e-5, 2.38e-7.

    The merged checkpoint then loads in transformers and reproduces the logits to the tolerance
    tests/test_model_parity.py uses (atol 2e-5, rtol 1e-4)."""
    import copy

    import transformers
    m = _trained(name)
    ids, am, lab = _batch(m.config.vocab_size, seed=11)
    with torch.no_grad():
        adapted = m(input_ids=ids, attention_mask=am, labels=lab, return_logits=True).logits
        adapted64 = copy.deepcopy(m).double()(input_ids=ids, attention_mask=am, labels=lab, return_logits=True).logits
    reassoc = (adapted.double() - adapted64).abs().max().item()
    before = {n for n, _ in m.named_parameters() if "lora_" not in n}
    merge_lora(m)
    assert {n for n, _ in m.named_parameters()} == before and not adapted_layers(m)
    with torch.no_grad():
        merged = m(input_ids=ids, attention_mask=am, labels=lab, return_logits=True).logits
    dist = (merged - adapted).abs().max().item()
    print(f"[merge {name}] composite fp32-vs-fp64 {reassoc:.3g}, merged-vs-adapted {dist:.3g}")
    assert reassoc > 0 and dist <= 10 * reassoc, (dist, reassoc)
    save_pretrained(m, str(tmp_path))
    assert not os.path.exists(tmp_path / "adapter_model.safetensors")
    hf = transformers.AutoModelForSeq2SeqLM.from_pretrained(str(tmp_path), attn_implementation="eager").eval()
    with torch.no_grad():
        ref = hf(input_ids=ids, attention_mask=am, labels=lab).logits
    torch.testing.assert_close(merged, ref, atol=2e-5, rtol=1e-4)


def test_merge_restores_trainability():
    m = build_model("t5-tiny")
    names = {n for n, p in m.named_parameters() if p.requires_grad}
    apply_lora(m, LoraConfig(r=2))
    merge_lora(m)
    assert {n for n, p in m.named_parameters() if p.requires_grad} == names
    apply_lora(m, LoraConfig(r=2))  # a merged model can be adapted again


# ---------------------------------------------------------------------------------------------------------- checkpoint
@pytest.mark.parametrize("name", TINY)
def test_adapter_checkpoint_layout_and_round_trip(name, tmp_path):
    from safetensors.torch import load_file
    torch.manual_seed(0)
    m = build_model(name)
    apply_lora(m, LoraConfig(r=4, alpha=12, dropout=0.05, targets=("q", "v", "wi")))
    _randomise_b(m)
    assert sorted(save_adapter(m, str(tmp_path))) == ["adapter_config.json", "adapter_model.safetensors"]
    conf = json.load(open(tmp_path / "adapter_config.json"))
    assert conf["peft_type"] == "LORA" and conf["task_type"] == "SEQ_2_SEQ_LM"
    assert conf["r"] == 4 and conf["lora_alpha"] == 12 and conf["lora_dropout"] == 0.05
    want = {"t5-tiny": ["q", "v", "wi"], "t5-tiny-gated": ["q", "v", "wi_0", "wi_1"],
            "bart-tiny": ["fc1", "q_proj", "v_proj"], "led-tiny": ["fc1", "q_proj", "query", "v_proj", "value"]}[name]
    assert conf["target_modules"] == want
    sd = load_file(str(tmp_path / "adapter_model.safetensors"))
    assert all(k.startswith("base_model.model.") and k.endswith((".lora_A.weight", ".lora_B.weight")) for k in sd)
    first = {"t5-tiny": "encoder.block.0.layer.0.SelfAttention.q", "t5-tiny-gated": "encoder.block.0.layer.0.SelfAttention.q",
             "bart-tiny": "model.encoder.layers.0.self_attn.q_proj",
             "led-tiny": "led.encoder.layers.0.self_attn.longformer_self_attn.query"}[name]
    assert sd[f"base_model.model.{first}.lora_A.weight"].shape == (4, m.config.d_model)
    assert sd[f"base_model.model.{first}.lora_B.weight"].shape[1] == 4
    # the HF module paths are those of the unfused projections of the base checkpoint
    from distributed_llms_example_amd.models import to_hf_state_dict
    hf_keys = set(to_hf_state_dict(m))
    assert not any("lora_" in k for k in hf_keys)
    for k in sd:
        assert k[len("base_model.model."):].rsplit(".lora_", 1)[0] + ".weight" in hf_keys, k
    # round trip, bit for bit: into a model that has adapters, and into a plain one (adapters built from the config)
    torch.manual_seed(5)
    m2 = build_model(name)
    apply_lora(m2, LoraConfig(r=4, alpha=12, dropout=0.05, targets=("q", "v", "wi")))
    m3 = build_model(name)
    for other in (load_adapter(m2, str(tmp_path)), load_adapter(m3, str(tmp_path))):
        keys, mine = adapter_keys(other), adapter_keys(m)
        assert keys.keys() == mine.keys() == sd.keys()
        for k in mine:
            assert torch.equal(keys[k], mine[k]), k
    assert m3._lora_cfg == LoraConfig(r=4, alpha=12, dropout=0.05, targets=("q", "v", "wi"))


def test_trainer_resume_with_adapters_is_exact(tmp_path):
    """6 steps straight vs 3 + resume + 3 (the tests/test_training_cpu.py pattern): identical adapters; the optimizer
    state covers the adapters only."""
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
        apply_lora(m, LoraConfig(r=4, dropout=0.1, targets=("q", "v")))
        args = TrainingArguments(output_dir=str(out), max_steps=max_steps, per_device_train_batch_size=4,
                                 learning_rate=1e-2, warmup_steps=2, logging_steps=100, save_steps=save_steps,
                                 bf16=False, seed=3)
        return Trainer(m, args, train_dataset=ds, data_collator=coll, env=env)

    t1 = make(tmp_path / "a", 6, 1000)
    t1.train()
    t2 = make(tmp_path / "b", 3, 3)
    t2.train()
    ck = tmp_path / "b" / "checkpoint-3"
    assert (ck / "adapter_model.safetensors").exists() and (ck / "adapter_config.json").exists()
    state = torch.load(ck / "training_state.pt", map_location="cpu", weights_only=True)
    n_adapter = t2.engine.flat.numel
    assert all("lora_" in s.name for s in t2.engine.flat.segments)
    assert max(v.numel() for v in state["optimizer"].values() if torch.is_tensor(v)) <= n_adapter
    t3 = make(tmp_path / "b", 6, 1000)
    t3.train(resume_from_checkpoint=str(ck))
    assert t3.state.global_step == 6
    assert t1.engine.flat.param_buf.abs().sum() > 0
    torch.testing.assert_close(t1.engine.flat.param_buf, t3.engine.flat.param_buf, atol=1e-6, rtol=1e-5)


# --------------------------------------------------------------------------------------------------------- distributed
def _lora_grad_case(rank, world, native=None):
    from distributed_llms_example_amd.parallel.env import DistEnv
    from distributed_llms_example_amd.train.engine import TrainEngine
    torch.manual_seed(0)
    model = build_model("t5-tiny")
    apply_lora(model, LoraConfig(r=4, targets=ALL))
    _randomise_b(model)
    env = DistEnv(rank=rank, world_size=world, backend="gloo", device=torch.device("cpu"))
    if rank == 1:  # a different adapter init on rank 1: the broadcast must overwrite it
        with torch.no_grad():
            for n, p in model.named_parameters():
                if "lora_" in n:
                    p.add_(1.0)
    os.environ["DLLM_ROUTE"] = "reducer=native" if native else "reducer=python"
    eng = TrainEngine(model, env, lr=1e-3, dtype=torch.float32, bucket_mb=0.01, overlap=True)
    if native:
        assert eng.reducer.native is not None
    eng.train(False)
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(3, 500, (4 * world, 10), generator=g)
    lab = torch.randint(3, 500, (4 * world, 5), generator=g)
    s = slice(rank * 4, rank * 4 + 4)
    eng.forward_backward({"input_ids": ids[s], "attention_mask": torch.ones_like(ids[s]), "labels": lab[s]})
    return (eng.flat.to_canonical(eng.flat.grad_buf).clone(), eng.flat.to_canonical(eng.flat.param_buf).clone(),
            len(eng.reducer.buckets))


@pytest.mark.parametrize("native", [False, pytest.param(True, marks=pytest.mark.skipif(
    not _native_available(), reason="native extension not built"))])
def test_two_ranks_with_adapters_match_single_process(native):
    out = run_ranks(functools.partial(_lora_grad_case, native=native))
    torch.manual_seed(0)
    model = build_model("t5-tiny").eval()
    apply_lora(model, LoraConfig(r=4, targets=ALL))
    _randomise_b(model)
    flat = FlatParams(model)
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(3, 500, (8, 10), generator=g)
    lab = torch.randint(3, 500, (8, 5), generator=g)
    loss = sum(model(input_ids=ids[r * 4:(r + 1) * 4], attention_mask=torch.ones(4, 10, dtype=torch.long),
                     labels=lab[r * 4:(r + 1) * 4]).loss for r in range(2)) / 2
    loss.backward()
    g0, p0, nb = (torch.as_tensor(x) if not isinstance(x, int) else x for x in out[0])
    g1, p1, _ = (torch.as_tensor(x) if not isinstance(x, int) else x for x in out[1])
    assert nb > 1 and g0.numel() == flat.numel
    torch.testing.assert_close(g0, g1)
    torch.testing.assert_close(p0, p1)
    torch.testing.assert_close(p0, flat.param_buf)
    torch.testing.assert_close(g0, flat.grad_buf, atol=1e-5, rtol=1e-4)


# --------------------------------------------------------------------------------------------------------- entry point
def test_train_torchrun_with_lora(tmp_path):
    env = dict(os.environ)
    env.update({"VH_ROOT": str(tmp_path), "DLLM_FORCE_CPU": "1", "OMP_NUM_THREADS": "2", "PYTHONPATH": ROOT})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train-torchrun.py"), "--model-ckpt", "t5-tiny",
                        "--output-dir", "out", "--batch-size", "4", "--grad-accum", "2", "--evaluation-steps", "4",
                        "--warmup-steps", "1", "--lora-r", "4", "--lora-dropout", "0.1", "--lora-targets", "q,v,wo",
                        "--synthetic", "16", "--max-source-length", "40", "--max-target-length", "10",
                        "--gen-max-length", "8"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    logs = [json.loads(l) for l in r.stdout.splitlines() if l.strip().startswith("{")]
    counts = [x for x in logs if "trainable_params" in x]
    assert len(counts) == 1 and 0 < counts[0]["trainable_params"] < counts[0]["total_params"] // 5
    out = tmp_path / "outputs" / "out"
    for f in ("config.json", "model.safetensors", "adapter_config.json", "adapter_model.safetensors",
              "adapter_model.safetensors.metadata.json"):
        assert (out / f).exists(), f
    m = build_model("t5-tiny")
    load_adapter(m, str(out))
    assert m._lora_cfg.targets == ("q", "v", "wo") and m._lora_cfg.r == 4
    assert any(a.B.abs().sum() > 0 for _, l in adapted_layers(m) for a in l._lora[0])  # it trained


def test_flags_off_by_default():
    from distributed_llms_example_amd.cli import base_parser, maybe_apply_lora
    args = base_parser("x").parse_args([])
    assert args.lora_r == 0 and args.lora_targets == "q,v" and args.lora_alpha == 16.0 and args.lora_dropout == 0.0
    m = build_model("t5-tiny")
    assert maybe_apply_lora(m, args) is m and not adapted_layers(m)
    assert all(p.requires_grad for p in m.parameters())
