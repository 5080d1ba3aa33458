"""BigBird-Pegasus on the CPU against transformers (eager) with our weights: the block plan against transformers' own
random masks, the composite with that plan against ``BigBirdPegasusBlockSparseAttention``, model parity in train and
eval mode (block-sparse at S = 100, the full-attention rule at S = 60), checkpoint and config.json round trips,
generation, what the family does not implement, and an entry-point smoke.

transformers pads the input to a multiple of the block size and computes five row groups with gathered key blocks; on
every valid query row that equals one softmax over the keys of the listed blocks, a block listed twice counting twice
(models/bigbird.py).  Its padded query rows are not ours, so encoder states are compared at valid positions only;
logits, loss and gradients never see those rows.  Tolerances are those of tests/test_longt5_cpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_llms_example_amd.models import (PRESETS, Seq2SeqConfig, build_model, from_pretrained, resolve_config,
                                                 save_pretrained, to_hf_state_dict)
from distributed_llms_example_amd.models import bigbird
from distributed_llms_example_amd.ops import attention as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TIED = {"model.encoder.embed_tokens.weight", "model.decoder.embed_tokens.weight", "lm_head.weight"}


# ------------------------------------------------------------------------------------------------------- the plan
def _hf_attention(block, r, heads, seed, training, maxpos, d_model=None):
    import transformers
    from transformers.models.bigbird_pegasus.modeling_bigbird_pegasus import BigBirdPegasusBlockSparseAttention
    cfg = transformers.BigBirdPegasusConfig(d_model=d_model or heads * 8, encoder_attention_heads=heads,
                                            block_size=block, num_random_blocks=r, max_position_embeddings=maxpos,
                                            use_bias=False)
    return BigBirdPegasusBlockSparseAttention(cfg, seed=seed).train(training)


def _hf_rand(padded, block, r, heads, seed, training, maxpos):
    """transformers' random blocks [heads, n - 2, r], drawn as bigbird_block_sparse_attention draws them."""
    m = _hf_attention(block, r, heads, seed, training, maxpos)
    np.random.seed(seed)
    if padded in (1024, 3072, 4096):
        ra = [m._bigbird_block_rand_mask(maxpos, maxpos, block, block, r, last_idx=1024)[:padded // block - 2]
              for _ in range(heads)]
    else:
        plan_len, plan_r = m._get_rand_attn_plan(padded, block, r)
        ra = m._bigbird_block_rand_mask_with_head(from_seq_length=padded, to_seq_length=padded, from_block_size=block,
                                                  to_block_size=block, num_heads=heads, plan_from_length=plan_len,
                                                  plan_num_rand_blocks=plan_r)
    return np.stack(ra, axis=0)


PLAN_CASES = ([(64, 3, L, 4096) for L in (768, 832, 1024, 2048, 3072, 4096)]
              + [(8, 1, L, 256) for L in (64, 96, 104)] + [(8, 2, L, 256) for L in (80, 96, 104)]
              + [(8, 3, L, 256) for L in (96, 104, 120)])


@pytest.mark.parametrize("block,r,padded,maxpos", PLAN_CASES)
@pytest.mark.parametrize("training", [True, False])
def test_plan_equals_transformers(block, r, padded, maxpos, training):
    heads = 4
    for seed in range(4):
        want = _hf_rand(padded, block, r, heads, seed, training, maxpos)
        np.random.seed(12345)
        state = np.random.get_state()
        for seq_len in (padded, padded - block + 1):  # the plan is decided on the padded length
            got = bigbird.bigbird_rand_blocks(seq_len, block, r, heads, seed, training, maxpos)
            assert got.shape == want.shape and np.array_equal(got, want), (seed, seq_len)
        after = np.random.get_state()
        assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
        n = padded // block
        plan = bigbird.bigbird_plan(padded, block, r, heads, seed, training, maxpos)
        assert len(plan) == heads and all(len(rows) == n for rows in plan)
        for h in range(heads):
            assert plan[h][0] == list(range(n)) and plan[h][n - 1] == list(range(n))
            assert plan[h][1] == [0, 1, 2, n - 1] + want[h, 0].tolist()
            assert plan[h][n - 2] == [0, n - 3, n - 2, n - 1] + want[h, n - 3].tolist()
            for i in range(2, n - 2):
                assert plan[h][i] == [0, i - 1, i, i + 1] + want[h, i - 1].tolist() + [n - 1]


def test_repeats_are_real():
    """Eval mode repeats block 0 in every sliding row; the old plan at 1024 repeats in training too."""
    ev = bigbird.bigbird_plan(832, 64, 3, 2, 0, False)
    assert all(row.count(0) == 4 for row in ev[0][1:-1])
    tr = bigbird.bigbird_plan(1024, 64, 3, 2, 0, True)
    assert sum(len(row) - len(set(row)) for hd in tr for row in hd[1:-1]) > 0
    with pytest.raises(ValueError, match="at least 5"):
        bigbird.bigbird_plan(32, 8, 1, 1, 0, True)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("S,block,r", [(104, 8, 2), (96, 8, 3), (64, 4, 1)])
def test_composite_with_the_plan_equals_hf_block_sparse_attention(S, block, r, training):
    """transformers' module on a padded batch (row 1 valid up to 70 % of S) against the composite with our plan, on
    the valid rows, in fp64."""
    from transformers.models.bigbird_pegasus.modeling_bigbird_pegasus import BigBirdPegasusEncoder
    torch.manual_seed(S + r)
    heads, D, B, seed = 2, 8, 2, 1
    m = _hf_attention(block, r, heads, seed, training, 256, d_model=heads * D).double()
    x = torch.randn(B, S, heads * D, dtype=torch.float64)
    am = torch.ones(B, S, dtype=torch.float64)
    am[1, int(0.7 * S):] = 0
    blocked, band, frm, to = BigBirdPegasusEncoder.create_masks_for_block_sparse_attn(am, block)
    with torch.no_grad():
        ref, _ = m(x, band, frm, to, blocked, blocked)
        q, k, v = (lin(x).view(B, S, heads, D) for lin in (m.query, m.key, m.value))
    plan = bigbird.bigbird_plan(S, block, r, heads, seed, training, 256)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) / D ** 0.5
    cnt = torch.from_numpy(A.block_lists(plan, block=block).counts()).double()
    cnt = cnt.repeat_interleave(block, 1).repeat_interleave(block, 2)[None] * am[:, None, None, :]
    e = torch.exp(s - s.max(-1, keepdim=True).values) * cnt
    want = torch.einsum("bhqk,bkhd->bqhd", e / e.sum(-1, keepdim=True), v).reshape(B, S, heads * D)
    valid = am.bool()
    assert (want[valid] - ref[valid]).abs().max().item() < 1e-12  # the definition is transformers' computation
    got = A.attention(q.float(), k.float(), v.float(), scale=D ** -0.5, key_padding_mask=valid,
                      block_lists=A.block_lists(plan, block=block)).reshape(B, S, heads * D)
    torch.testing.assert_close(got[valid], ref[valid].float(), atol=2e-6, rtol=1e-5)


# ------------------------------------------------------------------------------------------------------ the model
def _hf_for(model):
    """The transformers model of one of our BigBird-Pegasus configs, with our weights."""
    import transformers
    d = model.config.to_hf_dict()
    assert d.pop("model_type") == "bigbird_pegasus"
    assert d.pop("architectures") == ["BigBirdPegasusForConditionalGeneration"]
    d.pop("torch_dtype")
    hf = transformers.BigBirdPegasusForConditionalGeneration(
        transformers.BigBirdPegasusConfig(**d, attn_implementation="eager"))
    missing, unexpected = hf.load_state_dict(to_hf_state_dict(model), strict=False)
    assert set(missing) <= _TIED, missing  # transformers ties these to `model.shared`
    assert not unexpected, unexpected
    return hf


def _pair(training=False):
    """bigbird-tiny at dropout 0 and a FRESH transformers model (its switch to full attention is sticky)."""
    torch.manual_seed(0)
    cfg = PRESETS["bigbird-tiny"].replace(dropout_rate=0.0, attention_dropout=0.0, activation_dropout=0.0)
    ours = build_model(cfg)
    with torch.no_grad():  # zero-initialised they would not take part
        ours.final_logits_bias.normal_(0.0, 0.5)
        for n, p in ours.named_parameters():
            if n.endswith(".bias"):
                p.normal_(0.0, 0.05)
    return ours.train(training), _hf_for(ours).train(training)


def _batch(V, S, valid1, B=2, T=9, pad_id=0):
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, V, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    am[1, valid1:] = 0
    ids[1, valid1:] = pad_id
    labels = torch.randint(3, V, (B, T), generator=g)
    labels[0, -2:] = -100
    return ids, am, labels


class _GradView:
    def __init__(self, m):
        self.config = m.config
        self._m = m

    def state_dict(self):
        return {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in self._m.named_parameters()}


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("S,valid1", [(100, 70), (60, 45)])
def test_forward_backward_matches_hf(S, valid1, training, monkeypatch):
    """S = 100: 13 blocks of 8 (tail of 4), block-sparse (100 > 72); S = 60: the full-attention rule."""
    ours, hf = _pair(training)
    seen = []
    qkv_call = A.attention_qkv
    monkeypatch.setattr(A, "attention_qkv", lambda qkv, **kw: (
        seen.append((qkv.shape[1], kw.get("block_lists"), kw.get("causal"), kw.get("dropout_p"))), qkv_call(qkv, **kw))[1])
    ids, am, labels = _batch(ours.config.vocab_size, S, valid1)
    out = ours(input_ids=ids, attention_mask=am, labels=labels, return_logits=True)
    enc_calls = [c for c in seen if not c[2]]
    assert len(enc_calls) == ours.config.num_layers
    if S == 100:  # one list call per encoder layer, its own plan each, no dropout on the probabilities
        assert all(c[1] is not None and c[1].block == 8 and c[1].heads == 4 and c[1].nq == 13 for c in enc_calls)
        assert enc_calls[0][1] is not enc_calls[1][1] and all(c[3] == 0.0 for c in enc_calls)
    else:
        assert all(c[1] is None for c in enc_calls)
    ref = hf(input_ids=ids, attention_mask=am, labels=labels)
    torch.testing.assert_close(out.logits, ref.logits, atol=2e-5, rtol=1e-4)
    torch.testing.assert_close(out.loss, ref.loss, atol=2e-5, rtol=1e-5)
    valid = am.bool()
    torch.testing.assert_close(out.encoder_last_hidden_state[valid], ref.encoder_last_hidden_state[valid],
                               atol=2e-5, rtol=1e-4)
    out.loss.backward()
    ref.loss.backward()
    mapped = to_hf_state_dict(_GradView(ours))
    hf_named = dict(hf.named_parameters())
    checked = 0
    for k, g in mapped.items():
        assert k in hf_named, k
        assert hf_named[k].grad is not None, k
        torch.testing.assert_close(g, hf_named[k].grad, atol=5e-5, rtol=1e-3, msg=k)
        checked += 1
    assert checked == len(hf_named)


def test_the_decision_is_per_call():
    """transformers' module stays on full attention after one short input; ours decides per call."""
    ours, hf = _pair()
    V = ours.config.vocab_size
    long_ids, long_am, _ = _batch(V, 100, 70)
    short_ids, short_am, _ = _batch(V, 60, 45)
    a = ours.encode(long_ids, long_am)
    ours.encode(short_ids, short_am)
    assert torch.equal(a, ours.encode(long_ids, long_am))
    full = build_model(ours.config.replace(attention_type="original_full")).eval()
    full.load_state_dict(ours.state_dict())
    assert not torch.equal(a, full.encode(long_ids, long_am))
    assert torch.equal(ours.encode(short_ids, short_am), full.encode(short_ids, short_am))


def test_plans_are_cached_per_layer_length_and_mode():
    bigbird._plans.clear()
    a = bigbird.cached_lists(100, 8, 2, 4, 0, True, 256, "cpu")
    assert bigbird.cached_lists(100, 8, 2, 4, 0, True, 256, "cpu") is a
    assert bigbird.cached_lists(97, 8, 2, 4, 0, True, 256, "cpu") is a  # the same padded length
    assert bigbird.cached_lists(100, 8, 2, 4, 1, True, 256, "cpu") is not a
    assert bigbird.cached_lists(100, 8, 2, 4, 0, False, 256, "cpu") is not a
    assert bigbird.cached_lists(108, 8, 2, 4, 0, True, 256, "cpu") is not a
    assert len(bigbird._plans) == 4


def test_module_names_mirror_hf():
    ours, hf = _pair()
    names = set(to_hf_state_dict(ours))
    for n in range(2):
        for w in ("query", "key", "value"):
            assert f"model.encoder.layers.{n}.self_attn.self.{w}.weight" in names
            assert f"model.encoder.layers.{n}.self_attn.self.{w}.bias" not in names  # use_bias = false
        assert f"model.encoder.layers.{n}.self_attn.output.weight" in names
        for w in ("self_attn_layer_norm", "fc1", "fc2", "final_layer_norm"):
            for t in ("weight", "bias"):
                assert f"model.encoder.layers.{n}.{w}.{t}" in names
        for w in ("q_proj", "k_proj", "v_proj", "out_proj"):
            assert f"model.decoder.layers.{n}.self_attn.{w}.weight" in names
            assert f"model.decoder.layers.{n}.encoder_attn.{w}.weight" in names
    for k in ("model.shared.weight", "model.encoder.embed_positions.weight", "model.decoder.embed_positions.weight",
              "model.encoder.layernorm_embedding.weight", "model.decoder.layernorm_embedding.bias",
              "final_logits_bias"):
        assert k in names
    assert names == set(hf.state_dict()) - _TIED
    assert hf.state_dict()["model.encoder.embed_positions.weight"].shape == (256, 64)
    # the same mapping names the parameters for Adafactor's unit rule and the LoRA adapter paths
    from distributed_llms_example_amd.models.hf_io import hf_param_names
    assert hf_param_names(ours.config, "model.encoder.layers.1.self_attn.qkv_proj.weight") == [
        f"model.encoder.layers.1.self_attn.self.{w}.weight" for w in ("query", "key", "value")]
    assert hf_param_names(ours.config, "model.decoder.layer_norm.weight") == ["model.decoder.layernorm_embedding.weight"]
    assert hf_param_names(ours.config, "model.decoder.layers.0.encoder_attn.kv_proj.weight") == [
        f"model.decoder.layers.0.encoder_attn.{w}.weight" for w in ("k_proj", "v_proj")]


def test_use_bias_switch():
    with_bias = build_model(PRESETS["bigbird-tiny"].replace(use_bias=True))
    assert with_bias.model.encoder.layers[0].self_attn.qkv_proj.bias is not None
    assert f"model.encoder.layers.0.self_attn.self.query.bias" in to_hf_state_dict(with_bias)
    hf = _hf_for(with_bias)
    assert hf.model.encoder.layers[0].self_attn.self.query.bias is not None
    assert build_model("bigbird-tiny").model.decoder.layers[0].encoder_attn.kv_proj.bias is None
    assert build_model("pegasus-tiny").model.encoder.layers[0].self_attn.qkv_proj.bias is not None


NAMES = ["bigbird-tiny", "bigbird-pegasus-large-arxiv", "bigbird-pegasus-large-pubmed", "bigbird-pegasus-large-bigpatent"]


@pytest.mark.parametrize("name", NAMES)
def test_config_round_trip(name, tmp_path):
    cfg = PRESETS[name]
    cfg.save(str(tmp_path))
    with open(os.path.join(tmp_path, "config.json")) as f:
        d = json.load(f)
    assert d["model_type"] == "bigbird_pegasus" and d["architectures"] == ["BigBirdPegasusForConditionalGeneration"]
    assert (d["attention_type"], d["block_size"], d["num_random_blocks"], d["use_bias"]) == (
        "block_sparse", cfg.block_size, cfg.num_random_blocks, False)
    back = resolve_config(str(tmp_path))
    a, b = cfg.to_dict(), back.to_dict()
    for k in a:
        if k not in ("name", "generation"):
            assert a[k] == b[k], k
    for bad in ({"attention_type": "etc"}, {"block_size": 0}):
        with pytest.raises(ValueError, match="BigBird-Pegasus"):
            Seq2SeqConfig.from_hf_dict({**d, **bad})


def test_presets_are_transformers_defaults():
    import transformers
    hf = transformers.BigBirdPegasusConfig()
    for name in NAMES[1:]:
        c = PRESETS[name]
        assert (c.vocab_size, c.d_model, c.num_heads, c.num_layers, c.num_decoder_layers, c.d_ff) == (
            hf.vocab_size, hf.d_model, hf.encoder_attention_heads, hf.encoder_layers, hf.decoder_layers,
            hf.encoder_ffn_dim)
        assert (c.block_size, c.num_random_blocks, c.attention_type, c.use_bias, c.max_position_embeddings) == (
            hf.block_size, hf.num_random_blocks, hf.attention_type, hf.use_bias, hf.max_position_embeddings)
        assert (c.feed_forward_proj, c.scale_embedding, c.dropout_rate, c.attention_dropout, c.activation_dropout) == (
            hf.activation_function, hf.scale_embedding, hf.dropout, hf.attention_dropout, hf.activation_dropout)
        assert (c.pad_token_id, c.eos_token_id, c.bos_token_id, c.decoder_start_token_id) == (
            hf.pad_token_id, hf.eos_token_id, hf.bos_token_id, hf.decoder_start_token_id)
        assert c.d_kv == 64 and c.normalize_before and not c.layernorm_embedding and c.final_logits_bias
        assert c.position_embedding == "learned0"
    t = PRESETS["bigbird-tiny"]
    assert (t.d_model, t.num_heads, t.num_layers, t.num_decoder_layers, t.vocab_size) == (64, 4, 2, 2, 512)
    assert (t.block_size, t.num_random_blocks, t.max_position_embeddings) == (8, 2, 256)
    assert resolve_config("google/bigbird-pegasus-large-arxiv").d_model == 1024
    assert "block_size" not in PRESETS["pegasus-large"].to_hf_dict()  # other configs do not grow BigBird keys


def test_from_pretrained_reads_transformers_save_pretrained(tmp_path):
    ours, hf = _pair()
    hf.save_pretrained(str(tmp_path), safe_serialization=True)
    back = from_pretrained(str(tmp_path))
    assert back.config.model_type == "bigbird_pegasus" and back.config.block_size == 8 and not back.config.use_bias
    a, b = ours.state_dict(), back.state_dict()
    assert a.keys() == b.keys()
    for k in a:
        torch.testing.assert_close(a[k], b[k], atol=0, rtol=0, msg=k)


def test_transformers_loads_our_save_pretrained(tmp_path):
    import transformers
    ours, _ = _pair()
    save_pretrained(ours, str(tmp_path))
    hf = transformers.AutoModelForSeq2SeqLM.from_pretrained(str(tmp_path), attn_implementation="eager").eval()
    assert type(hf).__name__ == "BigBirdPegasusForConditionalGeneration"
    assert hf.config.block_size == 8 and hf.config.num_random_blocks == 2 and hf.config.use_bias is False
    ids, am, labels = _batch(ours.config.vocab_size, 100, 70)
    out = ours(input_ids=ids, attention_mask=am, labels=labels, return_logits=True)
    ref = hf(input_ids=ids, attention_mask=am, labels=labels)
    torch.testing.assert_close(out.logits, ref.logits, atol=2e-5, rtol=1e-4)


def _through_eos(seq, eos, pad):
    """``seq`` with everything after each row's first eos (past the start token) replaced by ``pad``."""
    done = ((seq[:, 1:] == eos).long().cumsum(1) > 0).long().cumsum(1) > 1
    out = seq.clone()
    out[:, 1:][done] = pad
    return out


@pytest.mark.parametrize("beams", [1, 2])
def test_generate_matches_hf(beams):
    """Eval mode: the "random" blocks are all block 0, so the repeats are what generate() runs on."""
    ours, hf = _pair()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(4, ours.config.vocab_size, (3, 100), generator=g)
    am = torch.ones_like(ids)
    am[2, 70:] = 0
    ids[2, 70:] = ours.config.pad_token_id
    kw = dict(max_length=12, num_beams=beams, min_length=0, no_repeat_ngram_size=0, length_penalty=1.0,
              early_stopping=False)
    a = ours.generate(ids, attention_mask=am, **kw)
    b = hf.generate(ids, attention_mask=am, do_sample=False, **kw)
    L = min(a.shape[1], b.shape[1])
    eos, pad = ours.config.eos_token_id, ours.config.pad_token_id
    assert torch.equal(_through_eos(a[:, :L], eos, pad), _through_eos(b[:, :L], eos, pad)), (a, b)
    assert torch.equal(_through_eos(a, eos, pad), a)


def test_what_bigbird_pegasus_does_not_implement():
    ours, _ = _pair()
    with pytest.raises(NotImplementedError, match="BigBird-Pegasus"):
        ours.enable_context_parallel(None)
    ours.enable_context_parallel(enable=False)  # switching it off stays harmless
    ids, am, labels = _batch(ours.config.vocab_size, 100, 70)
    seg = torch.zeros_like(ids)
    dseg = torch.zeros_like(labels)
    with pytest.raises(NotImplementedError, match="BigBird-Pegasus"):
        ours(input_ids=ids, attention_mask=am, labels=labels, decoder_input_ids=labels.clamp_min(0), segment_ids=seg,
             decoder_segment_ids=dseg, position_ids=seg, decoder_position_ids=dseg)
    with pytest.raises(NotImplementedError, match="BigBird-Pegasus"):
        ours.encode(ids, am, seg=(seg, seg))


def test_gradient_checkpointing_is_the_same_step():
    ours, _ = _pair(training=True)
    ids, am, labels = _batch(ours.config.vocab_size, 100, 70)
    ours(input_ids=ids, attention_mask=am, labels=labels).loss.backward()
    want = {n: p.grad.clone() for n, p in ours.named_parameters()}
    ours.zero_grad()
    ours.gradient_checkpointing_enable()
    ours(input_ids=ids, attention_mask=am, labels=labels).loss.backward()
    for n, p in ours.named_parameters():
        torch.testing.assert_close(p.grad, want[n], atol=1e-6, rtol=1e-5, msg=n)


def test_train_torchrun_smoke(tmp_path):
    env = dict(os.environ)
    env.update({"VH_ROOT": str(tmp_path), "DLLM_FORCE_CPU": "1", "OMP_NUM_THREADS": "2", "PYTHONPATH": ROOT})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train-torchrun.py"), "--model-ckpt", "bigbird-tiny",
                        "--output-dir", "out", "--batch-size", "4", "--evaluation-steps", "2", "--warmup-steps", "1",
                        "--synthetic", "16", "--max-source-length", "100", "--max-target-length", "10",
                        "--gen-max-length", "8"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    logs = [json.loads(x) for x in r.stdout.splitlines() if x.strip().startswith("{")]
    assert any("eval_loss" in x for x in logs)
    final = [x for x in logs if "train_samples_per_second" in x]
    assert final and final[-1]["train_loss"] > 0
    out = tmp_path / "outputs" / "out"
    assert (out / "model.safetensors").exists()
    assert json.load(open(out / "config.json"))["model_type"] == "bigbird_pegasus"
