"""LongT5-local on the CPU against transformers' LongT5ForConditionalGeneration: forward / backward parity, checkpoint
and config.json round trips, generation, and what the family does not implement.

transformers' LongT5LocalAttention works on blocks of local_radius + 1 tokens and three-block windows; on every
non-padded query row that equals a softmax over the keys within local_radius (models/t5.py).  Padded query rows differ
(transformers averages over masked keys, ours are rows without a visible key), so encoder states are compared at valid
positions only; logits, loss and gradients never see those rows."""
import json
import os

import pytest
import torch

from distributed_llms_example_amd.models import (PRESETS, Seq2SeqConfig, build_model, from_pretrained, resolve_config,
                                                 save_pretrained, to_hf_state_dict)

TINY = ["longt5-tiny", "longt5-tiny-gated"]


def _hf_for(model):
    """The transformers model of one of our LongT5 configs, with our weights (the role of hf_oracle.hf_model_for)."""
    import transformers
    d = model.config.to_hf_dict()
    assert d.pop("model_type") == "longt5"
    assert d.pop("architectures") == ["LongT5ForConditionalGeneration"]
    d.pop("torch_dtype")
    hf = transformers.LongT5ForConditionalGeneration(transformers.LongT5Config(**d, attn_implementation="eager"))
    missing, unexpected = hf.load_state_dict(to_hf_state_dict(model), strict=False)
    # tied configs: transformers ties these to `shared`; untied ones: our state dict carries every one of them
    allowed = {"encoder.embed_tokens.weight", "decoder.embed_tokens.weight", "lm_head.weight"}
    assert not [m for m in missing if m not in allowed or not model.config.tie_word_embeddings], missing
    assert not unexpected, unexpected
    return hf


def _pair(name):
    torch.manual_seed(0)
    ours = build_model(name).eval()  # (unlike T5, transformers keeps an untied LongT5's lm_head its own)
    return ours, _hf_for(ours).eval()


def _batch(V, B=2, S=23, T=9, pad_id=0):
    """23 source tokens (not a multiple of radius + 1 = 6), row 1 padded from token 17 on."""
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, V, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    am[1, 17:] = 0
    ids[1, 17:] = pad_id
    labels = torch.randint(3, V, (B, T), generator=g)
    labels[0, -2:] = -100
    return ids, am, labels


class _GradView:
    def __init__(self, m):
        self.config = m.config
        self._m = m

    def state_dict(self):
        return {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in self._m.named_parameters()}


@pytest.mark.parametrize("name", TINY)
def test_forward_backward_matches_hf(name):
    ours, hf = _pair(name)
    assert ours.config.local_radius == 5
    ids, am, labels = _batch(ours.config.vocab_size, pad_id=ours.config.pad_token_id)
    out = ours(input_ids=ids, attention_mask=am, labels=labels, return_logits=True)
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
    if hasattr(ours, "lm_head"):
        # untied: transformers holds three embedding matrices where ours shares one between encoder and decoder
        for stack in ("encoder", "decoder"):
            mapped.pop(f"{stack}.embed_tokens.weight")
        torch.testing.assert_close(mapped.pop("shared.weight"), hf_named["encoder.embed_tokens.weight"].grad +
                                   hf_named["decoder.embed_tokens.weight"].grad, atol=5e-5, rtol=1e-3)
    checked = 0
    for k, g in mapped.items():
        if k in hf_named and hf_named[k].grad is not None:
            torch.testing.assert_close(g, hf_named[k].grad, atol=5e-5, rtol=1e-3, msg=k)
            checked += 1
    assert checked >= 10
    assert any(".LocalSelfAttention.relative_attention_bias" in k for k in mapped)


def test_the_window_matters():
    """The encoder is really windowed: a far-away source token does not reach a position's encoder state through one
    layer's radius times the depth, and the plain T5 of the same weights computes something else."""
    ours, _ = _pair("longt5-tiny")
    ids, am, _ = _batch(ours.config.vocab_size)
    a = ours.encode(ids, am)
    ids2 = ids.clone()
    ids2[0, 22] = (ids2[0, 22] + 1) % ours.config.vocab_size
    b = ours.encode(ids2, am)
    reach = ours.config.local_radius * ours.config.num_layers  # 10
    assert torch.equal(a[0, :22 - reach], b[0, :22 - reach])
    assert not torch.equal(a[0, 22 - reach:], b[0, 22 - reach:])
    plain = build_model(ours.config.replace(t5_flavor="t5")).eval()
    sd = {k.replace("LocalSelfAttention", "SelfAttention"): v for k, v in ours.state_dict().items()}
    plain.load_state_dict(sd)
    assert not torch.allclose(plain.encode(ids, am), a, atol=1e-3)


def test_module_names_mirror_hf():
    ours, hf = _pair("longt5-tiny-gated")
    names = set(to_hf_state_dict(ours))
    assert "encoder.block.0.layer.0.LocalSelfAttention.relative_attention_bias.weight" in names
    assert "encoder.block.1.layer.0.LocalSelfAttention.relative_attention_bias.weight" not in names
    for n in range(2):
        for w in "qkvo":
            assert f"encoder.block.{n}.layer.0.LocalSelfAttention.{w}.weight" in names
            assert f"decoder.block.{n}.layer.0.SelfAttention.{w}.weight" in names
            assert f"decoder.block.{n}.layer.1.EncDecAttention.{w}.weight" in names
    assert names <= set(hf.state_dict())


@pytest.mark.parametrize("name", TINY + ["long-t5-local-base", "long-t5-local-large"])
def test_config_round_trip(name, tmp_path):
    cfg = PRESETS[name]
    assert cfg.t5_flavor == "longt5" and cfg.local_encoder and cfg.encoder_attention_type == "local"
    cfg.save(str(tmp_path))
    with open(os.path.join(tmp_path, "config.json")) as f:
        d = json.load(f)
    assert d["model_type"] == "longt5" and d["architectures"] == ["LongT5ForConditionalGeneration"]
    assert d["encoder_attention_type"] == "local" and d["local_radius"] == cfg.local_radius
    assert d["global_block_size"] == 16
    back = resolve_config(str(tmp_path))
    a, b = cfg.to_dict(), back.to_dict()
    for k in a:
        if k not in ("name", "generation"):
            assert a[k] == b[k], k
    d["global_block_size"] = 8  # passed through
    assert Seq2SeqConfig.from_hf_dict(d).to_hf_dict()["global_block_size"] == 8


def test_presets_have_the_published_shapes():
    b, l = PRESETS["long-t5-local-base"], PRESETS["long-t5-local-large"]
    assert (b.d_model, b.d_kv, b.num_heads, b.num_layers, b.num_decoder_layers, b.d_ff) == (768, 64, 12, 12, 12, 2048)
    assert (l.d_model, l.d_kv, l.num_heads, l.num_layers, l.num_decoder_layers, l.d_ff) == (1024, 64, 16, 24, 24, 2816)
    for c in (b, l):
        assert c.feed_forward_proj == "gated-gelu" and not c.tie_word_embeddings and c.vocab_size == 32128
        assert c.local_radius == 127
    assert resolve_config("google/long-t5-local-base").d_model == 768
    # T5 configs do not grow LongT5 keys
    assert "local_radius" not in PRESETS["t5-base"].to_hf_dict()


def test_transient_global_raises():
    d = PRESETS["longt5-tiny"].to_hf_dict()
    d["encoder_attention_type"] = "transient-global"
    with pytest.raises(ValueError, match="transient-global"):
        Seq2SeqConfig.from_hf_dict(d)


@pytest.mark.parametrize("name", TINY)
def test_from_pretrained_reads_transformers_save_pretrained(name, tmp_path):
    ours, hf = _pair(name)
    hf.save_pretrained(str(tmp_path), safe_serialization=True)
    back = from_pretrained(str(tmp_path))
    assert back.config.t5_flavor == "longt5" and back.config.local_radius == 5
    a, b = ours.state_dict(), back.state_dict()
    assert a.keys() == b.keys()
    for k in a:
        torch.testing.assert_close(a[k], b[k], atol=0, rtol=0, msg=k)


@pytest.mark.parametrize("name", TINY)
def test_transformers_loads_our_save_pretrained(name, tmp_path):
    import transformers
    ours, _ = _pair(name)
    save_pretrained(ours, str(tmp_path))
    hf = transformers.AutoModelForSeq2SeqLM.from_pretrained(str(tmp_path), attn_implementation="eager").eval()
    assert type(hf).__name__ == "LongT5ForConditionalGeneration"
    assert hf.config.local_radius == 5 and hf.config.encoder_attention_type == "local"
    ids, am, labels = _batch(ours.config.vocab_size)
    out = ours(input_ids=ids, attention_mask=am, labels=labels, return_logits=True)
    ref = hf(input_ids=ids, attention_mask=am, labels=labels)
    torch.testing.assert_close(out.logits, ref.logits, atol=2e-5, rtol=1e-4)


def _through_eos(seq, eos, pad):
    """``seq`` with everything after each row's first eos (past the start token) replaced by ``pad``."""
    done = ((seq[:, 1:] == eos).long().cumsum(1) > 0).long().cumsum(1) > 1
    out = seq.clone()
    out[:, 1:][done] = pad
    return out


@pytest.mark.parametrize("name", TINY)
@pytest.mark.parametrize("beams", [1, 2])
def test_generate_matches_hf(name, beams):
    ours, hf = _pair(name)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(4, ours.config.vocab_size, (3, 23), generator=g)
    am = torch.ones_like(ids)
    am[2, 17:] = 0
    ids[2, 17:] = ours.config.pad_token_id
    kw = dict(max_length=12, num_beams=beams, min_length=0, no_repeat_ngram_size=0, length_penalty=1.0,
              early_stopping=False)
    a = ours.generate(ids, attention_mask=am, **kw)
    b = hf.generate(ids, attention_mask=am, do_sample=False, **kw)
    L = min(a.shape[1], b.shape[1])
    eos, pad = ours.config.eos_token_id, ours.config.pad_token_id
    # what follows a row's first eos is filler, not tokens: ours writes pad_token_id, transformers' beam search writes
    # `pad_token_id or eos_token_id` (generation/utils.py _beam_search: eos when the pad id is 0, as T5's is)
    assert torch.equal(_through_eos(a[:, :L], eos, pad), _through_eos(b[:, :L], eos, pad)), (a, b)
    assert torch.equal(_through_eos(a, eos, pad), a)


def test_context_parallel_is_not_implemented():
    m = build_model("longt5-tiny")
    with pytest.raises(NotImplementedError, match="LongT5"):
        m.enable_context_parallel(None)
    m.enable_context_parallel(enable=False)  # switching it off stays harmless
    assert not hasattr(m.encoder, "_cp_group")


def test_long_inputs_are_not_chunked(monkeypatch):
    """Above attn_chunk_min the plain T5 encoder hands a chunk marker to its self-attention; the windowed encoder keeps
    its ordinary LUT and one attention call per layer at the full length."""
    from distributed_llms_example_amd.ops import attention as A, routing
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(attn_chunk_min=16, attn_chunk=8))
    ours, _ = _pair("longt5-tiny")
    calls = []
    orig = A.attention_qkv
    monkeypatch.setattr(A, "attention_qkv", lambda qkv, **kw: (calls.append((qkv.shape[1], kw.get("window"))),
                                                                 orig(qkv, **kw))[1])
    ids, am, _ = _batch(ours.config.vocab_size)
    ours.encode(ids, am)
    assert calls == [(23, 5)] * ours.config.num_layers
