"""T5Gemma on the CPU against transformers' T5GemmaForConditionalGeneration (eager attention, fp32): forward / backward
parity with and without an attention mask, in evaluation and in training mode, checkpoint and config.json round trips,
generation, what the family does not implement, and the op-level references the model stands on (soft-capped attention,
RoPE, capped cross-entropy, the norm offset).

The oracle is built from our ``to_hf_dict()`` and loaded with our ``to_hf_state_dict()`` (the method of
tests/test_longt5_cpu.py).  Both tiny presets are re-initialised so that the architecture's details show: norm weights
with std 0.3 (``1 + w`` is not 1) and projections scaled up until both soft caps bite — asserted on the oracle alone."""
import json
import os

import pytest
import torch

from distributed_llms_example_amd.models import (PRESETS, Seq2SeqConfig, build_model, from_pretrained, resolve_config,
                                                 save_pretrained, to_hf_state_dict)

TINY = ["t5gemma-tiny", "t5gemma-tiny-gqa"]
LOGITS = dict(atol=2e-5, rtol=1e-4)


def _hf_config(cfg, **over):
    import transformers
    d = cfg.to_hf_dict()
    assert d.pop("model_type") == "t5gemma"
    assert d.pop("architectures") == ["T5GemmaForConditionalGeneration"]
    d.pop("torch_dtype")
    for k, v in over.items():  # a module-level key, set in both stacks
        d["encoder"][k] = v
        d["decoder"][k] = v
    return transformers.T5GemmaConfig(**d, attn_implementation="eager")


def _hf_for(model, **over):
    import transformers
    hf = transformers.T5GemmaForConditionalGeneration(_hf_config(model.config, **over))
    missing, unexpected = hf.load_state_dict(to_hf_state_dict(model), strict=False)
    assert missing == ["lm_head.out_proj.weight"], missing  # tied to model.decoder.embed_tokens.weight
    assert not unexpected, unexpected
    hf.tie_weights()
    return hf


def _reinit(model, embed=12.0, proj=5.0):
    """Norm weights with std 0.3; projections and embeddings scaled up so that scores and logits reach their caps."""
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "layernorm" in n or n.endswith(".norm.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
            elif "embed_tokens" in n:
                p.mul_(embed)
            else:
                p.mul_(proj)
    return model


def _pair(name, **scales):
    torch.manual_seed(0)
    ours = _reinit(build_model(name), **scales).eval()
    return ours, _hf_for(ours).eval()


def _batch(V, B=2, S=23, T=9, pad_id=0):
    """23 source tokens, row 1 padded from token 17 on; 9 labels, the last two of row 0 ignored."""
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
def test_both_caps_bite(name):
    """On the oracle alone: without either cap the logits move by more than 100x the parity tolerance."""
    ours, hf = _pair(name)
    ids, am, labels = _batch(ours.config.vocab_size)
    with torch.no_grad():
        ref = hf(input_ids=ids, attention_mask=am, labels=labels).logits
        for key in ("attn_logit_softcapping", "final_logit_softcapping"):
            other = _hf_for(ours, **{key: None}).eval()
            moved = (other(input_ids=ids, attention_mask=am, labels=labels).logits - ref).abs().max().item()
            assert moved > 100 * LOGITS["atol"], (key, moved)


@pytest.mark.parametrize("name", TINY)
@pytest.mark.parametrize("masked", [True, False], ids=["attention_mask", "default_masks"])
@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_forward_backward_matches_hf(name, masked, training):
    """Without an attention_mask transformers' pad-id default masks are exercised; in training mode (the tiny presets
    have no dropout, so it is deterministic) its decoder also masks the pad input ids, among them the shifted -100."""
    ours, hf = _pair(name)
    ours.train(training)
    hf.train(training)
    cfg = ours.config
    assert cfg.dropout_rate == 0.0 and cfg.attention_dropout == 0.0
    ids, am, labels = _batch(cfg.vocab_size, pad_id=cfg.pad_token_id)
    mask = am if masked else None
    out = ours(input_ids=ids, attention_mask=mask, labels=labels, return_logits=True)
    ref = hf(input_ids=ids, attention_mask=mask, labels=labels)
    torch.testing.assert_close(out.logits, ref.logits, **LOGITS)
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
        assert k in hf_named and hf_named[k].grad is not None, k
        torch.testing.assert_close(g, hf_named[k].grad, atol=5e-5, rtol=1e-3, msg=k)
        checked += 1
    assert checked >= 20
    for k in ("model.encoder.embed_tokens.weight", "model.decoder.embed_tokens.weight"):
        assert k in mapped and mapped[k].abs().max() > 0


def test_the_window_matters():
    """With every encoder layer sliding, a source token farther than window x layers away leaves a position's state
    alone; with the preset's full layer it does not."""
    torch.manual_seed(0)
    cfg = PRESETS["t5gemma-tiny"].replace(layer_types=["sliding_attention", "sliding_attention"])
    ours = _reinit(build_model(cfg)).eval()
    ids, am, _ = _batch(cfg.vocab_size)
    with torch.no_grad():
        a = ours.encode(ids, am)
        ids2 = ids.clone()
        ids2[0, 22] = (ids2[0, 22] + 1) % cfg.vocab_size
        b = ours.encode(ids2, am)
        reach = cfg.sliding_window * cfg.num_layers  # 8
        assert torch.equal(a[0, :22 - reach], b[0, :22 - reach])
        assert not torch.equal(a[0, 22 - reach:], b[0, 22 - reach:])
        full, _ = _pair("t5gemma-tiny")
        assert not torch.equal(full.encode(ids, am)[0, :22 - reach], full.encode(ids2, am)[0, :22 - reach])


def test_rope_matters():
    ours, hf = _pair("t5gemma-tiny")
    ids, am, _ = _batch(ours.config.vocab_size)
    with torch.no_grad():
        a = ours.encode(ids, am)
        pos = torch.arange(23)[None].expand(2, -1) * 2 + 5
        b = ours.encode(ids, am, position_ids=pos)
        assert not torch.allclose(a, b, atol=1e-3)
        ref = hf.get_encoder()(input_ids=ids, attention_mask=am, position_ids=pos).last_hidden_state
    torch.testing.assert_close(b[am.bool()], ref[am.bool()], atol=2e-5, rtol=1e-4)


def test_module_names_mirror_hf():
    ours, hf = _pair("t5gemma-tiny-gqa")
    names = set(to_hf_state_dict(ours))
    for n in range(2):
        for stack in ("encoder", "decoder"):
            for w in ("q_proj", "k_proj", "v_proj", "o_proj"):
                assert f"model.{stack}.layers.{n}.self_attn.{w}.weight" in names
            for w in ("gate_proj", "up_proj", "down_proj"):
                assert f"model.{stack}.layers.{n}.mlp.{w}.weight" in names
            assert f"model.{stack}.layers.{n}.pre_self_attn_layernorm.weight" in names
        assert f"model.decoder.layers.{n}.cross_attn.k_proj.weight" in names
    assert "lm_head.out_proj.weight" not in names  # tied: stored once
    assert names == set(hf.state_dict()) - {"lm_head.out_proj.weight"}
    sd = to_hf_state_dict(ours)
    assert sd["model.encoder.layers.0.self_attn.q_proj.weight"].shape == (64, 64)
    assert sd["model.encoder.layers.0.self_attn.k_proj.weight"].shape == (32, 64)  # 2 K/V heads of 16


@pytest.mark.parametrize("name", TINY)
def test_config_round_trip(name, tmp_path):
    cfg = PRESETS[name]
    cfg.save(str(tmp_path))
    with open(os.path.join(tmp_path, "config.json")) as f:
        d = json.load(f)
    assert d["model_type"] == "t5gemma" and d["architectures"] == ["T5GemmaForConditionalGeneration"]
    assert d["encoder"]["sliding_window"] == 4 and d["decoder"]["sliding_window"] == 64
    assert d["encoder"]["num_key_value_heads"] == cfg.num_kv_heads
    assert d["decoder"]["rope_parameters"]["rope_theta"] == cfg.rope_theta
    back = resolve_config(str(tmp_path))
    a, b = cfg.to_dict(), back.to_dict()
    for k in a:
        if k not in ("name", "generation"):
            assert a[k] == b[k], k
    assert Seq2SeqConfig.from_hf_dict(d).to_hf_dict() == d  # nested in, nested out
    # transformers reads it, and what transformers writes back reads the same
    hc = _hf_config(cfg)
    again = Seq2SeqConfig.from_hf_dict(json.loads(hc.to_json_string()))
    for k in a:
        if k not in ("name", "generation"):
            assert a[k] == again.to_dict()[k], k


def test_presets():
    a, b = PRESETS["t5gemma-tiny"], PRESETS["t5gemma-tiny-gqa"]
    assert (a.d_model, a.num_layers, a.num_decoder_layers, a.num_heads, a.num_kv_heads, a.d_kv) == (64, 2, 2, 4, 4, 16)
    assert b.num_kv_heads == 2
    for c in (a, b):
        assert c.layer_types == ["sliding_attention", "full_attention"] and c.vocab_size == 512
        assert (c.sliding_window, c.decoder_sliding_window, c.max_position_embeddings) == (4, 64, 128)
        assert (c.attn_logit_softcapping, c.final_logit_softcapping) == (2.0, 3.0)
    assert "encoder" not in PRESETS["t5-tiny"].to_hf_dict()


@pytest.mark.parametrize("name", TINY)
def test_from_pretrained_reads_transformers_save_pretrained(name, tmp_path):
    ours, hf = _pair(name)
    hf.save_pretrained(str(tmp_path), safe_serialization=True)
    back = from_pretrained(str(tmp_path))
    assert back.config.model_type == "t5gemma" and back.config.num_kv_heads == ours.config.num_kv_heads
    a, b = ours.state_dict(), back.state_dict()
    assert a.keys() == b.keys()
    for k in a:
        torch.testing.assert_close(a[k], b[k], atol=0, rtol=0, msg=k)


@pytest.mark.parametrize("name", TINY)
def test_transformers_loads_our_save_pretrained(name, tmp_path):
    import transformers
    ours, _ = _pair(name)
    save_pretrained(ours, str(tmp_path))
    hf, info = transformers.AutoModelForSeq2SeqLM.from_pretrained(str(tmp_path), attn_implementation="eager",
                                                                  output_loading_info=True)
    hf.eval()
    assert type(hf).__name__ == "T5GemmaForConditionalGeneration"
    assert set(info["missing_keys"]) <= {"lm_head.out_proj.weight"} and not info["unexpected_keys"], info
    ids, am, labels = _batch(ours.config.vocab_size)
    out = ours(input_ids=ids, attention_mask=am, labels=labels, return_logits=True)
    ref = hf(input_ids=ids, attention_mask=am, labels=labels)
    torch.testing.assert_close(out.logits, ref.logits, **LOGITS)


def _through_eos(seq, eos, pad):
    """``seq`` with everything after each row's first eos (past the start token) replaced by ``pad``."""
    done = ((seq[:, 1:] == eos).long().cumsum(1) > 0).long().cumsum(1) > 1
    out = seq.clone()
    out[:, 1:][done] = pad
    return out


@pytest.mark.parametrize("name", TINY)
@pytest.mark.parametrize("beams", [1, 3])
def test_generate_matches_hf(name, beams):
    # smaller embeddings than the parity tests': with the tied head's logits at their cap every step repeats its input
    ours, hf = _pair(name, embed=1.0, proj=10.0)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(4, ours.config.vocab_size, (3, 23), generator=g)
    am = torch.ones_like(ids)
    am[2, 17:] = 0
    ids[2, 17:] = ours.config.pad_token_id
    kw = dict(max_length=12, num_beams=beams, min_length=0, no_repeat_ngram_size=0, length_penalty=1.0,
              early_stopping=False)
    a = ours.generate(ids, attention_mask=am, **kw)
    b = hf.generate(ids, attention_mask=am, do_sample=False, **kw)
    assert a[:, 0].eq(ours.config.bos_token_id).all()  # the decoder starts with decoder.bos_token_id
    L = min(a.shape[1], b.shape[1])
    eos, pad = ours.config.eos_token_id, ours.config.pad_token_id
    assert torch.equal(_through_eos(a[:, :L], eos, pad), _through_eos(b[:, :L], eos, pad)), (a, b)
    assert a[:, 1:].unique().numel() > 3  # not one token repeated


def test_unbalanced_config_raises():
    d = PRESETS["t5gemma-tiny"].to_hf_dict()
    for key, val in (("hidden_size", 128), ("head_dim", 32), ("num_attention_heads", 8), ("num_key_value_heads", 2)):
        bad = json.loads(json.dumps(d))
        bad["decoder"][key] = val
        with pytest.raises(ValueError, match=key):
            Seq2SeqConfig.from_hf_dict(bad)
    ok = json.loads(json.dumps(d))
    ok["decoder"].update(num_hidden_layers=3, sliding_window=32,
                         layer_types=["sliding_attention", "full_attention", "sliding_attention"])
    cfg = Seq2SeqConfig.from_hf_dict(ok)  # layer counts and windows may differ
    assert (cfg.num_layers, cfg.num_decoder_layers, cfg.decoder_sliding_window) == (2, 3, 32)
    with pytest.raises(ValueError, match="unsupported model_type"):
        Seq2SeqConfig.from_hf_dict({"model_type": "t5gemma2"})


def test_decoder_length_above_the_window_raises():
    cfg = PRESETS["t5gemma-tiny"].replace(decoder_sliding_window=8)
    m = build_model(cfg).eval()
    ids, am, labels = _batch(cfg.vocab_size)  # 9 labels > 8
    with pytest.raises(NotImplementedError, match="decoder.sliding_window = 8"):
        m(input_ids=ids, attention_mask=am, labels=labels)
    m(input_ids=ids, attention_mask=am, labels=labels[:, :8])  # at the window: served
    with pytest.raises(NotImplementedError, match="decoder.sliding_window = 8"):
        m.generate(ids, attention_mask=am, max_length=9)
    assert m.generate(ids, attention_mask=am, max_length=8).shape[1] <= 8
    # no sliding decoder layer: no limit
    free = build_model(cfg.replace(decoder_layer_types=["full_attention", "full_attention"])).eval()
    free(input_ids=ids, attention_mask=am, labels=labels)


def test_unsupported_modes_raise():
    from distributed_llms_example_amd.models.lora import LoraConfig, apply_lora
    m = build_model("t5gemma-tiny")
    ids, am, labels = _batch(m.config.vocab_size)
    with pytest.raises(NotImplementedError, match="T5Gemma"):
        apply_lora(m, LoraConfig(r=4))
    with pytest.raises(NotImplementedError, match="T5Gemma"):
        m.lm_head_operands(input_ids=ids, attention_mask=am, labels=labels)  # as a teacher
    with pytest.raises(NotImplementedError, match="T5Gemma"):
        m(input_ids=ids, attention_mask=am, labels=labels, distill=object())  # as a student
    with pytest.raises(NotImplementedError, match="T5Gemma"):
        m(input_ids=ids, attention_mask=am, labels=labels, preference=object())
    with pytest.raises(NotImplementedError, match="T5Gemma"):
        m(input_ids=ids, attention_mask=am, labels=labels, segment_ids=am, decoder_segment_ids=labels)
    with pytest.raises(NotImplementedError, match="T5Gemma"):
        m.enable_context_parallel(None)
    m.enable_context_parallel(enable=False)  # switching it off stays harmless


# ------------------------------------------------------------------------------------------------ op level


def _softmax_attention_f64(q, k, v, scale, cap, kpm=None, causal=False, window=None):
    """Hand-written: q [B, Sq, H, D], k / v [B, Sk, H, D] in fp64."""
    q, k, v = q.double(), k.double(), v.double()
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    out = torch.zeros(B, Sq, H, D, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            s = (q[b, :, h] @ k[b, :, h].T) * scale
            s = cap * torch.tanh(s / cap)
            i = torch.arange(Sq)[:, None]
            j = torch.arange(Sk)[None, :]
            hide = torch.zeros(Sq, Sk, dtype=torch.bool)
            if kpm is not None:
                hide |= ~kpm[b].bool()[None, :]
            if causal:
                hide |= j > i + (Sk - Sq)
            if window is not None:
                hide |= (j - i).abs() > window
            s = s.masked_fill(hide, float("-inf"))
            e = torch.exp(s - s.max(-1, keepdim=True).values)
            out[b, :, h] = (e / e.sum(-1, keepdim=True)) @ v[b, :, h]
    return out


@pytest.mark.parametrize("case", ["plain", "padded", "causal", "decode", "window"])
def test_attention_reference_softcap(case):
    from distributed_llms_example_amd.ops import attention as A
    g = torch.Generator().manual_seed(3)
    B, H, D, S = 2, 3, 16, 37
    Sq = 5 if case == "decode" else S
    q = torch.randn(B, Sq, H, D, generator=g) * 2
    k = torch.randn(B, S, H, D, generator=g) * 2
    v = torch.randn(B, S, H, D, generator=g)
    kpm = None
    if case == "padded":
        kpm = torch.ones(B, S, dtype=torch.bool)
        kpm[1, 29:] = False
    kw = dict(scale=0.5, causal=case in ("causal", "decode"), key_padding_mask=kpm,
              window=6 if case == "window" else None)
    cap = 3.0
    ref = _softmax_attention_f64(q, k, v, 0.5, cap, kpm, kw["causal"], kw["window"])
    out = A.attention(q, k, v, softcap=cap, **kw)
    torch.testing.assert_close(out.double(), ref, atol=2e-6, rtol=1e-5)
    assert (out - A.attention(q, k, v, **kw)).abs().max() > 1e-2  # the cap bites
    assert torch.equal(A.attention(q, k, v, softcap=None, **kw), A.attention(q, k, v, **kw))
    if case == "plain":
        qkv = torch.stack((q, k, v), 2)
        assert torch.equal(A.attention_qkv(qkv, softcap=cap, **kw), out)
        assert torch.equal(A.attention_q_kv(q, torch.stack((k, v), 2), softcap=cap, **kw), out)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="softcap"):
                A.attention(q, k, v, softcap=bad, **kw)


def test_routing_with_softcap():
    from distributed_llms_example_amd.ops import routing
    assert routing.attention_route(64, True) == "attn.hip"
    assert routing.attention_route(64, True, softcap=True) == "attn_hd.hip"  # csrc/attn.hip has no cap
    assert routing.attention_route(64, True, 4, softcap=True) == "attn_hd.hip"
    assert routing.attention_route(64, False, softcap=True) == "attn_f32.hip"
    assert routing.attention_route(128, True, softcap=True) == "attn_hd.hip"
    assert routing.attention_route(32, True, softcap=True) == "composite"
    assert routing.attention_route(32, True) == "attn_hd.hip"
    assert routing.attention_route(16, True, softcap=True) == "composite"
    assert routing.attention_route(256, True, softcap=True) == "composite"
    assert routing.attention_route(64, True, softcap=True, segments=True) == "composite"


@pytest.mark.parametrize("D", [16, 64])
def test_rope_reference_matches_transformers(D):
    from transformers.models.t5gemma.modeling_t5gemma import apply_rotary_pos_emb
    from distributed_llms_example_amd.ops.rope import rope, rope_table
    g = torch.Generator().manual_seed(5)
    B, S, H = 2, 11, 3
    qkv = torch.randn(B, S, 3, H, D, generator=g)
    theta = 10000.0
    cos, sin = rope_table(theta, D, 64)
    assert cos.shape == (64, D // 2) and cos.dtype == torch.float32
    for pos in (torch.arange(S), torch.arange(S)[None].expand(B, -1) + torch.tensor([[7], [20]])):
        out = rope(qkv, pos, cos, sin, slots=2)
        assert torch.equal(out[:, :, 2], qkv[:, :, 2])  # v untouched
        p2 = pos if pos.dim() == 2 else pos[None].expand(B, -1)
        inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float) / D))
        fr = p2[:, :, None].float() * inv[None, None, :]
        emb = torch.cat((fr, fr), -1)
        # transformers' layout is [B, H, S, D]
        qh, kh = apply_rotary_pos_emb(qkv[:, :, 0].transpose(1, 2), qkv[:, :, 1].transpose(1, 2), emb.cos(), emb.sin())
        torch.testing.assert_close(out[:, :, 0], qh.transpose(1, 2), atol=1e-6, rtol=1e-6)
        torch.testing.assert_close(out[:, :, 1], kh.transpose(1, 2), atol=1e-6, rtol=1e-6)
    # a lone q view, and the gradient: the rotation is orthogonal, so backward(forward) is the identity
    x = qkv[:, :, 0].unsqueeze(2).clone().requires_grad_(True)
    y = rope(x, torch.arange(S), cos, sin)
    gr = torch.randn(y.shape, generator=g)
    y.backward(gr)
    from distributed_llms_example_amd.ops.rope import _reference
    torch.testing.assert_close(_reference(x.grad, torch.arange(S), cos, sin), gr, atol=1e-6, rtol=1e-6)
    with pytest.raises(ValueError, match="rope"):
        rope(qkv, torch.arange(S + 1), cos, sin)


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_capped_cross_entropy_reference(smoothing):
    import torch.nn.functional as F
    from distributed_llms_example_amd.ops.cross_entropy import cross_entropy
    from distributed_llms_example_amd.ops.lm_head import lm_head_loss
    g = torch.Generator().manual_seed(9)
    N, V, c = 13, 50, 3.0
    x = (torch.randn(N, V, generator=g) * 4).requires_grad_(True)
    y = torch.randint(0, V, (N,), generator=g)
    y[3] = -100
    loss = cross_entropy(x, y, label_smoothing=smoothing, softcap=c)
    x2 = x.detach().clone().requires_grad_(True)
    ref = F.cross_entropy(c * torch.tanh(x2 / c), y, ignore_index=-100, label_smoothing=smoothing)
    torch.testing.assert_close(loss, ref, atol=1e-6, rtol=1e-6)
    loss.backward()
    ref.backward()
    torch.testing.assert_close(x.grad, x2.grad, atol=1e-7, rtol=1e-5)
    assert (x.detach().abs() > c).float().mean() > 0.3  # many logits sit in the saturated range
    assert not torch.allclose(cross_entropy(x.detach(), y, label_smoothing=smoothing), loss.detach(), atol=1e-2)
    h, w = torch.randn(N, 8, generator=g), torch.randn(V, 8, generator=g) * 2
    torch.testing.assert_close(lm_head_loss(h, w, y, label_smoothing=smoothing, softcap=c),
                               F.cross_entropy(c * torch.tanh(h @ w.T / c), y, label_smoothing=smoothing),
                               atol=1e-6, rtol=1e-6)
    with pytest.raises(ValueError, match="softcap"):
        cross_entropy(x, y, softcap=0.0)


def test_norm_offset_reference():
    from distributed_llms_example_amd.ops import norms
    g = torch.Generator().manual_seed(11)
    x = torch.randn(5, 7, 32, generator=g, requires_grad=True)
    r = torch.randn(5, 7, 32, generator=g)
    w = (torch.randn(32, generator=g) * 0.3).requires_grad_(True)
    eps = 1e-6

    def gemma(t):  # transformers' T5GemmaRMSNorm
        return t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + eps) * (1.0 + w)

    torch.testing.assert_close(norms.rms_norm(x, w, eps, offset=1.0), gemma(x), atol=1e-6, rtol=1e-6)
    n, s = norms.add_dropout_rms_norm(r, x, w, eps, 0.0, 0, offset=1.0)
    torch.testing.assert_close(s, r + x)
    torch.testing.assert_close(n, gemma(r + x), atol=1e-6, rtol=1e-6)
    n2, _ = norms.dropout_rms_norm(x, w, eps, 0.0, 0, offset=1.0)
    torch.testing.assert_close(n2, gemma(x), atol=1e-6, rtol=1e-6)
    gw, = torch.autograd.grad(norms.rms_norm(x, w, eps, offset=1.0).square().sum(), w)
    gw_ref, = torch.autograd.grad(gemma(x).square().sum(), w)
    torch.testing.assert_close(gw, gw_ref, atol=1e-5, rtol=1e-5)
    assert torch.equal(norms.rms_norm(x, w, eps), norms.rms_norm(x, w, eps, offset=0.0))  # no offset: as before


def test_train_torchrun_entry_point(tmp_path):
    """The entry point trains, evaluates (generation included) and saves a T5Gemma model like any other family, and
    transformers' config class reads the saved config.json (the method of tests/test_entrypoints_cpu.py)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.update({"VH_ROOT": str(tmp_path), "DLLM_FORCE_CPU": "1", "OMP_NUM_THREADS": "2", "PYTHONPATH": root})
    r = subprocess.run([sys.executable, os.path.join(root, "train-torchrun.py"), "--model-ckpt", "t5gemma-tiny",
                        "--output-dir", "out", "--batch-size", "4", "--grad-accum", "2", "--evaluation-steps", "2",
                        "--warmup-steps", "1", "--synthetic", "32", "--max-source-length", "40",
                        "--max-target-length", "10", "--gen-max-length", "8"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    logs = [json.loads(x) for x in r.stdout.splitlines() if x.strip().startswith("{")]
    assert any("eval_loss" in x for x in logs)
    final = [x for x in logs if "train_samples_per_second" in x]
    assert final and final[-1]["train_loss"] > 0
    out = tmp_path / "outputs" / "out"
    for f in ("config.json", "model.safetensors", "generation_config.json"):
        assert (out / f).exists(), f
    back = from_pretrained(str(out))
    assert back.config.model_type == "t5gemma" and back.config.sliding_window == 4


# ------------------------------------------------------------------------------------------------ Adafactor


@pytest.mark.parametrize("mode", ["trainer", "relative"])
@pytest.mark.parametrize("name", TINY)
def test_adafactor_matches_transformers(name, mode):
    """FusedAdafactor's units are transformers' parameters: with grouped K/V heads the fused qkv_proj splits into q
    (64 rows) and the shorter k and v (32 each), every one with its own factored moments, clip and scale — four steps
    against ``transformers.optimization.Adafactor`` on identical gradients, the method and bound of
    tests/test_adafactor_cpu.py (atol 1e-6, rtol 1e-5 on every weight)."""
    from transformers.optimization import Adafactor
    from distributed_llms_example_amd.models.hf_io import hf_param_parts
    from distributed_llms_example_amd.ops.optim import FusedAdafactor
    from distributed_llms_example_amd.parallel.flat import FlatParams
    kw = {"trainer": dict(lr=1e-2, scale_parameter=False, relative_step=False),
          "relative": dict(lr=None, scale_parameter=True, relative_step=True)}[mode]
    torch.manual_seed(0)
    ours = _reinit(build_model(name), embed=1.0, proj=1.0).train()
    hf = _hf_for(ours)
    cfg = ours.config
    qkv = "model.encoder.layers.0.self_attn.qkv_proj.weight"
    assert hf_param_parts(cfg, qkv) == ([64, 32, 32] if cfg.num_kv_heads == 2 else 3)
    assert hf_param_parts(cfg, "model.decoder.layers.0.cross_attn.kv_proj.weight") == 2
    assert hf_param_parts(cfg, "model.encoder.layers.0.mlp.wi.weight") == 2
    assert hf_param_parts(cfg, "model.encoder.norm.weight") == 1
    flat = FlatParams(ours)
    opt = FusedAdafactor(flat, parts=lambda n: hf_param_parts(cfg, n), **kw)
    units = [u for u in opt.units if u["name"] == qkv]
    assert [(u["rows"], u["start"]) for u in units] == ([(64, 0), (32, 64 * 64), (32, 96 * 64)]
                                                         if cfg.num_kv_heads == 2 else
                                                         [(64, 0), (64, 64 * 64), (64, 128 * 64)])
    ref = Adafactor([p for n, p in hf.named_parameters() if n != "lm_head.out_proj.weight"], **kw)
    for s in range(4):
        g = torch.Generator().manual_seed(s)
        ids = torch.randint(3, cfg.vocab_size, (3, 13), generator=g)
        am = torch.ones(3, 13, dtype=torch.long)
        am[1, 9:] = 0
        lab = torch.randint(3, cfg.vocab_size, (3, 7), generator=g)
        flat.reset_pending()
        ours(input_ids=ids, attention_mask=am, labels=lab).loss.backward()
        mapped = to_hf_state_dict(_GradView(ours))
        for n, p in hf.named_parameters():
            if n in mapped:
                p.grad = mapped[n].detach().clone()
        opt.step()
        opt.zero_grad()
        ref.step()
    got, want = to_hf_state_dict(ours), hf.state_dict()
    assert len(got) > 20
    for k, v in got.items():
        torch.testing.assert_close(v, want[k], atol=1e-6, rtol=1e-5, msg=lambda m: f"{k}: {m}")


def test_adafactor_engine_step_with_grouped_heads(monkeypatch):
    """``TrainEngine(optim="adafactor")`` builds and steps on the grouped-K/V preset (its qkv_proj has no three equal
    slices), and a wrong size list is refused."""
    from distributed_llms_example_amd.ops.optim import FusedAdafactor
    from distributed_llms_example_amd.parallel import env as env_mod
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.parallel.flat import FlatParams
    from distributed_llms_example_amd.train.engine import TrainEngine
    monkeypatch.setattr(env_mod, "_ENV", None)
    env = init_distributed(cpu=True)
    torch.manual_seed(0)
    m = build_model("t5gemma-tiny-gqa")
    eng = TrainEngine(m, env, lr=1e-2, dtype=torch.float32, optim="adafactor")
    eng.train()
    assert sorted({u["rows"] for u in eng.optimizer.units if u["name"].endswith("self_attn.qkv_proj.weight")}) == [32, 64]
    ids, am, labels = _batch(m.config.vocab_size)
    batch = dict(input_ids=ids, attention_mask=am, labels=labels)
    losses = []
    for _ in range(4):
        losses.append(float(eng.forward_backward(batch)))
        eng.step()
    assert all(x == x for x in losses) and losses[-1] < losses[0], losses
    with pytest.raises(ValueError, match="does not split into dim-0 slices"):
        FusedAdafactor(FlatParams(build_model("t5gemma-tiny-gqa")), lr=1e-2, relative_step=False,
                       parts=lambda n: [64, 32, 16] if n.endswith("qkv_proj.weight") else 1)
