"""LED on the CPU against transformers' LEDForConditionalGeneration (eager) with our weights: forward / backward
parity, checkpoint and config.json round trips, generation, the two ways to name the global tokens, and what the
family does not implement.

transformers pads the input to a multiple of attention_window and works on overlapping chunks; on every valid query
row that equals one softmax over the valid keys that are inside the window or global, and full attention through the
global projections at the global rows (models/bart.py).  Its padded query rows are 0 and ours are not, so encoder
states are compared at valid positions only; logits, loss and gradients never see those rows.  Tolerances are those
of tests/test_longt5_cpu.py."""
import json
import os

import pytest
import torch

from distributed_llms_example_amd.data.collator import DataCollatorForSeq2Seq
from distributed_llms_example_amd.models import (PRESETS, Seq2SeqConfig, build_model, from_pretrained, resolve_config,
                                                 save_pretrained, to_hf_state_dict)

_TIED = {"led.encoder.embed_tokens.weight", "led.decoder.embed_tokens.weight", "lm_head.weight"}


def _hf_for(model):
    """The transformers model of one of our LED configs, with our weights."""
    import transformers
    d = model.config.to_hf_dict()
    assert d.pop("model_type") == "led"
    assert d.pop("architectures") == ["LEDForConditionalGeneration"]
    d.pop("torch_dtype")
    hf = transformers.LEDForConditionalGeneration(transformers.LEDConfig(**d, attn_implementation="eager"))
    missing, unexpected = hf.load_state_dict(to_hf_state_dict(model), strict=False)
    assert set(missing) <= _TIED, missing  # transformers ties these to `led.shared`
    assert not unexpected, unexpected
    return hf


def _pair():
    torch.manual_seed(0)
    ours = build_model("led-tiny").eval()
    with torch.no_grad():  # the global projections and the logits bias take part (zero-initialised they would not)
        ours.final_logits_bias.normal_(0.0, 0.5)
    return ours, _hf_for(ours).eval()


def _batch(V, globs, B=2, S=23, T=9, pad_id=1):
    """23 source tokens (not a multiple of the window 8), row 1 padded from token 17 on; ``globs[b]``: the global
    tokens of row b."""
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, V, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    am[1, 17:] = 0
    ids[1, 17:] = pad_id
    labels = torch.randint(3, V, (B, T), generator=g)
    labels[0, -2:] = -100
    gm = torch.zeros(B, S, dtype=torch.long)
    for b, gs in enumerate(globs):
        gm[b, list(gs)] = 1
    return ids, am, labels, gm


class _GradView:
    def __init__(self, m):
        self.config = m.config
        self._m = m

    def state_dict(self):
        return {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in self._m.named_parameters()}


CASES = {"token 0": ((0,), (0,)), "two in one row": ((0, 13), (0,))}


@pytest.mark.parametrize("case", list(CASES))
def test_forward_backward_matches_hf(case):
    ours, hf = _pair()
    assert ours.config.attention_window == [8, 8]
    ids, am, labels, gm = _batch(ours.config.vocab_size, CASES[case])
    out = ours(input_ids=ids, attention_mask=am, labels=labels, return_logits=True, global_attention_mask=gm)
    ref = hf(input_ids=ids, attention_mask=am, labels=labels, global_attention_mask=gm)
    torch.testing.assert_close(out.logits, ref.logits, atol=2e-5, rtol=1e-4)
    torch.testing.assert_close(out.loss, ref.loss, atol=2e-5, rtol=1e-5)
    valid = am.bool()
    torch.testing.assert_close(out.encoder_last_hidden_state[valid], ref.encoder_last_hidden_state[valid],
                               atol=2e-5, rtol=1e-4)
    out.loss.backward()
    ref.loss.backward()
    mapped = to_hf_state_dict(_GradView(ours))
    hf_named = dict(hf.named_parameters())
    checked, glob_checked = 0, 0
    for k, g in mapped.items():
        assert k in hf_named, k
        assert hf_named[k].grad is not None, k
        torch.testing.assert_close(g, hf_named[k].grad, atol=5e-5, rtol=1e-3, msg=k)
        checked += 1
        if "_global." in k:
            assert g.abs().max().item() > 0 and hf_named[k].grad.abs().max().item() > 0, k
            glob_checked += 1
    assert checked == len(hf_named) and glob_checked == 2 * 3 * ours.config.num_layers  # weight + bias, q / k / v


def test_mask_and_index_name_the_same_tokens():
    ours, _ = _pair()
    ids, am, labels, gm = _batch(ours.config.vocab_size, CASES["two in one row"])
    gi = torch.tensor([[0, 13], [0, -1]])
    a = ours(input_ids=ids, attention_mask=am, labels=labels, return_logits=True, global_attention_mask=gm)
    b = ours(input_ids=ids, attention_mask=am, labels=labels, return_logits=True, global_index=gi)
    c = ours(input_ids=ids, attention_mask=am, labels=labels, return_logits=True, global_attention_mask=gm,
             global_index=gi)
    for o in (b, c):
        assert torch.equal(a.logits, o.logits) and torch.equal(a.encoder_last_hidden_state, o.encoder_last_hidden_state)
    assert torch.equal(ours.encode(ids, am, global_attention_mask=gm), a.encoder_last_hidden_state)
    # no global token: None, an all-zero mask and an all -1 index are the same windowed encoder
    none = ours.encode(ids, am)
    assert torch.equal(none, ours.encode(ids, am, global_attention_mask=torch.zeros_like(gm)))
    assert torch.equal(none, ours.encode(ids, am, global_index=torch.full((2, 1), -1)))
    assert not torch.equal(none, a.encoder_last_hidden_state)
    with pytest.raises(ValueError, match="LED"):
        build_model("bart-tiny").eval()(input_ids=ids, attention_mask=am, labels=labels, global_attention_mask=gm)


def test_collator_emits_mask_and_index():
    ours, _ = _pair()
    col = DataCollatorForSeq2Seq.for_model(ours)
    feats = [{"input_ids": list(range(3, 20)), "labels": [5, 6, 7]},
             {"input_ids": list(range(3, 12)), "labels": [8, 9]}]
    batch = col(feats)
    assert batch["global_attention_mask"].shape == (2, 17) and batch["global_attention_mask"].dtype == torch.int64
    assert batch["global_attention_mask"][:, 0].tolist() == [1, 1] and batch["global_attention_mask"].sum().item() == 2
    assert batch["global_index"].tolist() == [[0], [0]] and batch["global_index"].dtype == torch.int64
    out = ours(**batch)  # the batch is the model's keyword arguments as it stands
    assert torch.isfinite(out.loss)
    assert "global_attention_mask" not in DataCollatorForSeq2Seq.for_model(build_model("bart-tiny"))(feats)


def test_the_window_matters():
    """A far token does not reach a non-global position (2 layers x 4 keys on either side), and it does once token 0
    is global: position 0 then reads every token, and every position reads position 0."""
    ours, _ = _pair()
    ids, am, _, gm = _batch(ours.config.vocab_size, CASES["token 0"])
    ids2 = ids.clone()
    ids2[0, 22] = (ids2[0, 22] + 1) % ours.config.vocab_size
    reach = (ours.config.attention_window[0] // 2) * ours.config.num_layers  # 8
    a, b = ours.encode(ids, am), ours.encode(ids2, am)
    assert torch.equal(a[0, :22 - reach], b[0, :22 - reach])
    assert not torch.equal(a[0, 22 - reach:], b[0, 22 - reach:])
    a, b = (ours.encode(x, am, global_attention_mask=gm) for x in (ids, ids2))
    assert not torch.equal(a[0, 0], b[0, 0])   # the global row attends to everything
    assert not torch.equal(a[0, 5], b[0, 5])   # and a far position reads it in the next layer
    assert torch.equal(a[1], b[1])


def test_module_names_mirror_hf():
    ours, hf = _pair()
    names = set(to_hf_state_dict(ours))
    att = "led.encoder.layers.{}.self_attn.longformer_self_attn.{}.{}"
    for n in range(2):
        for w in ("query", "key", "value", "query_global", "key_global", "value_global"):
            for t in ("weight", "bias"):
                assert att.format(n, w, t) in names
        assert f"led.encoder.layers.{n}.self_attn.output.weight" in names
        for w in ("q_proj", "k_proj", "v_proj", "out_proj"):
            assert f"led.decoder.layers.{n}.self_attn.{w}.weight" in names
            assert f"led.decoder.layers.{n}.encoder_attn.{w}.weight" in names
    for k in ("led.shared.weight", "led.encoder.embed_positions.weight", "led.decoder.embed_positions.weight",
              "led.encoder.layernorm_embedding.weight", "led.decoder.layernorm_embedding.bias", "final_logits_bias"):
        assert k in names
    assert names == set(hf.state_dict()) - _TIED
    assert hf.state_dict()["led.encoder.embed_positions.weight"].shape == (256, 64)
    assert hf.state_dict()["led.decoder.embed_positions.weight"].shape == (64, 64)


@pytest.mark.parametrize("name", ["led-tiny", "led-base-16384", "led-large-16384"])
def test_config_round_trip(name, tmp_path):
    cfg = PRESETS[name]
    cfg.save(str(tmp_path))
    with open(os.path.join(tmp_path, "config.json")) as f:
        d = json.load(f)
    assert d["model_type"] == "led" and d["architectures"] == ["LEDForConditionalGeneration"]
    assert d["attention_window"] == cfg.attention_window and len(d["attention_window"]) == cfg.num_layers
    assert d["max_encoder_position_embeddings"] == cfg.max_encoder_position_embeddings
    assert d["max_decoder_position_embeddings"] == cfg.max_position_embeddings
    assert "max_position_embeddings" not in d
    back = resolve_config(str(tmp_path))
    a, b = cfg.to_dict(), back.to_dict()
    for k in a:
        if k not in ("name", "generation"):
            assert a[k] == b[k], k
    d["attention_window"] = 16  # an int is accepted and expanded
    assert Seq2SeqConfig.from_hf_dict(d).attention_window == [16] * cfg.num_layers
    for bad in (7, 0, [8] * (cfg.num_layers + 1)):
        d["attention_window"] = bad
        with pytest.raises(ValueError, match="attention_window"):
            Seq2SeqConfig.from_hf_dict(d)


def test_presets_have_the_published_shapes():
    b, l = PRESETS["led-base-16384"], PRESETS["led-large-16384"]
    assert (b.d_model, b.num_heads, b.num_layers, b.num_decoder_layers, b.d_ff) == (768, 12, 6, 6, 3072)
    assert (l.d_model, l.num_heads, l.num_layers, l.num_decoder_layers, l.d_ff) == (1024, 16, 12, 12, 4096)
    for c in (b, l):
        assert c.vocab_size == 50265 and c.d_kv == 64 and c.attention_window == [1024] * c.num_layers
        assert c.max_encoder_position_embeddings == 16384 and c.max_position_embeddings == 1024
        assert c.position_embedding == "learned0" and c.layernorm_embedding and not c.normalize_before
        assert c.final_logits_bias
    t = PRESETS["led-tiny"]
    assert t.attention_window == [8, 8] and t.d_kv == 16 and (t.num_layers, t.num_decoder_layers) == (2, 2)
    assert resolve_config("allenai/led-base-16384").d_model == 768
    assert "attention_window" not in PRESETS["bart-base"].to_hf_dict()  # BART configs do not grow LED keys


def test_from_pretrained_reads_transformers_save_pretrained(tmp_path):
    ours, hf = _pair()
    hf.save_pretrained(str(tmp_path), safe_serialization=True)
    back = from_pretrained(str(tmp_path))
    assert back.config.model_type == "led" and back.config.attention_window == [8, 8]
    a, b = ours.state_dict(), back.state_dict()
    assert a.keys() == b.keys()
    for k in a:
        torch.testing.assert_close(a[k], b[k], atol=0, rtol=0, msg=k)


def test_transformers_loads_our_save_pretrained(tmp_path):
    import transformers
    ours, _ = _pair()
    save_pretrained(ours, str(tmp_path))
    hf = transformers.AutoModelForSeq2SeqLM.from_pretrained(str(tmp_path), attn_implementation="eager").eval()
    assert type(hf).__name__ == "LEDForConditionalGeneration"
    assert hf.config.attention_window == [8, 8] and hf.config.max_encoder_position_embeddings == 256
    ids, am, labels, gm = _batch(ours.config.vocab_size, CASES["two in one row"])
    out = ours(input_ids=ids, attention_mask=am, labels=labels, return_logits=True, global_attention_mask=gm)
    ref = hf(input_ids=ids, attention_mask=am, labels=labels, global_attention_mask=gm)
    torch.testing.assert_close(out.logits, ref.logits, atol=2e-5, rtol=1e-4)


def _through_eos(seq, eos, pad):
    """``seq`` with everything after each row's first eos (past the start token) replaced by ``pad``."""
    done = ((seq[:, 1:] == eos).long().cumsum(1) > 0).long().cumsum(1) > 1
    out = seq.clone()
    out[:, 1:][done] = pad
    return out


@pytest.mark.parametrize("beams", [1, 2])
def test_generate_matches_hf(beams):
    ours, hf = _pair()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(4, ours.config.vocab_size, (3, 23), generator=g)
    am = torch.ones_like(ids)
    am[2, 17:] = 0
    ids[2, 17:] = ours.config.pad_token_id
    gm = torch.zeros_like(ids)
    gm[:, 0] = 1
    kw = dict(max_length=12, num_beams=beams, min_length=0, no_repeat_ngram_size=0, length_penalty=1.0,
              early_stopping=False)
    a = ours.generate(ids, attention_mask=am, global_attention_mask=gm, **kw)
    b = hf.generate(ids, attention_mask=am, global_attention_mask=gm, do_sample=False, **kw)
    L = min(a.shape[1], b.shape[1])
    eos, pad = ours.config.eos_token_id, ours.config.pad_token_id
    assert torch.equal(_through_eos(a[:, :L], eos, pad), _through_eos(b[:, :L], eos, pad)), (a, b)
    assert torch.equal(_through_eos(a, eos, pad), a)
    assert torch.equal(a, ours.generate(ids, attention_mask=am, global_index=torch.zeros(3, 1, dtype=torch.long), **kw))


def test_what_led_does_not_implement():
    ours, _ = _pair()
    with pytest.raises(NotImplementedError, match="LED"):
        ours.enable_context_parallel(None)
    ours.enable_context_parallel(enable=False)  # switching it off stays harmless
    ids, am, labels, gm = _batch(ours.config.vocab_size, CASES["token 0"])
    seg = torch.zeros_like(ids)
    dseg = torch.zeros_like(labels)
    with pytest.raises(NotImplementedError, match="LED"):
        ours(input_ids=ids, attention_mask=am, labels=labels, decoder_input_ids=labels.clamp_min(0), segment_ids=seg,
             decoder_segment_ids=dseg, position_ids=seg, decoder_position_ids=dseg)
    with pytest.raises(NotImplementedError, match="LED"):
        ours.encode(ids, am, seg=(seg, seg))
    with pytest.raises(NotImplementedError, match="LED"):
        DataCollatorForSeq2Seq.for_model(ours)([{"input_ids": [3, 4], "segment_ids": [0, 0]}])
    long = torch.full((1, ours.config.max_encoder_position_embeddings + 1), 5)
    with pytest.raises(ValueError, match="max_encoder_position_embeddings"):
        ours.encode(long)


def test_long_inputs_are_not_chunked(monkeypatch):
    """Above attn_chunk_min the plain T5 encoder chunks its self-attention; LED's encoder keeps one windowed call per
    layer at the full length, with the global keys, and one call for the global rows."""
    from distributed_llms_example_amd.ops import attention as A, routing
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(attn_chunk_min=16, attn_chunk=8))
    ours, _ = _pair()
    calls, rows = [], []
    qkv_call, q_kv_call = A.attention_qkv, A.attention_q_kv
    monkeypatch.setattr(A, "attention_qkv", lambda qkv, **kw: (
        calls.append((qkv.shape[1], kw.get("window"), kw.get("global_keys") is not None)), qkv_call(qkv, **kw))[1])
    monkeypatch.setattr(A, "attention_q_kv", lambda q, kv, **kw: (
        rows.append((q.shape[1], kv.shape[1], kw.get("window"))), q_kv_call(q, kv, **kw))[1])
    ids, am, _, gm = _batch(ours.config.vocab_size, CASES["two in one row"])
    ours.encode(ids, am, global_attention_mask=gm)
    assert calls == [(23, 4, True)] * ours.config.num_layers
    assert rows == [(2, 23, None)] * ours.config.num_layers


def test_evaluation_scores_led_with_its_global_first_token(monkeypatch):
    """train/evaluation.py generates for LED with the collator's recipe (token 0 global), and for BART without."""
    from distributed_llms_example_amd.data.tokenization import WordTokenizer
    from distributed_llms_example_amd.train.evaluation import calculate_metric_on_test_ds
    ds = {"article": ["the cat sat on the mat", "a dog ran in the park", "birds fly south"],
          "highlights": ["cat on mat", "dog in park", "birds fly"]}
    tok = WordTokenizer.build(ds["article"] + ds["highlights"], 500)
    for name, led in (("led-tiny", True), ("bart-tiny", False)):
        torch.manual_seed(0)
        m = build_model(name)
        seen = []
        real = m.generate
        monkeypatch.setattr(m, "generate", lambda ids, **kw: (seen.append((ids.shape[0], kw.get("global_index"))),
                                                              real(ids, **kw))[1])
        scores = calculate_metric_on_test_ds(m, tok, ds, batch_size=2, max_source_length=16, num_beams=2, max_length=6)
        assert set(scores) >= {"rouge1", "rougeL"} and [n for n, _ in seen] == [2, 1]
        for n, gi in seen:
            assert (gi is not None and gi.tolist() == [[0]] * n) if led else gi is None
