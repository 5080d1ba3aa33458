"""Sampling and the repetition penalty of models/generation.py on CPU: the torch composite against transformers'
processors and warpers, generate() against transformers' generate(), the counter-based draw and its statistics."""
import itertools
import logging

import pytest
import torch

from distributed_llms_example_amd.models import build_model
from distributed_llms_example_amd.models import generation as gen
from hf_oracle import hf_model_for

NINF = float("-inf")


def _prefix(rows, V, g):
    """Decoder prefixes of length 7 with repeated tokens."""
    p = torch.randint(0, V, (rows, 7), generator=g)
    p[:, 4] = p[:, 1]
    p[:, 6] = p[:, 0]
    return p


def _fp64_margin(logits, prefix, T, k, p, r):
    """fp64 evaluation of the chain: (scores distinct on every row, smallest distance between top_p and the mass of
    the strictly larger scores over every top-k survivor but the maximum, which is kept whatever its mass)."""
    x = logits.double()
    s = x.gather(1, prefix)
    x = x.scatter(1, prefix, torch.where(s < 0, s * r, s / r)) / T
    distinct = all(row.unique().numel() == row.numel() for row in x)
    V = x.shape[1]
    if 0 < k < V:
        x = x.masked_fill(x < x.topk(k, dim=1).values[:, -1:], NINF)
    srt = x.sort(dim=1, descending=True).values
    cum = srt.softmax(1).cumsum(1)
    above = cum[:, :-1]  # mass of the strictly larger scores of sort positions 1 ..
    live = torch.isfinite(srt[:, 1:])
    d = (above - p).abs()[live]
    return distinct, (float(d.min()) if d.numel() else float("inf"))


def _inputs(rows, V, T, k, p, r):
    """Seeded logits and prefixes: the first seed at which the scores are distinct and the top-p boundary is at least
    1e-3 of mass away from top_p on every row (the tests assert it again before they compare)."""
    for seed in range(200):
        g = torch.Generator().manual_seed(1000 * V + seed)
        logits = torch.randn(rows, V, generator=g) * 4.0
        prefix = _prefix(rows, V, g)
        distinct, margin = _fp64_margin(logits, prefix, T, k, p, r)
        if distinct and (p >= 1.0 or margin >= 1e-3):
            return logits, prefix
    raise AssertionError("no seed with a clear top-p boundary")


def _hf_chain(logits, prefix, T, k, p, r):
    from transformers.generation.logits_process import (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper)
    x = RepetitionPenaltyLogitsProcessor(penalty=r)(prefix, logits.clone())
    x = TemperatureLogitsWarper(T)(prefix, x)
    if k > 0:  # transformers builds no top-k warper for 0
        x = TopKLogitsWarper(top_k=k)(prefix, x)
    return TopPLogitsWarper(top_p=p)(prefix, x)


@pytest.mark.parametrize("rows,V", [(4, 97), (3, 1000)])
def test_composite_filter_matches_transformers(rows, V):
    for k, p, T, r in itertools.product([0, 1, 5, V + 3], [1.0, 0.9, 0.3, 1e-6], [1.0, 0.7], [1.0, 1.3]):
        logits, prefix = _inputs(rows, V, T, k, p, r)
        distinct, margin = _fp64_margin(logits, prefix, T, k, p, r)
        assert distinct and (p >= 1.0 or margin >= 1e-3), (k, p, T, r, margin)
        ours = gen._warp(gen._penalize(logits.clone(), prefix, prefix.shape[1], r), T, k, p)
        ref = _hf_chain(logits, prefix, T, k, p, r)
        kept, kept_ref = torch.isfinite(ours), torch.isfinite(ref)
        assert torch.equal(kept, kept_ref), (k, p, T, r, kept.sum(1), kept_ref.sum(1))
        assert kept.any(1).all()
        torch.testing.assert_close(ours[kept], ref[kept], rtol=0, atol=1e-6)


def test_all_equal_row_keeps_every_tie():
    x = torch.full((2, 50), 1.25)
    for k, p in [(5, 1.0), (5, 0.3), (0, 0.3), (1, 1e-6)]:
        out = gen._warp(x.clone(), 0.7, k, p)
        assert torch.isfinite(out).all(), (k, p)


def test_row_with_one_unbanned_token():
    x = torch.full((3, 64), NINF)
    x[0, 17], x[1, 0], x[2, 63] = 0.3, -2.0, 5.0
    out = gen._warp(x.clone(), 0.7, 5, 0.9)
    assert torch.equal(torch.isfinite(out), torch.isfinite(x))
    assert gen._gumbel_argmax(out, 11, 3).tolist() == [17, 0, 63]


def _pair(name):
    """Our tiny model and transformers' with the same weights.  The layer weights are scaled by 8: at the initial
    scale the layers are near the identity, the last token's own embedding dominates the logits by more than any
    penalty moves, and greedy bart-tiny emits one token whatever the penalty."""
    torch.manual_seed(0)
    ours = build_model(name).eval()
    with torch.no_grad():
        if hasattr(ours, "lm_head"):
            ours.lm_head.weight.copy_(ours.shared.weight)
        for n, p in ours.named_parameters():
            if p.dim() >= 2 and "shared" not in n and "embed" not in n and "lm_head" not in n:
                p.mul_(8.0)
    return ours, hf_model_for(ours).eval()


@pytest.mark.parametrize("name", ["t5-tiny", "bart-tiny"])
@pytest.mark.parametrize("beams", [1, 2])
def test_generate_repetition_penalty_matches_hf(name, beams):
    ours, hf = _pair(name)
    ids = torch.randint(4, ours.config.vocab_size, (3, 17), generator=torch.Generator().manual_seed(1))
    am = torch.ones_like(ids)
    kw = dict(max_length=12, num_beams=beams, min_length=0, no_repeat_ngram_size=0, length_penalty=1.0,
              early_stopping=False)
    extra = {}
    if ours.config.model_type != "t5":
        extra = dict(forced_bos_token_id=ours.config.forced_bos_token_id,
                     forced_eos_token_id=ours.config.forced_eos_token_id)
    a = ours.generate(ids, attention_mask=am, repetition_penalty=1.3, **kw)
    b = hf.generate(ids, attention_mask=am, do_sample=False, repetition_penalty=1.3, **kw, **extra)
    L = min(a.shape[1], b.shape[1])
    assert torch.equal(a[:, :L], b[:, :L]), (a, b)
    plain = ours.generate(ids, attention_mask=am, **kw)
    assert plain.shape != a.shape or not torch.equal(plain, a)  # the option acts on this input


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    m = build_model("t5-tiny").eval()
    ids = torch.randint(4, m.config.vocab_size, (3, 12), generator=torch.Generator().manual_seed(1))
    return m, ids


def test_sampling_seeds(tiny):
    m, ids = tiny
    kw = dict(max_length=24, do_sample=True, top_k=50, top_p=0.9, temperature=0.7)
    a = m.generate(ids, seed=5, **kw)
    b = m.generate(ids, seed=5, **kw)
    c = m.generate(ids, seed=6, **kw)
    assert torch.equal(a, b)
    assert a.shape != c.shape or not torch.equal(a, c)
    # no seed: the default seed stream moves on between calls
    d, e = m.generate(ids, **kw), m.generate(ids, **kw)
    assert d.shape != e.shape or not torch.equal(d, e)


@pytest.mark.parametrize("opt", [dict(top_k=1), dict(top_k=0, top_p=1e-6)])
def test_sampling_degenerates_to_greedy(tiny, opt):
    m, ids = tiny
    greedy = m.generate(ids, max_length=24, repetition_penalty=1.2)
    got = m.generate(ids, max_length=24, repetition_penalty=1.2, do_sample=True, temperature=0.7, seed=3, **opt)
    assert torch.equal(greedy, got)


def test_every_drawn_token_is_kept(tiny, monkeypatch):
    m, ids = tiny
    steps = []
    orig = gen._sample_step

    def spy(logits, seqs, cur, proc, penalty, temperature, top_k, top_p, seed, step):
        tok = orig(logits, seqs, cur, proc, penalty, temperature, top_k, top_p, seed, step)
        kept = torch.isfinite(gen._sample_scores(logits, seqs, cur, proc, penalty, temperature, top_k, top_p))
        assert kept.gather(1, tok.view(-1, 1)).all()
        steps.append(int(kept.sum(1).max()))
        return tok

    monkeypatch.setattr(gen, "_sample_step", spy)
    m.generate(ids, max_length=24, do_sample=True, top_k=20, top_p=0.8, temperature=1.5, repetition_penalty=1.2,
               no_repeat_ngram_size=2, min_length=6, seed=9)
    assert len(steps) >= 6 and max(steps) > 1  # the draw had a choice


# 99.9 % quantiles of chi-square at 1 .. 12 degrees of freedom (standard table)
_CHI2_999 = [10.828, 13.816, 16.266, 18.467, 20.515, 22.458, 24.322, 26.124, 27.877, 29.588, 31.264, 32.909]


def _chi2_quantile_999(df):
    return _CHI2_999[df - 1]


def test_draw_statistics():
    """200 000 draws (2000 rows x 100 steps of the counter space) from one row of 40 logits under top_k=12,
    top_p=0.95 follow the softmax over the kept set.  Deterministic: seed 20261 (the first one tried)."""
    seed = 20261
    logits = torch.randn(1, 40, generator=torch.Generator().manual_seed(7)) * 1.5
    scores = gen._warp(logits, 1.0, 12, 0.95)
    kept = torch.isfinite(scores[0])
    n_kept = int(kept.sum())
    assert 5 <= n_kept <= 12
    rows, steps = 2000, 100
    counts = torch.zeros(40, dtype=torch.long)
    block = scores.expand(rows, 40).contiguous()
    for step in range(steps):
        counts += torch.bincount(gen._gumbel_argmax(block, seed, step), minlength=40)
    assert int(counts.sum()) == rows * steps and int(counts[~kept].sum()) == 0
    expect = scores[0, kept].double().softmax(0) * rows * steps
    chi2 = float(((counts[kept].double() - expect) ** 2 / expect).sum())
    print(f"chi2 = {chi2:.2f} at {n_kept - 1} degrees of freedom, bound {_chi2_quantile_999(n_kept - 1):.2f}")
    assert chi2 < _chi2_quantile_999(n_kept - 1)


def test_beam_sampling_raises(tiny):
    m, ids = tiny
    with pytest.raises(ValueError, match="beam sampling"):
        m.generate(ids, max_length=8, do_sample=True, num_beams=2)


def test_ignored_key_warns_once(tiny, caplog):
    m, ids = tiny
    gen._warned_keys.discard("encoder_no_repeat_ngram_size")
    with caplog.at_level(logging.WARNING, logger="distributed_llms_example_amd"):
        a = m.generate(ids, max_length=8, encoder_no_repeat_ngram_size=3, num_return_sequences=1, bad_words_ids=None)
        b = m.generate(ids, max_length=8, encoder_no_repeat_ngram_size=3)
    hits = [r for r in caplog.records if "encoder_no_repeat_ngram_size" in r.getMessage()]
    assert len(hits) == 1 and "num_return_sequences" not in hits[0].getMessage()
    assert torch.equal(a, b) and torch.equal(a, m.generate(ids, max_length=8))


def test_generation_config_keys_survive_a_checkpoint(tmp_path, tiny):
    """A saved generation_config.json hands repetition_penalty and the sampling keys back to generate()."""
    from distributed_llms_example_amd.models import resolve_config
    m, ids = tiny
    cfg = m.config.replace(generation={"repetition_penalty": 1.3, "do_sample": True, "top_k": 7, "top_p": 0.8,
                                       "temperature": 0.9, "max_length": 16})
    cfg.save(str(tmp_path))
    back = resolve_config(str(tmp_path)).generation
    assert back == cfg.generation
