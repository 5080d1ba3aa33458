"""Sequence packing on the CPU path: the packer's invariants (data/packing.py), a packed batch against the same examples
padded (loss and every parameter gradient, models/t5.py and models/bart.py with segment ids on the composite),
isolation between the examples of one row, the --pack-sequences flag through an entry point, and what packing
rejects."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_llms_example_amd.data.collator import DataCollatorForSeq2Seq
from distributed_llms_example_amd.data.packing import (first_fit_decreasing, pack_examples, pack_features,
                                                       unpad_features)
from distributed_llms_example_amd.models import build_model, resolve_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _examples(lens, vocab=500, seed=0, lo=4):
    rng = np.random.default_rng(seed)
    return [(rng.integers(lo, vocab, size=s), rng.integers(lo, vocab, size=t)) for s, t in lens]


# ------------------------------------------------------------------------------------------------------- the packer
def test_packer_invariants():
    rng = np.random.default_rng(1)
    lens = [(int(s), int(t)) for s, t in zip(rng.integers(1, 60, 200), rng.integers(1, 14, 200))]
    ex = _examples(lens, seed=2)
    S, T = 64, 16
    pk = pack_examples(ex, S, T, pad_token_id=0, decoder_start_token_id=3, seed=5)
    a = pk.arrays
    assert sorted(i for r in pk.rows for i in r) == list(range(200))  # every example exactly once
    assert pk.num_examples == 200 and len(pk) == len(pk.rows) < 200
    for r, members in enumerate(pk.rows):
        assert sum(len(ex[i][0]) for i in members) <= S and sum(len(ex[i][1]) for i in members) <= T
        for seg, cap in ((a["segment_ids"][r], S), (a["decoder_segment_ids"][r], T)):
            n = int((seg >= 0).sum())
            assert (seg[:n] >= 0).all() and (seg[n:] == -1).all()       # a -1 tail only
            assert (np.diff(seg[:n]) >= 0).all() and seg[0] == 0        # 0, 1, 2, ... non-decreasing
            assert set(seg[:n]) == set(range(len(members)))
        so = to = 0
        for g, i in enumerate(members):
            s, t = ex[i]
            assert (a["input_ids"][r, so:so + len(s)] == s).all()
            assert (a["position_ids"][r, so:so + len(s)] == np.arange(len(s))).all()
            assert (a["labels"][r, to:to + len(t)] == t).all()
            # decoder inputs per segment as the collator builds them per row: start token, then the shifted labels
            assert a["decoder_input_ids"][r, to] == 3
            assert (a["decoder_input_ids"][r, to + 1:to + len(t)] == t[:-1]).all()
            assert (a["decoder_position_ids"][r, to:to + len(t)] == np.arange(len(t))).all()
            so, to = so + len(s), to + len(t)
        assert (a["labels"][r, to:] == -100).all() and (a["input_ids"][r, so:] == 0).all()
        assert (a["attention_mask"][r] == (a["segment_ids"][r] >= 0)).all()
    assert pk.source_tokens == sum(s for s, _ in lens)
    assert abs(pk.efficiency - pk.source_tokens / (len(pk) * S)) < 1e-12 and 0.5 < pk.efficiency <= 1.0
    again = pack_examples(ex, S, T, pad_token_id=0, decoder_start_token_id=3, seed=5)
    assert again.rows == pk.rows and all((again.arrays[k] == a[k]).all() for k in a)  # same seed, same rows


def test_packer_needs_both_source_and_target_room():
    """Sources of 10 fit six to a 64-token row, but targets of 8 only two to a 16-token row."""
    rows = first_fit_decreasing([10] * 6, [8] * 6, 64, 16)
    assert [len(r) for r in rows] == [2, 2, 2]
    with pytest.raises(ValueError):
        first_fit_decreasing([65], [1], 64, 16)


def test_unpad_and_collate_round_trip():
    from distributed_llms_example_amd.data.dataset import Seq2SeqFeatures
    ids = np.array([[5, 6, 7, 0, 0], [8, 9, 0, 0, 0]])
    am = (ids != 0).astype(np.int8)
    labels = np.array([[11, 12, 0], [13, 0, 0]])  # padded with the pad id (the default) ...
    ex = unpad_features(Seq2SeqFeatures(ids, am, labels), 0)
    assert [list(s) for s, _ in ex] == [[5, 6, 7], [8, 9]] and [list(t) for _, t in ex] == [[11, 12], [13]]
    ex2 = unpad_features(Seq2SeqFeatures(ids, am, np.where(labels == 0, -100, labels)), 0)  # ... or with -100
    assert [list(t) for _, t in ex2] == [[11, 12], [13]]
    cfg = resolve_config("t5-tiny")
    pk = pack_features(Seq2SeqFeatures(ids, am, labels), cfg, 8, 4)
    batch = DataCollatorForSeq2Seq.for_model(cfg)([pk[i] for i in range(len(pk))])
    assert set(batch) == set(pk.arrays) and all(v.dtype == torch.int64 for v in batch.values())
    assert batch["input_ids"].tolist() == [[5, 6, 7, 8, 9, 0, 0, 0]]
    assert batch["labels"].tolist() == [[11, 12, 13, -100]]  # pad labels are not trained on


# ------------------------------------------------------------------------------------------------------ model parity
# boundaries mid-row, one row with a padded tail, one single-token target
LENS = [(9, 4), (5, 1), (7, 3), (12, 5), (3, 2)]
MODELS = ["t5-tiny", "t5-tiny-gated", "umt5-tiny", "bart-tiny", "pegasus-tiny", "m2m100-tiny", "blenderbot-tiny"]


def _padded_batch(ex, cfg):
    feats = [{"input_ids": s, "attention_mask": np.ones(len(s), np.int64), "labels": t} for s, t in ex]
    return DataCollatorForSeq2Seq.for_model(cfg)(feats)  # labels padded with -100: pad labels ignored


def _packed_batch(ex, cfg, S=24, T=10):
    pk = pack_examples(ex, S, T, cfg.pad_token_id, cfg.decoder_start_token_id, shift_mode=cfg.shift_mode)
    assert len(pk) == 2 and sorted(len(r) for r in pk.rows) == [2, 3]
    assert (pk.arrays["segment_ids"][:, -1] == -1).any()  # a row with a padded tail
    return DataCollatorForSeq2Seq.for_model(cfg)([pk[i] for i in range(len(pk))]), pk


def _loss_and_grads(model, batch):
    model.zero_grad()
    extra = {k: batch[k] for k in ("segment_ids", "decoder_segment_ids", "position_ids", "decoder_position_ids")
             if k in batch}
    out = model(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"],
                decoder_input_ids=batch["decoder_input_ids"], labels=batch["labels"], **extra)
    out.loss.backward()
    return out.loss.detach(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("name", MODELS)
def test_packed_batch_matches_padded_batch(name):
    """Loss (mean over the same non-ignored labels) and every parameter gradient of one packed batch against the same
    examples in an ordinary padded batch with pad labels ignored, at the bounds tests/test_longt5_cpu.py holds this
    framework to against transformers: 2e-5 / 1e-4 on the loss, 5e-5 / 1e-3 on gradients."""
    cfg = resolve_config(name)
    torch.manual_seed(0)
    model = build_model(cfg).eval()
    ex = _examples(LENS, seed=3)
    padded = _padded_batch(ex, cfg)
    packed, _ = _packed_batch(ex, cfg)
    assert (packed["labels"] != -100).sum() == (padded["labels"] != -100).sum() == sum(t for _, t in LENS)
    l0, g0 = _loss_and_grads(model, padded)
    l1, g1 = _loss_and_grads(model, packed)
    print(f"[{name}] loss padded {l0.item():.6f} packed {l1.item():.6f}")
    torch.testing.assert_close(l1, l0, atol=2e-5, rtol=1e-4)
    assert set(g0) == set(g1)
    for n in g0:
        torch.testing.assert_close(g1[n], g0[n], atol=5e-5, rtol=1e-3, msg=lambda m, n=n: f"{name} {n}: {m}")


@pytest.mark.parametrize("name", ["t5-tiny", "bart-tiny"])
def test_examples_of_one_row_are_isolated(name):
    """Changing one example's tokens leaves the encoder states of another example of the same row bit-identical."""
    cfg = resolve_config(name)
    torch.manual_seed(0)
    model = build_model(cfg).eval()
    batch, pk = _packed_batch(_examples(LENS, seed=3), cfg)
    r = [i for i, m in enumerate(pk.rows) if len(m) == 3][0]
    seg = batch["segment_ids"]
    other = batch["input_ids"].clone()
    other[r][seg[r] == 1] = (other[r][seg[r] == 1] + 7) % 400 + 4
    assert not torch.equal(other, batch["input_ids"])
    outs = []
    with torch.no_grad():
        for ids in (batch["input_ids"], other):
            outs.append(model(input_ids=ids, attention_mask=batch["attention_mask"],
                              decoder_input_ids=batch["decoder_input_ids"], labels=batch["labels"],
                              segment_ids=seg, decoder_segment_ids=batch["decoder_segment_ids"],
                              position_ids=batch["position_ids"],
                              decoder_position_ids=batch["decoder_position_ids"]).encoder_last_hidden_state)
    keep = seg[r] != 1
    assert torch.equal(outs[0][r][keep & (seg[r] >= 0)], outs[1][r][keep & (seg[r] >= 0)])
    assert not torch.equal(outs[0][r][seg[r] == 1], outs[1][r][seg[r] == 1])


def test_global_token_normalisation_counts_packed_labels():
    """D8 (train/engine.py token_count) counts non-ignored labels: on packed rows, the examples' target tokens."""
    from distributed_llms_example_amd.train.engine import token_count
    cfg = resolve_config("t5-tiny")
    batch, _ = _packed_batch(_examples(LENS, seed=3), cfg)
    assert int(token_count(batch["labels"])) == sum(t for _, t in LENS)


# --------------------------------------------------------------------------------------------------------- rejections
def _packed_kwargs(cfg):
    batch, _ = _packed_batch(_examples(LENS, seed=3), cfg)
    return {k: v for k, v in batch.items()}


def test_longt5_rejects_packed_inputs():
    cfg = resolve_config("longt5-tiny")
    kw = _packed_kwargs(cfg)
    with pytest.raises(NotImplementedError, match="LongT5"):
        build_model(cfg).eval()(**kw)


def test_context_parallel_rejects_packed_inputs():
    cfg = resolve_config("t5-tiny")
    kw = _packed_kwargs(cfg)
    model = build_model(cfg).eval()
    model.encoder._cp_group = None  # what enable_context_parallel(None) sets: sharded over the default group
    with pytest.raises(NotImplementedError, match="context parallel"):
        model(**kw)


def test_packed_inputs_come_complete():
    cfg = resolve_config("t5-tiny")
    kw = _packed_kwargs(cfg)
    model = build_model(cfg).eval()
    with pytest.raises(ValueError, match="both"):
        model(**{k: v for k, v in kw.items() if k != "decoder_segment_ids"})
    with pytest.raises(ValueError, match="decoder_input_ids"):
        model(**{k: v for k, v in kw.items() if k != "decoder_input_ids"})
    bart = build_model(resolve_config("bart-tiny")).eval()
    with pytest.raises(ValueError, match="position_ids"):
        bart(**{k: v for k, v in _packed_kwargs(bart.config).items() if k != "position_ids"})


def test_cli_rejects_packing_for_longt5_and_context_parallel():
    from distributed_llms_example_amd import cli
    ap = cli.base_parser("t")
    common = ["--synthetic", "8", "--max-source-length", "40", "--max-target-length", "10", "--pack-sequences"]
    a = ap.parse_args(["--model-ckpt", "longt5-tiny"] + common)
    with pytest.raises(NotImplementedError, match="LongT5"):
        cli.build_data(a, cli.model_config(a))
    a = ap.parse_args(["--model-ckpt", "t5-tiny", "--context-parallel", "2"] + common)
    with pytest.raises(NotImplementedError, match="context-parallel"):
        cli.build_data(a, cli.model_config(a))
    assert ap.parse_args([]).pack_sequences is False  # off by default


# ------------------------------------------------------------------------------------------------------- entry point
def test_pack_sequences_through_train_torchrun(tmp_path):
    """--pack-sequences on synthetic SAMSum records with gradient accumulation 2: rows, not examples, are the samples
    of steps and schedules, and the final log adds examples per second and the packing efficiency."""
    env = dict(os.environ)
    env.update({"VH_ROOT": str(tmp_path), "DLLM_FORCE_CPU": "1", "OMP_NUM_THREADS": "2", "PYTHONPATH": ROOT})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train-torchrun.py"), "--model-ckpt", "t5-tiny",
                        "--output-dir", "out", "--batch-size", "2", "--grad-accum", "2", "--evaluation-steps", "100",
                        "--warmup-steps", "1", "--synthetic", "48", "--max-source-length", "256",
                        "--max-target-length", "48", "--gen-max-length", "8", "--max-eval-samples", "4",
                        "--pack-sequences"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    logs = [json.loads(x) for x in r.stdout.splitlines() if x.strip().startswith("{")]
    final = [x for x in logs if "train_samples_per_second" in x][-1]
    assert final["train_loss"] > 0 and final["batch_shape"] == [2, 256, 48]
    assert final["packing_examples_per_row"] > 1.5 and 0 < final["packing_efficiency"] <= 1
    assert final["train_examples_per_second"] > final["train_samples_per_second"]
