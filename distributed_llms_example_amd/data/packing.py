"""Sequence packing: several examples per training row, told apart by segment ids.

The reference pads every example to ``max_source_length`` x ``max_target_length`` (data/dataset.py), and SAMSum
dialogues and summaries are a small fraction of those lengths, so most of a padded step is padding.  ``pack_features``
lays the unpadded examples into rows of that same shape, offline and deterministically (first-fit-decreasing by source
length): an example joins a row only if its source fits the row's remaining source tokens AND its target fits the
remaining target tokens.  Each row carries

* ``input_ids`` / ``segment_ids`` / ``position_ids`` ``[max_source_length]``: the examples' source tokens back to back,
  ids 0, 1, 2, ... in order (non-decreasing, what the kernels' block skipping is exact for), -1 on the padded tail,
  and each token's index within its example (0 on the tail);
* ``labels`` / ``decoder_input_ids`` / ``decoder_segment_ids`` / ``decoder_position_ids`` ``[max_target_length]``: the
  labels are each example's target ids and -100 everywhere else — packing implies that pad labels are not trained on —
  and the decoder inputs are built PER SEGMENT exactly as data/collator.py builds them per row: the start token, then
  the segment's labels shifted right (mBART-style models: the segment's last token first);
* ``attention_mask`` = ``segment_ids >= 0``.

The models confine attention to a segment (models/t5.py, models/bart.py ``segment_ids=``); steps, schedules and samplers
count rows.  Evaluation and generation stay unpacked.
"""
from __future__ import annotations

import numpy as np

PACKED_KEYS = ("segment_ids", "decoder_segment_ids", "position_ids", "decoder_position_ids")


def unpad_features(features, pad_token_id: int) -> list[tuple[np.ndarray, np.ndarray]]:
    """(source ids, target ids) of every example of right-padded ``features`` without the padding: source by its
    attention mask, target by its labels that are neither -100 nor the pad id."""
    out = []
    for i in range(len(features)):
        f = features[i]
        ids = np.asarray(f["input_ids"])
        n = int(np.asarray(f["attention_mask"]).sum()) if "attention_mask" in f else int((ids != pad_token_id).sum())
        lab = np.asarray(f["labels"])
        m = int(((lab != -100) & (lab != pad_token_id)).sum())
        out.append((ids[:n], lab[:m]))
    return out


def first_fit_decreasing(src_lens, tgt_lens, max_source_length: int, max_target_length: int, seed: int = 0):
    """Rows (lists of example indices, in packing order) by first-fit-decreasing on the source length; ties are broken
    by a permutation drawn from ``seed``, so the same seed gives the same rows."""
    src_lens, tgt_lens = np.asarray(src_lens), np.asarray(tgt_lens)
    n = len(src_lens)
    if n and (src_lens.max() > max_source_length or tgt_lens.max() > max_target_length):
        raise ValueError("pack: an example is longer than a row (truncate to the max lengths first)")
    tie = np.random.default_rng(seed).permutation(n)
    order = np.lexsort((tie, -src_lens))
    rem_s = np.empty(n, dtype=np.int64)
    rem_t = np.empty(n, dtype=np.int64)
    rows: list[list[int]] = []
    for i in order:
        ls, lt = int(src_lens[i]), int(tgt_lens[i])
        fit = np.flatnonzero((rem_s[: len(rows)] >= ls) & (rem_t[: len(rows)] >= lt))
        if len(fit):
            r = int(fit[0])
        else:
            r = len(rows)
            rows.append([])
            rem_s[r], rem_t[r] = max_source_length, max_target_length
        rows[r].append(int(i))
        rem_s[r] -= ls
        rem_t[r] -= lt
    return rows


class PackedSeq2SeqFeatures:
    """Packed rows (numpy) with the dataset surface the loops use; ``rows[r]`` lists the examples of row ``r``."""

    def __init__(self, arrays: dict, rows: list[list[int]], source_tokens: int, target_tokens: int):
        self.arrays = arrays
        self.rows = rows
        self.num_examples = sum(len(r) for r in rows)
        self.source_tokens, self.target_tokens = source_tokens, target_tokens

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, i):
        return {k: v[i] for k, v in self.arrays.items()}

    @property
    def column_names(self):
        return list(self.arrays)

    @property
    def examples_per_row(self) -> float:
        return self.num_examples / max(1, len(self.rows))

    @property
    def efficiency(self) -> float:
        """Real source tokens over the rows' source capacity."""
        return self.source_tokens / max(1, self.arrays["input_ids"].size)


def pack_examples(examples, max_source_length: int, max_target_length: int, pad_token_id: int,
                  decoder_start_token_id: int, seed: int = 0, shift_mode: str = "bart") -> PackedSeq2SeqFeatures:
    """Pack ``examples`` = [(source ids, target ids)] (unpadded; longer ones are truncated to the max lengths, as the
    tokenizer does today; an example without a target token is dropped: it has nothing to train on)."""
    ex = [(np.asarray(s)[:max_source_length], np.asarray(t)[:max_target_length]) for s, t in examples]
    ex = [(s, t) for s, t in ex if len(t) > 0 and len(s) > 0]
    rows = first_fit_decreasing([len(s) for s, _ in ex], [len(t) for _, t in ex], max_source_length,
                                max_target_length, seed)
    R, S, T = len(rows), max_source_length, max_target_length
    a = {"input_ids": np.full((R, S), pad_token_id, np.int32), "attention_mask": np.zeros((R, S), np.int8),
         "segment_ids": np.full((R, S), -1, np.int32), "position_ids": np.zeros((R, S), np.int32),
         "labels": np.full((R, T), -100, np.int32), "decoder_input_ids": np.full((R, T), pad_token_id, np.int32),
         "decoder_segment_ids": np.full((R, T), -1, np.int32), "decoder_position_ids": np.zeros((R, T), np.int32)}
    for r, members in enumerate(rows):
        so = to = 0
        for g, i in enumerate(members):
            s, t = ex[i]
            a["input_ids"][r, so:so + len(s)] = s
            a["attention_mask"][r, so:so + len(s)] = 1
            a["segment_ids"][r, so:so + len(s)] = g
            a["position_ids"][r, so:so + len(s)] = np.arange(len(s))
            a["labels"][r, to:to + len(t)] = t
            a["decoder_input_ids"][r, to] = t[-1] if shift_mode == "mbart" else decoder_start_token_id
            a["decoder_input_ids"][r, to + 1:to + len(t)] = t[:-1]
            a["decoder_segment_ids"][r, to:to + len(t)] = g
            a["decoder_position_ids"][r, to:to + len(t)] = np.arange(len(t))
            so += len(s)
            to += len(t)
    return PackedSeq2SeqFeatures(a, rows, sum(len(s) for s, _ in ex), sum(len(t) for _, t in ex))


def pack_features(features, cfg, max_source_length: int, max_target_length: int, seed: int = 0):
    """Pack right-padded tokenised ``features`` (data/dataset.py Seq2SeqFeatures) for the model config ``cfg``."""
    return pack_examples(unpad_features(features, cfg.pad_token_id), max_source_length, max_target_length,
                         cfg.pad_token_id, cfg.decoder_start_token_id, seed, getattr(cfg, "shift_mode", "bart"))
