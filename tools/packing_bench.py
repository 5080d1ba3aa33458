#!/usr/bin/env python
"""Packed against padded training throughput on one GPU: full training steps (forward, backward, AdamW) of t5-base and
bart-large at 1024 source / 128 target tokens per row, on one seeded synthetic length distribution.

Lengths (tokens, drawn once from ``--seed``): log-normal, clipped to [8, 1024] / [4, 128] —

    source: median 120, sigma 0.60  ->  mean ~141   (SAMSum dialogues under the T5 / BART tokenizers: ~140 - 150)
    target: median  24, sigma 0.45  ->  mean ~26.5  (SAMSum summaries: ~25 - 30)

The same examples run once padded (today's path: every example its own 1024 x 128 row, pad labels ignored) and once
packed (data/packing.py, --pack-sequences), alternating ``--rounds`` times in one process, each arm for ``--window``
seconds after ``--warmup`` steps.  Reported per arm: real (non-padding source + target) tokens per second and examples
per second, the median over the rounds and the spread (max - min) / median.  A separate profiled run of the packed arm
(torch.profiler, ``--profile-steps``) reports the attention kernels' share of the GPU kernel time.  No GPU: it fails.

    python tools/packing_bench.py [--models t5-base,bart-large] [--rows 32] [--rounds 3] [--window 4]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_llms_example_amd import _ext  # noqa: E402
from distributed_llms_example_amd.data.collator import DataCollatorForSeq2Seq  # noqa: E402
from distributed_llms_example_amd.data.packing import pack_examples  # noqa: E402
from distributed_llms_example_amd.models import build_model, resolve_config  # noqa: E402
from distributed_llms_example_amd.parallel.env import init_distributed  # noqa: E402
from distributed_llms_example_amd.train.engine import TrainEngine  # noqa: E402

SRC_MEDIAN, SRC_SIGMA, TGT_MEDIAN, TGT_SIGMA = 120.0, 0.60, 24.0, 0.45
S, T = 1024, 128


def examples(n: int, vocab: int, seed: int):
    rng = np.random.default_rng(seed)
    ls = np.clip(rng.lognormal(np.log(SRC_MEDIAN), SRC_SIGMA, n).round(), 8, S).astype(int)
    lt = np.clip(rng.lognormal(np.log(TGT_MEDIAN), TGT_SIGMA, n).round(), 4, T).astype(int)
    return [(rng.integers(3, vocab, size=a), rng.integers(3, vocab, size=b)) for a, b in zip(ls, lt)]


def batches(ex, cfg, rows: int, packed: bool, device):
    """Device batches of ``rows`` rows and, per batch, (examples, real tokens)."""
    coll = DataCollatorForSeq2Seq.for_model(cfg)
    if packed:
        pk = pack_examples(ex, S, T, cfg.pad_token_id, cfg.decoder_start_token_id, shift_mode=cfg.shift_mode)
        feats = [pk[i] for i in range(len(pk))]
        count = [(len(m), sum(len(ex[i][0]) + len(ex[i][1]) for i in m)) for m in pk.rows]
        eff = pk.efficiency
    else:
        feats = []
        for s, t in ex:
            ids = np.full(S, cfg.pad_token_id, np.int64)
            ids[: len(s)] = s
            lab = np.full(T, -100, np.int64)
            lab[: len(t)] = t
            feats.append({"input_ids": ids, "attention_mask": (np.arange(S) < len(s)).astype(np.int64), "labels": lab})
        count = [(1, len(s) + len(t)) for s, t in ex]
        eff = sum(len(s) for s, _ in ex) / (len(ex) * S)
    out = []
    for b in range(len(feats) // rows):
        sl = slice(b * rows, (b + 1) * rows)
        batch = {k: v.to(device) for k, v in coll(feats[sl]).items()}
        out.append((batch, sum(c[0] for c in count[sl]), sum(c[1] for c in count[sl])))
    return out, eff


def run_window(eng, data, start: int, seconds: float, min_steps: int = 2):
    """Steps over ``data`` from index ``start`` for at least ``seconds``: (steps, examples, tokens, elapsed)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps = n_ex = n_tok = 0
    while True:
        batch, e, t = data[(start + steps) % len(data)]
        eng.forward_backward(batch)
        eng.step()
        steps, n_ex, n_tok = steps + 1, n_ex + e, n_tok + t
        if steps >= min_steps:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= seconds:
                break
    return steps, n_ex, n_tok, time.perf_counter() - t0


def attention_share(eng, data, steps: int) -> dict:
    """The packed arm under torch.profiler: GPU kernel time of the attention kernels over all kernels."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for i in range(steps):
            eng.forward_backward(data[i % len(data)][0])
            eng.step()
        torch.cuda.synchronize()
    total = attn = 0.0
    for ev in prof.key_averages():
        t = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0))
        total += t
        if "attn_" in ev.key:
            attn += t
    return {"attention_kernel_share": round(attn / total, 4) if total else None,
            "kernel_time_ms": round(total / 1e3, 2)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="t5-base,bart-large")
    ap.add_argument("--rows", type=int, default=32, help="rows (1024 x 128) per step, both arms")
    ap.add_argument("--examples", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=4.0, help="seconds per arm and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("packing_bench: needs a GPU (no fall-back)")
    if _ext.native() is None:
        raise SystemExit(f"packing_bench: native extension not loaded: {_ext.load_error()}")
    env = init_distributed()
    for name in a.models.split(","):
        cfg = resolve_config(name)
        torch.manual_seed(a.seed)
        eng = TrainEngine(build_model(cfg), env, lr=5e-5, weight_decay=0.01, max_grad_norm=1.0, dtype=torch.bfloat16)
        eng.train()
        ex = examples(a.examples, cfg.vocab_size, a.seed)
        arms, eff = {}, {}
        for arm in ("padded", "packed"):
            arms[arm], eff[arm] = batches(ex, cfg, a.rows, arm == "packed", env.device)
        res = {arm: [] for arm in arms}
        for arm, data in arms.items():
            for i in range(a.warmup):
                eng.forward_backward(data[i % len(data)][0])
                eng.step()
        for r in range(a.rounds):
            for arm, data in arms.items():  # alternating: padded, packed, padded, packed, ...
                steps, n_ex, n_tok, dt = run_window(eng, data, r * 7, a.window)
                res[arm].append({"steps": steps, "tokens_per_s": n_tok / dt, "examples_per_s": n_ex / dt,
                                 "rows_per_s": steps * a.rows / dt})
        out = {"model": name, "rows_per_step": a.rows, "row_shape": [S, T], "examples": len(ex),
               "mean_source_tokens": round(float(np.mean([len(s) for s, _ in ex])), 1),
               "mean_target_tokens": round(float(np.mean([len(t) for _, t in ex])), 1),
               "device": torch.cuda.get_device_name(0)}
        for arm, runs in res.items():
            for key in ("tokens_per_s", "examples_per_s", "rows_per_s"):
                vals = [x[key] for x in runs]
                med = statistics.median(vals)
                out[f"{arm}_{key}"] = round(med, 1)
                out[f"{arm}_{key}_spread"] = round((max(vals) - min(vals)) / med, 4)
            out[f"{arm}_source_efficiency"] = round(eff[arm], 4)
        out["packed_over_padded_tokens_per_s"] = round(out["packed_tokens_per_s"] / out["padded_tokens_per_s"], 3)
        if a.profile_steps > 0:
            out.update(attention_share(eng, arms["packed"], a.profile_steps))
        print(json.dumps(out), flush=True)
        del eng, arms
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
