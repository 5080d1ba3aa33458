"""8-bit AdamW measurements on the GPU: the step kernel of csrc/adamw_q8.hip against the fp32 step of csrc/adamw.hip on
the same flat buffers, and whole training steps with either optimizer.

    python tools/adamw_q8_bench.py --opt     # (a) the two step kernels, alternating, on the flat layouts of --opt-models
    python tools/adamw_q8_bench.py --step    # (b) whole training steps, adamw | adamw_8bit, of --models (name:batch)

One JSON line per model.  Times are device events around ``--iters`` calls, medians (min, max) over ``--rounds`` rounds
that alternate the arms.  (a) runs ``step(max_grad_norm=None)``: one launch each, no gradient norm.  Bytes per parameter,
bf16 parameters + fp32 master + decay mask: the fp32 step reads grad 4, master 4, m 4, v 4, mask 1 and writes master 4,
m 4, v 4, param 2 = 31; the 8-bit step moves grad 4, master 4 + 4, param 2, codes 2 + 2, mask 1 and 20 / 64 of scales
and slot = 19.3 on a quantised block, and 4 + 8 + 2 + 16 (fp32 moments) + 2 (codes, read and dropped) + 1 + 12 / 64 =
33.2 on a block whose moments stay fp32; the line reports the layout's mix.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from distributed_llms_example_amd.models import build_model, resolve_config  # noqa: E402
from distributed_llms_example_amd.ops.optim import FusedAdamW, FusedAdamW8bit, embedding_parameters  # noqa: E402
from distributed_llms_example_amd.ops.rng import manual_seed  # noqa: E402
from distributed_llms_example_amd.parallel.flat import FlatParams  # noqa: E402


def _timed(fn, iters: int) -> float:
    """ms per call: device events around ``iters`` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _summary(vals, nd=4):
    return {"median": round(statistics.median(vals), nd), "min": round(min(vals), nd), "max": round(max(vals), nd)}


def opt_level(a) -> None:
    for name in a.opt_models:
        torch.manual_seed(0)
        model = build_model(resolve_config(name)).to(device="cuda", dtype=torch.bfloat16)
        flat = FlatParams(model, grad_dtype=torch.float32)
        n = flat.numel
        nd = lambda s: "layer_norm" in s
        opts = {"adamw": FusedAdamW(flat, lr=1e-5, weight_decay=0.01, no_decay=nd),
                "adamw_8bit": FusedAdamW8bit(flat, lr=1e-5, weight_decay=0.01, no_decay=nd,
                                             keep_fp32=embedding_parameters(model).__contains__)}
        side = int((opts["adamw_8bit"].slots >= 0).sum()) * 64
        bytes_pp = {"adamw": 31.0, "adamw_8bit": (19.3125 * (n - side) + 33.1875 * side) / n}
        flat.grad_buf.copy_(torch.randn(n, device="cuda") * 1e-3)
        arms = tuple(opts)
        for arm in arms:
            for _ in range(3):
                opts[arm].step()
        torch.cuda.synchronize()
        res = {k: [] for k in arms}
        for _ in range(a.rounds):
            for arm in arms:  # alternating
                res[arm].append(_timed(opts[arm].step, a.iters))
        out = {"bench": "opt_step", "model": name, "flat_numel": n, "fp32_moment_elements": side,
               "rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
        for arm in arms:
            s = _summary(res[arm])
            out[f"{arm}_ms"] = s
            out[f"{arm}_bytes_per_param"] = round(bytes_pp[arm], 2)
            out[f"{arm}_tb_per_s"] = round(bytes_pp[arm] * n / (s["median"] / 1e3) / 1e12, 3)
            out[f"{arm}_state_bytes"] = opts[arm].state_bytes()
        out["q8_over_fp32_time"] = round(out["adamw_8bit_ms"]["median"] / out["adamw_ms"]["median"], 3)
        print(json.dumps(out), flush=True)
        del opts, flat, model
        torch.cuda.empty_cache()


def step_level(a) -> None:
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    env = init_distributed()
    for spec in a.models:
        name, _, b = spec.partition(":")
        B = int(b)
        g = torch.Generator().manual_seed(1000)
        arms = ("adamw", "adamw_8bit")
        out = {"bench": "train_step", "model": name, "batch": B, "src_len": a.src_len, "tgt_len": a.tgt_len,
               "device": torch.cuda.get_device_name(0)}
        cfg = resolve_config(name)
        torch.manual_seed(0)
        built = build_model(cfg)
        engines = {}
        for arm in arms:
            model = copy.deepcopy(built) if arm == arms[0] else built  # the engine moves its model to the GPU in place
            manual_seed(1)
            engines[arm] = TrainEngine(model, env, lr=5e-5, weight_decay=0.01, max_grad_norm=1.0,
                                       dtype=torch.bfloat16, optim=arm)
            engines[arm].train()
        batches = [{"input_ids": torch.randint(2, cfg.vocab_size, (B, a.src_len), generator=g).cuda(),
                    "attention_mask": torch.ones(B, a.src_len, dtype=torch.long).cuda(),
                    "labels": torch.randint(2, cfg.vocab_size, (B, a.tgt_len), generator=g).cuda()} for _ in range(2)]

        def step(arm, i):
            engines[arm].forward_backward(batches[i % 2])
            engines[arm].step()

        for arm in arms:
            step(arm, 0)
            step(arm, 1)
        torch.cuda.synchronize()
        res = {k: [] for k in arms}
        for r in range(a.rounds):
            for arm in arms:  # alternating
                res[arm].append(B / (_timed(lambda: step(arm, r), a.step_iters) / 1e3))
        for arm in arms:
            out[f"{arm}_samples_per_s"] = _summary(res[arm], 2)
            out[f"{arm}_state_bytes"] = engines[arm].optimizer.state_bytes()
        out["q8_over_fp32"] = round(out["adamw_8bit_samples_per_s"]["median"] / out["adamw_samples_per_s"]["median"], 4)
        out["resident_gib"] = round(torch.cuda.memory_allocated() / 2 ** 30, 2)
        print(json.dumps(out), flush=True)
        del engines, batches
        torch.cuda.empty_cache()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--opt", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--opt-models", type=lambda s: s.split(","), default=["t5-base", "google/flan-t5-xl"])
    ap.add_argument("--models", type=lambda s: s.split(","), default=["t5-base:512"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=2)
    ap.add_argument("--src-len", type=int, default=1024)
    ap.add_argument("--tgt-len", type=int, default=128)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("tools/adamw_q8_bench.py needs a GPU", file=sys.stderr)
        return 2
    if a.opt or not a.step:
        opt_level(a)
    if a.step:
        step_level(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
