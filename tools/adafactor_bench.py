"""Adafactor measurements on the GPU: the fused kernels (csrc/adafactor.hip, route ``adafactor=fused``) against the
per-unit torch composite (``adafactor=composite``) and against the fused AdamW step on the same flat buffers, and whole
training steps with either optimizer.

    python tools/adafactor_bench.py --opt     # (a) optimizer step on the flat layouts of --opt-models
    python tools/adafactor_bench.py --step    # (b) whole training steps, adamw | adafactor, of --models

Arms alternate inside one process, round after round, so drift of the shared machine hits every arm alike; every arm is
warmed before its timed windows; times are device events around work that ends in a synchronise.  Reported: the median
over rounds with min..max.  Needs a GPU: there is no fall-back.

(a) bf16 parameters + fp32 master, fp32 gradients, global-norm clip on (one more gradient read in every arm).  Bytes
per parameter are what the algorithm has to move, computed here from the launches: the clip's norm reads the gradient
(4); Adafactor reads it three more times (12), reads and writes the master (8) and writes the bf16 parameter (2): 26,
30 with ``scale_parameter`` (the master once more); AdamW reads gradient, master and two moments (16), writes master,
moments and parameter (14), + 4 for the clip: 34 (+ 1 with a decay mask).  ``hbm_fraction`` is those bytes over the time
against the 8.0 TB/s HBM3E peak (MI355X; a float4 copy reaches 79 % of it).
(b) reports samples/s, the peak memory of a step above what is resident and the optimizer's ``state_bytes()``.
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
from distributed_llms_example_amd.models.hf_io import hf_param_names  # noqa: E402
from distributed_llms_example_amd.ops import routing  # noqa: E402
from distributed_llms_example_amd.ops.optim import FusedAdafactor, FusedAdamW  # noqa: E402
from distributed_llms_example_amd.ops.rng import manual_seed  # noqa: E402
from distributed_llms_example_amd.parallel.flat import FlatParams  # noqa: E402

HBM_PEAK = 8.0e12


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


def _model(name):
    cfg = resolve_config(name)
    torch.manual_seed(0)
    return build_model(cfg), cfg


def opt_level(a) -> None:
    for name in a.opt_models:
        model, cfg = _model(name)
        model = model.to(device="cuda", dtype=torch.bfloat16)
        flat = FlatParams(model, grad_dtype=torch.float32)
        n = flat.numel
        nd = lambda s: "layer_norm" in s
        parts = lambda s: len(hf_param_names(cfg, s))
        opts = {"adafactor": FusedAdafactor(flat, lr=1e-3, relative_step=False, scale_parameter=False,
                                            weight_decay=0.01, no_decay=nd, parts=parts),
                "adafactor_scale": FusedAdafactor(flat, lr=1e-3, relative_step=False, scale_parameter=True,
                                                  weight_decay=0.01, no_decay=nd, parts=parts),
                "adamw": FusedAdamW(flat, lr=1e-5, weight_decay=0.01, no_decay=nd)}
        bytes_pp = {"adafactor": 26, "adafactor_scale": 30, "adamw": 35, "composite": None}
        flat.grad_buf.copy_(torch.randn(n, device="cuda") * 1e-3)

        def run(arm):
            os.environ["DLLM_ROUTE"] = routing.merged(adafactor="composite" if arm == "composite" else "fused")
            opts["adafactor" if arm == "composite" else arm].step(max_grad_norm=1.0)

        arms = ("adafactor", "adafactor_scale", "adamw", "composite")
        for arm in arms:
            run(arm)
            run(arm)
        torch.cuda.synchronize()
        res = {k: [] for k in arms}
        for _ in range(a.rounds):
            for arm in arms:  # alternating
                res[arm].append(_timed(lambda: run(arm), 2 if arm == "composite" else a.iters))
        os.environ["DLLM_ROUTE"] = routing.merged(adafactor="fused")
        out = {"bench": "opt_step", "model": name, "flat_numel": n, "units": len(opts["adafactor"].units),
               "segments": len(flat.segments), "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
        for arm in arms:
            s = _summary(res[arm])
            out[f"{arm}_ms"] = s
            if bytes_pp[arm]:
                out[f"{arm}_bytes_per_param"] = bytes_pp[arm]
                out[f"{arm}_hbm_fraction"] = round(bytes_pp[arm] * n / (s["median"] / 1e3) / HBM_PEAK, 3)
        out["fused_over_composite"] = round(out["composite_ms"]["median"] / out["adafactor_ms"]["median"], 2)
        out["adafactor_over_adamw_time"] = round(out["adafactor_ms"]["median"] / out["adamw_ms"]["median"], 3)
        out["adafactor_state_bytes"] = opts["adafactor"].state_bytes()
        out["adamw_state_bytes"] = opts["adamw"].state_bytes()
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
        arms = ("adamw", "adafactor")
        out = {"bench": "train_step", "model": name, "batch": B, "src_len": a.src_len, "tgt_len": a.tgt_len,
               "device": torch.cuda.get_device_name(0)}
        engines = {}
        built, cfg = _model(name)
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

        for arm in arms:  # warm-up, and the peak memory of one step above what is resident before it
            step(arm, 0)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step(arm, 1)
            torch.cuda.synchronize()
            out[f"{arm}_step_peak_gib"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 2)
        out["resident_gib"] = round(torch.cuda.memory_allocated() / 2 ** 30, 2)
        res = {k: [] for k in arms}
        for r in range(a.rounds):
            for arm in arms:  # alternating
                res[arm].append(B / (_timed(lambda: step(arm, r), a.step_iters) / 1e3))
        for arm in arms:
            out[f"{arm}_samples_per_s"] = _summary(res[arm], 2)
            out[f"{arm}_state_bytes"] = engines[arm].optimizer.state_bytes()
        out["adafactor_over_adamw"] = round(out["adafactor_samples_per_s"]["median"] /
                                            out["adamw_samples_per_s"]["median"], 4)
        print(json.dumps(out), flush=True)
        del engines, batches
        torch.cuda.empty_cache()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--opt", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--opt-models", type=lambda s: s.split(","), default=["t5-base", "google/flan-t5-xl"])
    ap.add_argument("--models", type=lambda s: s.split(","), default=["t5-base:512", "google/flan-t5-xl:16"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=2)
    ap.add_argument("--src-len", type=int, default=1024)
    ap.add_argument("--tgt-len", type=int, default=128)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("tools/adafactor_bench.py needs a GPU", file=sys.stderr)
        return 2
    if a.opt:
        opt_level(a)
    if a.step:
        step_level(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
