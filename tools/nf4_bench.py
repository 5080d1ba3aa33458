"""NF4 frozen-base measurements on the GPU: the GEMMs on the 4-bit codes (csrc/nf4.hip, route ``nf4=fused``) against
``nf4=dequant`` (nf4_dequant into a transient bf16 weight + the projection routes) and against the bf16 frozen path
(``linear_fwd`` / ``linear_dgrad`` on the unquantised weight), and the peak memory of a LoRA step with and without a
quantised base.

    python tools/nf4_bench.py --kernel   # (1) fused | dequant | bf16 at the projection shapes x --rows, NT and NN
    python tools/nf4_bench.py --step     # (2) peak memory of one --model --lora-r 8 step, bf16 base | NF4 base

Arms alternate inside one process, repetition after repetition, so drift of the shared machine hits every arm alike;
every arm is warmed at every shape before its timed windows; a window is --iters-scaled back-to-back calls between
device events and ends in a synchronise.  Reported per shape: each arm's microseconds per call in each repetition,
and in how many repetitions ``fused`` beat ``dequant`` (the route default is ``fused`` where that is all of them,
docs/PERF_HISTORY.md) and the bf16 library path.  Needs a GPU: there is no fall-back.

Bytes a call has to move at least: the weight (N K / 2 + 4 N K / 64 quantised, 2 N K in bf16) plus the activations in
and out; ``weight_stream`` is the fused arm's weight bytes over its time against the 8.0 TB/s HBM3E peak (meaningful at
the decode rows, where the weight is all the traffic).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from distributed_llms_example_amd import _ext  # noqa: E402
from distributed_llms_example_amd.models import build_model, resolve_config  # noqa: E402
from distributed_llms_example_amd.models.lora import LoraConfig, apply_lora, frozen_bytes  # noqa: E402
from distributed_llms_example_amd.ops import nf4, routing  # noqa: E402
from distributed_llms_example_amd.ops.gemm import linear_dgrad, linear_fwd  # noqa: E402

HBM_PEAK = 8.0e12
# (model, projection, N = out features, K = in features)
SHAPES = [("t5-base", "qkv", 2304, 768), ("t5-base", "o", 768, 768), ("t5-base", "wi", 3072, 768),
          ("t5-base", "wo", 768, 3072), ("bart-large", "qkv", 3072, 1024), ("bart-large", "o", 1024, 1024),
          ("bart-large", "fc1", 4096, 1024), ("bart-large", "fc2", 1024, 4096), ("flan-t5-xl", "qkv", 6144, 2048),
          ("flan-t5-xl", "o", 2048, 2048), ("flan-t5-xl", "wi", 10240, 2048), ("flan-t5-xl", "wo", 2048, 5120)]


def _window_us(fn, iters: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def kernel_level(a) -> None:
    for model, proj, N, K in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(N + K)
        w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(torch.bfloat16)
        codes, absmax = nf4.quantize_nf4(w)
        for form in ("nt", "nn"):
            for M in a.rows:
                x = torch.randn(M, K if form == "nt" else N, device="cuda", generator=g).to(torch.bfloat16)

                def routed(route):
                    # the fused arm at EVERY shape: the route's row / depth bounds are what this measurement sets
                    os.environ["DLLM_ROUTE"] = routing.merged(nf4=route, nf4_fused_max_rows=2 ** 30,
                                                              nf4_fused_max_depth=2 ** 30)
                    return nf4._fwd2(x, codes, absmax, None) if form == "nt" else nf4._dgrad2(x, codes, absmax)

                arms = {"fused": lambda: routed("fused"), "dequant": lambda: routed("dequant"),
                        "bf16": (lambda: linear_fwd(x, w, None)) if form == "nt" else (lambda: linear_dgrad(x, w))}
                iters = max(a.min_iters, min(a.max_iters, int(a.window_flop / (2.0 * M * N * K))))
                for fn in arms.values():  # warm-up: code objects, the library's algorithm choice, allocator blocks
                    _window_us(fn, max(3, iters // 4))
                times = {k: [] for k in arms}
                for _ in range(a.reps):
                    for k, fn in arms.items():
                        times[k].append(round(_window_us(fn, iters), 2))
                f, d, b = times["fused"], times["dequant"], times["bf16"]
                print(json.dumps({
                    "model": model, "proj": proj, "form": form, "M": M, "N": N, "K": K, "iters": iters, "us": times,
                    "fused_beats_dequant": sum(x < y for x, y in zip(f, d)), "fused_beats_bf16": sum(
                        x < y for x, y in zip(f, b)), "reps": a.reps,
                    "fused_over_bf16": round(statistics.median(f) / statistics.median(b), 3),
                    "weight_stream": round(nf4.nbytes(N, K) / (statistics.median(f) * 1e-6) / HBM_PEAK, 4)}), flush=True)
    os.environ.pop("DLLM_ROUTE", None)


def step_level(a) -> None:
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    env = init_distributed()
    cfg = resolve_config(a.model)
    g = torch.Generator().manual_seed(0)
    batch = {"input_ids": torch.randint(3, cfg.vocab_size, (1, 1024), generator=g).cuda(),
             "attention_mask": torch.ones(1, 1024, dtype=torch.long).cuda(),
             "labels": torch.randint(3, cfg.vocab_size, (1, 128), generator=g).cuda()}
    for quant in (None, "nf4"):
        torch.manual_seed(0)
        m = build_model(cfg, dtype=torch.bfloat16, device="cuda")  # quantised on the GPU by nf4_quantize
        apply_lora(m, LoraConfig(r=8, alpha=16, targets=("q", "v"), quantize=quant))
        eng = TrainEngine(m, env, lr=1e-4, dtype=torch.bfloat16)
        eng.train()
        for _ in range(2):
            eng.forward_backward(batch)
            eng.step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ms = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            eng.forward_backward(batch)
            eng.step()
            t1.record()
            torch.cuda.synchronize()
            ms.append(round(t0.elapsed_time(t1), 2))
        print(json.dumps({"model": a.model, "lora_r": 8, "lora_quant": quant, "frozen_gib": round(
            frozen_bytes(m) / 2 ** 30, 3), "resident_gib": round(torch.cuda.memory_allocated() / 2 ** 30, 3),
            "peak_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3), "step_ms": ms}), flush=True)
        del eng, m
        torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--rows", type=lambda s: [int(x) for x in s.split(",")], default=[8, 64, 1024, 16384])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window-flop", type=float, default=4e12, help="multiply-adds x 2 per timed window")
    ap.add_argument("--min-iters", type=int, default=10)
    ap.add_argument("--max-iters", type=int, default=400)
    ap.add_argument("--model", default="flan-t5-xl")
    a = ap.parse_args()
    if not torch.cuda.is_available() or _ext.native() is None:
        raise SystemExit("tools/nf4_bench.py needs a GPU and the built extension")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "routes": {"nf4": routing.DEFAULTS["nf4"]}}))
    if a.kernel or not a.step:
        kernel_level(a)
    if a.step:
        step_level(a)


if __name__ == "__main__":
    main()
