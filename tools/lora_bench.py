"""LoRA measurements on the GPU: the adapter kernels (csrc/lora.hip, route ``lora=fused``) against the composite on
the library's GEMMs (``lora=lib``), and LoRA training steps against full fine-tuning.

    python tools/lora_bench.py --op            # (a) one adapted qkv projection, forward + backward
    python tools/lora_bench.py --step          # (b) whole training steps: full fine-tuning | LoRA fused | LoRA lib

Arms alternate inside one process, round after round, so drift of the shared machine hits every arm alike; every
shape is warmed before its timed windows; times are device events around work that ends in a synchronise.  Reported:
the median over rounds and the spread (max - min) / median.  Needs a GPU: there is no fall-back.

(a) times the frozen projection alone as a third arm (``base``), so the adapters' own cost is arm - base.
(b) reports samples/s, the peak memory of a step and the static training state (parameters + gradient buffer +
optimizer state of what is trained).
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
from distributed_llms_example_amd.models.lora import LoraConfig, apply_lora  # noqa: E402
from distributed_llms_example_amd.ops import routing  # noqa: E402
from distributed_llms_example_amd.ops.linear import Linear  # noqa: E402
from distributed_llms_example_amd.ops.lora import Adapter  # noqa: E402
from distributed_llms_example_amd.ops.rng import manual_seed  # noqa: E402


def _route(arm: str) -> None:
    os.environ["DLLM_ROUTE"] = routing.merged(lora="lib" if arm == "lib" else "fused")


def _timed(fn, iters: int) -> float:
    """ms per call: device events around ``iters`` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _summary(vals):
    med = statistics.median(vals)
    return round(med, 4), round((max(vals) - min(vals)) / med, 4)


def op_level(a) -> None:
    for tokens in a.tokens:
        for d in a.widths:
            x = (torch.randn(tokens, d, device="cuda") * 0.5).to(torch.bfloat16).requires_grad_(True)
            gy = (torch.randn(tokens, 3 * d, device="cuda") * 0.1).to(torch.bfloat16)
            lin = Linear(d, 3 * d, bias=False).cuda().to(torch.bfloat16)
            lin.weight.requires_grad_(False)
            for r in a.ranks:
                ads = []
                for i in (0, 2):  # q and v of the fused qkv
                    A = torch.nn.Parameter((torch.randn(r, d, device="cuda") * d ** -0.5).to(torch.bfloat16))
                    B = torch.nn.Parameter((torch.randn(d, r, device="cuda") * 0.02).to(torch.bfloat16))
                    ads.append(Adapter("qv"[i // 2], i * d, d, A, B, 16.0 / r))
                for p in a.dropouts:
                    def run(arm):
                        lin._lora = None if arm == "base" else (ads, p)
                        lin.train()
                        y = lin(x)
                        y.backward(gy)
                        x.grad = None
                        for ad in ads:
                            ad.A.grad = ad.B.grad = None

                    arms = ("base", "fused", "lib")
                    res = {k: [] for k in arms}
                    for arm in arms:  # warm-up: every arm at this shape
                        _route(arm)
                        run(arm)
                        run(arm)
                    torch.cuda.synchronize()
                    for _ in range(a.rounds):
                        for arm in arms:  # alternating
                            _route(arm)
                            res[arm].append(_timed(lambda: run(arm), a.iters))
                    out = {"bench": "op", "tokens": tokens, "d": d, "r": r, "p": p}
                    for arm in arms:
                        out[f"{arm}_ms"], out[f"{arm}_spread"] = _summary(res[arm])
                    out["adapters_fused_ms"] = round(out["fused_ms"] - out["base_ms"], 4)
                    out["adapters_lib_ms"] = round(out["lib_ms"] - out["base_ms"], 4)
                    out["lib_over_fused"] = round(out["lib_ms"] / out["fused_ms"], 3)
                    print(json.dumps(out), flush=True)
            del x, gy, lin
            torch.cuda.empty_cache()


def step_level(a) -> None:
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    env = init_distributed()
    for spec in a.models:
        name, _, b = spec.partition(":")
        B = int(b)
        cfg = resolve_config(name)
        g = torch.Generator().manual_seed(1000)
        batches = [{"input_ids": torch.randint(2, cfg.vocab_size, (B, a.src_len), generator=g).cuda(),
                    "attention_mask": torch.ones(B, a.src_len, dtype=torch.long).cuda(),
                    "labels": torch.randint(2, cfg.vocab_size, (B, a.tgt_len), generator=g).cuda()} for _ in range(2)]
        arms = ("full", "lora_fused", "lora_lib")
        engines = {}
        for arm in ("full", "lora"):
            torch.manual_seed(0)
            m = build_model(cfg)
            if arm == "lora":
                apply_lora(m, LoraConfig(r=a.step_rank, alpha=16, dropout=a.step_dropout, targets=("q", "v")))
            manual_seed(1)
            engines[arm] = TrainEngine(m, env, lr=5e-5, weight_decay=0.01, max_grad_norm=1.0, dtype=torch.bfloat16)
            engines[arm].train()

        def step(arm, i):
            eng = engines["full" if arm == "full" else "lora"]
            _route("lib" if arm == "lora_lib" else "fused")
            eng.forward_backward(batches[i % 2])
            eng.step()

        peak = {}
        for arm in arms:  # warm-up, and the peak memory of one step above what is resident before it
            step(arm, 0)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step(arm, 1)
            torch.cuda.synchronize()
            peak[arm] = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
        res = {k: [] for k in arms}
        for r in range(a.rounds):
            for arm in arms:  # alternating
                ms = _timed(lambda: step(arm, r), a.step_iters)
                res[arm].append(B / (ms / 1e3))
        out = {"bench": "step", "model": name, "batch": B, "src_len": a.src_len, "tgt_len": a.tgt_len,
               "lora_r": a.step_rank, "lora_targets": "q,v", "lora_dropout": a.step_dropout,
               "device": torch.cuda.get_device_name(0)}
        for arm in arms:
            out[f"{arm}_samples_per_s"], out[f"{arm}_spread"] = _summary(res[arm])
            out[f"{arm}_step_peak_gib"] = round(peak[arm], 2)
            fl = engines["full" if arm == "full" else "lora"].flat
            # bf16 parameters + fp32 gradients + fp32 master, two fp32 moments
            out[f"{arm}_train_state_gib"] = round(fl.numel * (2 + 4 + 12) / 2 ** 30, 3)
        out["lora_fused_over_full"] = round(out["lora_fused_samples_per_s"] / out["full_samples_per_s"], 3)
        out["lora_fused_over_lib"] = round(out["lora_fused_samples_per_s"] / out["lora_lib_samples_per_s"], 3)
        print(json.dumps(out), flush=True)
        del engines, batches
        torch.cuda.empty_cache()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--tokens", type=lambda s: [int(v) for v in s.split(",")], default=[65536, 524288])
    ap.add_argument("--widths", type=lambda s: [int(v) for v in s.split(",")], default=[768, 1024, 2048])
    ap.add_argument("--ranks", type=lambda s: [int(v) for v in s.split(",")], default=[8, 64])
    ap.add_argument("--dropouts", type=lambda s: [float(v) for v in s.split(",")], default=[0.0, 0.1])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--models", type=lambda s: s.split(","), default=["t5-base:512", "bart-large:256"])
    ap.add_argument("--src-len", type=int, default=1024)
    ap.add_argument("--tgt-len", type=int, default=128)
    ap.add_argument("--step-rank", type=int, default=8)
    ap.add_argument("--step-dropout", type=float, default=0.1)
    ap.add_argument("--step-iters", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_bench: needs a GPU (no fall-back)")
    if _ext.native() is None:
        raise SystemExit(f"lora_bench: native extension not loaded: {_ext.load_error()}")
    if a.op or not a.step:
        op_level(a)
    if a.step or not a.op:
        step_level(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
