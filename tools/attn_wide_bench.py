#!/usr/bin/env python
"""csrc/attn_wide.hip against what it replaces: ``attention_grouped`` forward + backward at head dim 256 with grouped
K/V heads (the T5Gemma 2b-2b / 9b-9b shapes: 8 / 4 and 16 / 8 heads), once on the kernels and once on the fallback
(``attn_wide`` = 0: K / V repeated per query head into the fp32 composite), on the same capped inputs.  Self-attention
at 1024 and 4096 tokens, full and — at 4096 — with a window of 2048, and one decode-shaped forward (Sq = 1, Sk = 1024).
For orientation only, csrc/attn_hd.hip at head dim 128 with twice the heads (equal FLOPs).

Times are device events around ``--iters`` calls after a warm-up, the arms alternating, ``--repeats`` times: the median
and the (max - min) / median spread are reported.  Peak memory is torch's peak allocation over one call above what the
inputs hold.  Writes one line per shape to stdout and into the last section of ``--out`` (profiles/attn_wide.txt).

    python tools/attn_wide_bench.py [--iters 5] [--repeats 5]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from distributed_llms_example_amd import _ext  # noqa: E402
from distributed_llms_example_amd.ops import attention as A  # noqa: E402
from distributed_llms_example_amd.ops import routing  # noqa: E402

CAP = 50.0
MARK = "== tools/attn_wide_bench.py (MI355X): forward + backward per call, median of the repeats"


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def _arms(B, H, Hkv, Sq, Sk, D, window, causal, backward):
    q = torch.randn(B, Sq, H, D, device="cuda").bfloat16().requires_grad_(backward)
    k, v = (torch.randn(B, Sk, Hkv, D, device="cuda").bfloat16().requires_grad_(backward) for _ in range(2))
    do = torch.randn(B, Sq, H, D, device="cuda").bfloat16()

    def call(route):
        os.environ["DLLM_ROUTE"] = route
        o = A.attention_grouped(q, k, v, scale=D ** -0.5, causal=causal, window=window, softcap=CAP)
        if backward:
            torch.autograd.grad(o, [q, k, v], do)

    arms = {"wide": lambda: call(routing.merged(attn_wide=1)), "fallback": lambda: call(routing.merged(attn_wide=0))}
    if D == 256 and backward:  # orientation: csrc/attn_hd.hip at head dim 128, twice the heads, K / V already repeated
        q2, k2, v2 = (torch.randn(B, S, 2 * H, 128, device="cuda").bfloat16().requires_grad_(True) for S in (Sq, Sk, Sk))
        do2 = torch.randn(B, Sq, 2 * H, 128, device="cuda").bfloat16()
        arms["attn_hd_d128"] = lambda: torch.autograd.grad(
            A.attention(q2, k2, v2, scale=128 ** -0.5, causal=causal, window=window, softcap=CAP), [q2, k2, v2], do2)
    return arms


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_wide.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available() or _ext.native() is None:
        raise SystemExit("attn_wide_bench: needs a GPU and the native extension")
    # tag, B, H, Hkv, Sq, Sk, window, causal, backward.  B: the fallback's fp32 [B, H, Sq, Sk] tensors stay at a few GiB
    shapes = [("train 1024", 8, 8, 4, 1024, 1024, None, False, True), ("train 1024", 4, 16, 8, 1024, 1024, None, False, True),
              ("train 4096", 1, 8, 4, 4096, 4096, None, False, True), ("train 4096 window 2048", 1, 8, 4, 4096, 4096, 2048, False, True),
              ("train 4096", 1, 16, 8, 4096, 4096, None, False, True), ("train 4096 window 2048", 1, 16, 8, 4096, 4096, 2048, False, True),
              ("decode forward", 32, 8, 4, 1, 1024, None, True, False), ("decode forward", 32, 16, 8, 1, 1024, None, True, False)]
    lines = []
    for tag, B, H, Hkv, Sq, Sk, window, causal, backward in shapes:
        arms = _arms(B, H, Hkv, Sq, Sk, 256, window, causal, backward)
        i, j = torch.arange(Sq)[:, None], torch.arange(Sk)[None, :]
        seen = (j <= i + Sk - Sq) if causal else ((j - i).abs() <= window) if window is not None else torch.ones(Sq, Sk)
        flop = 4.0 * B * H * 256 * float(seen.sum()) * (3.5 if backward else 1.0)  # visible pairs only; backward 2.5 x
        for fn in arms.values():  # warm-up: code objects, allocator
            fn()
        torch.cuda.synchronize()
        ms = {n: [] for n in arms}
        for _ in range(a.repeats):
            for n, fn in arms.items():  # alternating
                ms[n].append(_timed(fn, a.iters))
        row = f"{tag:24s} B={B:<2d} H={H}/{Hkv} {Sq}x{Sk}"
        for n, fn in arms.items():
            med = statistics.median(ms[n])
            row += (f" | {n}: {med:.3f} ms (spread {(max(ms[n]) - min(ms[n])) / med:.1%}) {flop / med / 1e9:.1f} TFLOP/s"
                    f" peak {_peak_mb(fn):.0f} MiB")
        row += f" | wide / fallback time {statistics.median(ms['wide']) / statistics.median(ms['fallback']):.3f}"
        print(row, flush=True)
        lines.append(row)
        del arms
        torch.cuda.empty_cache()
    os.environ.pop("DLLM_ROUTE", None)
    # the file's other sections (resource report, accuracy) stay: everything from the marker on is replaced
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    head = ""
    if os.path.exists(a.out):
        with open(a.out) as f:
            head = f.read().split(MARK)[0]
    with open(a.out, "w") as f:
        f.write(head + MARK + "\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
