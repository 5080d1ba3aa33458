"""Per-step time of the sampling step: csrc/sample.hip (one launch) against the torch composite of
models/generation.py, alternating in one process on the same inputs.

    python tools/sample_step_bench.py [--out profiles/sample_step.txt] [--iters 50] [--repeats 7]

Shapes: rows in {8, 64} x V in {32128, 250112}, bf16 logits, top_k=50, top_p=0.9, temperature 0.7, repetition
penalty 1.2, a decoder prefix of 64 tokens.  Each repeat times ``iters`` back-to-back steps of one arm between device
events (the window ends in a synchronise), then the other arm; the table gives the median over the repeats and their
min .. max as the run-to-run spread.  A third column times what transformers runs for the same options (its
processors' ops: sort-based top-p, softmax, torch.multinomial) as a torch-native yardstick with its own randomness.
Needs the GPU: there is no fall-back.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_llms_example_amd import _ext  # noqa: E402
from distributed_llms_example_amd.models import generation as gen  # noqa: E402

OPTS = dict(penalty=1.2, temperature=0.7, top_k=50, top_p=0.9)
PROC = (None, 0, None, None, 128, 1)  # no bans, no forced token


def _inputs(rows, V, prefix=64):
    g = torch.Generator().manual_seed(rows * 7 + V)
    logits = (torch.randn(rows, V, generator=g) * 3.0).to(torch.bfloat16).cuda()
    seqs = torch.randint(0, V, (rows, 128), generator=g).cuda()
    return logits, seqs, prefix


def _kernel(logits, seqs, cur, step):
    rc, tok, _ = _ext.native().sample_step(logits, seqs, cur, 0, -1, -1, OPTS["penalty"], OPTS["temperature"],
                                           OPTS["top_k"], OPTS["top_p"], 1234, step)
    if rc != 0:
        raise RuntimeError(f"sample_step did not take the arguments: rc={rc}")
    return tok


def _composite(logits, seqs, cur, step):
    x = gen._sample_scores(logits, seqs, cur, PROC, OPTS["penalty"], OPTS["temperature"], OPTS["top_k"], OPTS["top_p"])
    return gen._gumbel_argmax(x, 1234, step)


def _torch_native(logits, seqs, cur, step):
    x = gen._penalize(logits.float(), seqs, cur, OPTS["penalty"]) / OPTS["temperature"]
    x = x.masked_fill(x < x.topk(OPTS["top_k"], dim=-1).values[:, -1:], float("-inf"))
    srt, idx = torch.sort(x, descending=False)
    remove = srt.softmax(-1).cumsum(-1) <= 1 - OPTS["top_p"]
    remove[:, -1:] = False
    x = x.masked_fill(remove.scatter(1, idx, remove), float("-inf"))
    return torch.multinomial(x.softmax(-1), 1).view(-1)


def _time(fn, args, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(*args, i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "sample_step.txt"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available() or _ext.native() is None:
        raise SystemExit("sample_step_bench needs the GPU and the built extension")
    arms = [("kernel", _kernel), ("composite", _composite), ("torch-native", _torch_native)]
    lines = [f"sampling step, us per step (median of {a.repeats} repeats x {a.iters} steps [min .. max]); bf16 logits, "
             f"top_k={OPTS['top_k']} top_p={OPTS['top_p']} T={OPTS['temperature']} penalty={OPTS['penalty']}, "
             "prefix 64; arms alternate in one process",
             f"device: {torch.cuda.get_device_name(0)}",
             f"{'rows':>5} {'V':>7} | " + " | ".join(f"{n:^28}" for n, _ in arms) + " | composite / kernel"]
    for rows in (8, 64):
        for V in (32128, 250112):
            args = _inputs(rows, V)
            for _, fn in arms:  # warm-up: code objects, allocator, library algorithm choices
                for i in range(5):
                    fn(*args, i)
            torch.cuda.synchronize()
            t = {n: [] for n, _ in arms}
            for _ in range(a.repeats):
                for n, fn in arms:
                    t[n].append(_time(fn, args, a.iters))
            med = {n: statistics.median(v) for n, v in t.items()}
            cells = [f"{med[n]:9.1f} [{min(t[n]):8.1f} ..{max(t[n]):8.1f}]" for n, _ in arms]
            lines.append(f"{rows:>5} {V:>7} | " + " | ".join(cells) + f" | {med['composite'] / med['kernel']:6.2f}x")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
