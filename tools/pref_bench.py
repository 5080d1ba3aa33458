"""Preference-optimisation measurements on the GPU: the fused loss kernels (csrc/pref.hip, route ``pref=fused``) against
the torch composite (``pref=composite``) and against the cross-entropy kernels on one tensor, and whole training steps
with and without the reference policy.

    python tools/pref_bench.py --kernel   # (1) pref_fwd + pref_pairs x 2 + pref_bwd | composite | ce_fwd + ce_bwd
    python tools/pref_bench.py --step     # (2) plain CE step | pref=fused | pref=composite on --models
    python tools/pref_bench.py --kernel --step --out profiles/pref_step.txt

Arms alternate inside one process, round after round, so drift of the shared machine hits every arm alike; every arm is
warmed before its timed windows; times are device events around work that ends in a synchronise.  Reported: the median
over rounds with min..max.  Needs a GPU: there is no fall-back.

(1) bf16 logits ``[N, V]`` with ``N = 2 P T`` rows at ``T`` = --tgt-len.  Bytes are what the algorithm has to move: the
preference forward reads both tensors, its backward reads the policy's and writes the gradient over it (4 N V 2 bytes);
the CE forward reads one tensor, its backward reads and writes it (3 N V 2).  ``hbm_fraction`` is those bytes over the
time against the 8.0 TB/s HBM3E peak.  The backward runs in place, as in training: a timed window holds --kernel-iters
forward + backward pairs, each on a copy of the logits of its own, restored outside the window.
(2) the bench shapes (1024 source / 128 target tokens): ``batch`` prompts per step — the plain arm trains on ``batch``
targets, the preference arms on ``2 batch`` (chosen, rejected) — samples (prompts) per second per arm, the peak memory
of a step above what is resident, and the reference forward's share of the fused preference step.
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

from distributed_llms_example_amd import _ext  # noqa: E402
from distributed_llms_example_amd.models import build_model, resolve_config  # noqa: E402
from distributed_llms_example_amd.ops import preference as pref_ops  # noqa: E402
from distributed_llms_example_amd.ops import routing  # noqa: E402
from distributed_llms_example_amd.ops.rng import manual_seed  # noqa: E402

HBM_PEAK = 8.0e12
BETA, EPS, SFT = 0.1, 0.0, 0.0
_OUT = []


def emit(rec: dict) -> None:
    line = json.dumps(rec)
    print(line, flush=True)
    _OUT.append(line)


def _event_ms(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _summary(vals, nd=3):
    return {"median": round(statistics.median(vals), nd), "min": round(min(vals), nd), "max": round(max(vals), nd)}


def kernel_level(a) -> None:
    C = _ext.native()
    T = a.tgt_len
    for spec in a.shapes:
        N, V = (int(x) for x in spec.split("x"))
        P = N // (2 * T)
        g = torch.Generator(device="cuda").manual_seed(N + V)
        keep = (2.0 * torch.randn(N, V, device="cuda", generator=g)).to(torch.bfloat16)
        ref = (0.6 * keep.float() + 1.5 * torch.randn(N, V, device="cuda", generator=g)).to(torch.bfloat16)
        works = [keep.clone() for _ in range(a.kernel_iters)]  # one per pair of a timed window
        labels = torch.randint(0, V, (N,), device="cuda", generator=g)
        labels[::17] = -100
        count = (labels != -100).sum().float()
        one, ip = torch.ones(1, device="cuda"), torch.full((1,), 1.0 / P, device="cuda")
        scale = (1.0 / count).reshape(1)

        def pref(work):
            lp, lr, lse = C.pref_fwd(work, ref, labels, None, None, -100)
            C.pref_pairs(lp, lr, labels, None, ip, T, V, -100, BETA, 0, EPS, SFT)      # the forward's loss
            _, _, coef = C.pref_pairs(lp, lr, labels, one, ip, T, V, -100, BETA, 0, EPS, SFT)  # the backward's c
            C.pref_bwd(coef, work, labels, lse, None, True)

        def ce(work):
            _, lse = C.ce_fwd(work, labels, None, 0.0, -100)
            C.ce_bwd(scale, work, labels, lse, None, 0.0, -100, True)

        def composite(work):
            s = work.detach().requires_grad_(True)
            loss, _ = pref_ops._reference(s, ref, labels, T, None, None, BETA, "sigmoid", EPS, SFT)
            loss.backward()

        arms = {"pref": pref, "ce": ce, "composite": composite}
        nbytes = {"pref": 4 * N * V * 2, "ce": 3 * N * V * 2}
        res = {k: [] for k in arms}
        base = torch.cuda.memory_allocated()
        peaks = {}

        def restore():
            for w in works:
                w.copy_(keep)

        def window(fn):  # kernel_iters fwd + bwd pairs, each on logits of its own
            for w in works:
                fn(w)

        for name, fn in arms.items():  # each arm's peak memory above the resident tensors
            torch.cuda.reset_peak_memory_stats()
            restore()
            fn(works[0])
            torch.cuda.synchronize()
            peaks[name] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 2)
        for name, fn in arms.items():  # warm-up: a whole window, the allocator's blocks kept for the timed ones
            restore()
            window(fn)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for name, fn in arms.items():  # alternating
                restore()
                res[name].append(_event_ms(lambda: window(fn)) / a.kernel_iters)
        out = {"bench": "pref_kernels", "N": N, "V": V, "pairs": P, "T": T, "dtype": "bf16", "rounds": a.rounds,
               "pairs_per_window": a.kernel_iters, "device": torch.cuda.get_device_name(0)}
        for name in arms:
            s = _summary(res[name])
            out[f"{name}_ms"] = s
            out[f"{name}_extra_peak_gib"] = peaks[name]
            if name in nbytes:
                out[f"{name}_tb_per_s"] = round(nbytes[name] / (s["median"] / 1e3) / 1e12, 3)
                out[f"{name}_hbm_fraction"] = round(nbytes[name] / (s["median"] / 1e3) / HBM_PEAK, 3)
        out["fused_over_composite"] = round(out["composite_ms"]["median"] / out["pref_ms"]["median"], 2)
        out["fused_faster_in_every_round"] = all(p < c for p, c in zip(res["pref"], res["composite"]))
        out["pref_over_ce_time"] = round(out["pref_ms"]["median"] / out["ce_ms"]["median"], 3)
        out["pref_over_ce_bytes_per_s"] = round(out["pref_tb_per_s"] / out["ce_tb_per_s"], 3)
        emit(out)
        del keep, ref, works
        torch.cuda.empty_cache()


def step_level(a) -> None:
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    env = init_distributed()
    for name in a.models:
        torch.manual_seed(0)
        cfg = resolve_config(name)
        model = build_model(cfg)
        arms = ("plain", "pref_fused", "pref_composite")
        for B in a.batches:
            out = {"bench": "pref_step", "model": name, "batch": B, "src_len": a.src_len, "tgt_len": a.tgt_len,
                   "device": torch.cuda.get_device_name(0)}
            g = torch.Generator().manual_seed(1000)
            engines = {}
            try:
                for arm in arms:
                    manual_seed(1)
                    engines[arm] = TrainEngine(copy.deepcopy(model), env, lr=5e-5, weight_decay=0.01, max_grad_norm=1.0,
                                               dtype=torch.bfloat16,
                                               reference=None if arm == "plain" else copy.deepcopy(model),
                                               dpo_beta=BETA)
                    engines[arm].train()
                batches = [{"input_ids": torch.randint(2, cfg.vocab_size, (B, a.src_len), generator=g).cuda(),
                            "attention_mask": torch.ones(B, a.src_len, dtype=torch.long).cuda(),
                            "labels": torch.randint(2, cfg.vocab_size, (2 * B, a.tgt_len), generator=g).cuda()}
                           for _ in range(2)]

                def step(arm, i):
                    os.environ["DLLM_ROUTE"] = routing.merged(pref="composite" if arm == "pref_composite" else "fused")
                    b = batches[i % 2]
                    if arm == "plain":  # the chosen targets alone
                        b = dict(b, labels=b["labels"][0::2].contiguous())
                    engines[arm].forward_backward(b)
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
                rfwd = []
                r_eng = engines["pref_fused"]
                for r in range(a.rounds):
                    for arm in arms:  # alternating
                        ms = _event_ms(lambda: [step(arm, r + i) for i in range(a.step_iters)]) / a.step_iters
                        res[arm].append(B / (ms / 1e3))

                    def reference_fwd():
                        with torch.no_grad():
                            r_eng.reference.lm_head_operands(**batches[r % 2])
                    rfwd.append(_event_ms(reference_fwd))
            except torch.cuda.OutOfMemoryError:
                emit(dict(out, status="out of memory"))
                del engines
                torch.cuda.empty_cache()
                continue
            finally:
                os.environ["DLLM_ROUTE"] = routing.merged(pref=routing.DEFAULTS["pref"])
            for arm in arms:
                out[f"{arm}_samples_per_s"] = _summary(res[arm], 2)
            out["reference_forward_ms"] = _summary(rfwd, 2)
            out["reference_forward_share_of_fused_step"] = round(
                out["reference_forward_ms"]["median"] / (B / out["pref_fused_samples_per_s"]["median"] * 1e3), 3)
            out["fused_over_composite"] = round(out["pref_fused_samples_per_s"]["median"] /
                                                out["pref_composite_samples_per_s"]["median"], 4)
            out["fused_over_plain"] = round(out["pref_fused_samples_per_s"]["median"] /
                                            out["plain_samples_per_s"]["median"], 4)
            emit(out)
            del engines, batches
            torch.cuda.empty_cache()
            break  # the largest batch that fits


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--shapes", type=lambda s: s.split(","), default=["65536x32128", "16384x50265"])
    ap.add_argument("--models", type=lambda s: s.split(","), default=["t5-base"])
    ap.add_argument("--batches", type=lambda s: [int(x) for x in s.split(",")], default=[128, 64, 32])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel-iters", type=int, default=8, help="fwd + bwd pairs inside one timed window of --kernel")
    ap.add_argument("--step-iters", type=int, default=2)
    ap.add_argument("--src-len", type=int, default=1024)
    ap.add_argument("--tgt-len", type=int, default=128)
    ap.add_argument("--out", type=str, default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("tools/pref_bench.py needs a GPU", file=sys.stderr)
        return 2
    if a.kernel:
        kernel_level(a)
    if a.step:
        step_level(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(_OUT) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
