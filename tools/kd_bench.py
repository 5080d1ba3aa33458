"""Distillation measurements on the GPU: the fused loss kernels (csrc/kd.hip, route ``kd=fused``) against the torch
composite (``kd=composite``) and against the cross-entropy kernels on one tensor, and whole training steps with a
teacher.

    python tools/kd_bench.py --kernel   # (1) kd_fwd + kd_bwd | composite | ce_fwd + ce_bwd on --shapes
    python tools/kd_bench.py --step     # (2) student alone | kd=fused | kd=composite on --pairs

Arms alternate inside one process, round after round, so drift of the shared machine hits every arm alike; every arm is
warmed before its timed windows; times are device events around work that ends in a synchronise.  Reported: the median
over rounds with min..max.  Needs a GPU: there is no fall-back.

(1) bf16 logits ``[N, V]``.  Bytes are what the algorithm has to move: the distillation forward reads both tensors, its
backward reads both and writes the gradient over the student's (5 N V 2 bytes); the CE forward reads one tensor, its
backward reads and writes it (3 N V 2).  ``hbm_fraction`` is those bytes over the time against the 8.0 TB/s HBM3E peak.
The backward runs in place, as in training: a timed window holds --kernel-iters forward + backward pairs, each on a
copy of the logits of its own, restored outside the window; the time is the window's over the pairs.
(2) the bench shapes (1024 source / 128 target tokens), the largest batch of --batches that fits: samples/s per arm, the
peak memory of a step above what is resident, and the teacher forward's share of the fused distillation step.
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
from distributed_llms_example_amd.models.distill import make_student  # noqa: E402
from distributed_llms_example_amd.ops import distill as kd_ops  # noqa: E402
from distributed_llms_example_amd.ops import routing  # noqa: E402
from distributed_llms_example_amd.ops.rng import manual_seed  # noqa: E402

HBM_PEAK = 8.0e12
EPS, T, ALPHA = 0.1, 2.0, 0.5


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
    for spec in a.shapes:
        N, V = (int(x) for x in spec.split("x"))
        g = torch.Generator(device="cuda").manual_seed(N + V)
        keep_s = (2.0 * torch.randn(N, V, device="cuda", generator=g)).to(torch.bfloat16)
        teacher = (0.6 * keep_s.float() + 1.5 * torch.randn(N, V, device="cuda", generator=g)).to(torch.bfloat16)
        works = [keep_s.clone() for _ in range(a.kernel_iters)]  # one per pair of a timed window
        labels = torch.randint(0, V, (N,), device="cuda", generator=g)
        labels[::17] = -100
        count = (labels != -100).sum().float()
        w_ce, w_kl, scale = ((1 - ALPHA) / count).reshape(1), (ALPHA / count).reshape(1), (1.0 / count).reshape(1)

        def kd(work):
            _, _, stats = C.kd_fwd(work, teacher, labels, None, None, EPS, -100, T)
            C.kd_bwd(w_ce, w_kl, work, teacher, labels, stats, None, None, EPS, -100, T, True)

        def kd_t1(work):
            _, _, stats = C.kd_fwd(work, teacher, labels, None, None, EPS, -100, 1.0)
            C.kd_bwd(w_ce, w_kl, work, teacher, labels, stats, None, None, EPS, -100, 1.0, True)

        def ce(work):
            _, lse = C.ce_fwd(work, labels, None, EPS, -100)
            C.ce_bwd(scale, work, labels, lse, None, EPS, -100, True)

        def composite(work):
            s = work.detach().requires_grad_(True)
            loss, _, _ = kd_ops._reference(s, teacher, labels, None, None, EPS, -100, ALPHA, T)
            loss.backward()

        arms = {"kd": kd, "kd_T1": kd_t1, "ce": ce, "composite": composite}
        nbytes = {"kd": 5 * N * V * 2, "kd_T1": 5 * N * V * 2, "ce": 3 * N * V * 2}
        res = {k: [] for k in arms}
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        peaks = {}

        def restore():
            for w in works:
                w.copy_(keep_s)

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
        out = {"bench": "kd_kernels", "N": N, "V": V, "dtype": "bf16", "T": T, "eps": EPS, "rounds": a.rounds,
               "pairs_per_window": a.kernel_iters,
               "device": torch.cuda.get_device_name(0)}
        for name in arms:
            s = _summary(res[name])
            out[f"{name}_ms"] = s
            out[f"{name}_extra_peak_gib"] = peaks[name]
            if name in nbytes:
                out[f"{name}_tb_per_s"] = round(nbytes[name] / (s["median"] / 1e3) / 1e12, 3)
                out[f"{name}_hbm_fraction"] = round(nbytes[name] / (s["median"] / 1e3) / HBM_PEAK, 3)
        out["fused_over_composite"] = round(out["composite_ms"]["median"] / out["kd_ms"]["median"], 2)
        out["kd_over_ce_time"] = round(out["kd_ms"]["median"] / out["ce_ms"]["median"], 3)
        print(json.dumps(out), flush=True)
        del keep_s, teacher, works
        torch.cuda.empty_cache()


def step_level(a) -> None:
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    env = init_distributed()
    for spec in a.pairs:
        tname, _, sname = spec.partition(":")
        torch.manual_seed(0)
        tcfg = resolve_config(tname)
        teacher = build_model(tcfg)
        if "," in sname:
            student = make_student(teacher, *(int(x) for x in sname.split(",")))
        else:
            student = build_model(resolve_config(sname))
        arms = ("student", "kd_fused", "kd_composite")
        for B in a.batches:
            out = {"bench": "kd_step", "teacher": tname, "student": sname, "batch": B, "src_len": a.src_len,
                   "tgt_len": a.tgt_len, "device": torch.cuda.get_device_name(0)}
            g = torch.Generator().manual_seed(1000)
            engines = {}
            try:
                for arm in arms:
                    manual_seed(1)
                    engines[arm] = TrainEngine(copy.deepcopy(student), env, lr=5e-5, weight_decay=0.01, max_grad_norm=1.0,
                                               dtype=torch.bfloat16, label_smoothing=EPS,
                                               teacher=None if arm == "student" else copy.deepcopy(teacher),
                                               kd_alpha=ALPHA, kd_temperature=T)
                    engines[arm].train()
                batches = [{"input_ids": torch.randint(2, tcfg.vocab_size, (B, a.src_len), generator=g).cuda(),
                            "attention_mask": torch.ones(B, a.src_len, dtype=torch.long).cuda(),
                            "labels": torch.randint(2, tcfg.vocab_size, (B, a.tgt_len), generator=g).cuda()}
                           for _ in range(2)]

                def step(arm, i):
                    os.environ["DLLM_ROUTE"] = routing.merged(kd="composite" if arm == "kd_composite" else "fused")
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
                tfwd = []
                t_eng = engines["kd_fused"]
                for r in range(a.rounds):
                    for arm in arms:  # alternating
                        ms = _event_ms(lambda: [step(arm, r + i) for i in range(a.step_iters)]) / a.step_iters
                        res[arm].append(B / (ms / 1e3))

                    def teacher_fwd():
                        with torch.no_grad():
                            t_eng.teacher.lm_head_operands(**batches[r % 2])
                    tfwd.append(_event_ms(teacher_fwd))
            except torch.cuda.OutOfMemoryError:
                print(json.dumps(dict(out, status="out of memory")), flush=True)
                del engines
                torch.cuda.empty_cache()
                continue
            finally:
                os.environ["DLLM_ROUTE"] = routing.merged(kd="fused")
            for arm in arms:
                out[f"{arm}_samples_per_s"] = _summary(res[arm], 2)
            out["teacher_forward_ms"] = _summary(tfwd, 2)
            out["teacher_forward_share_of_fused_step"] = round(
                out["teacher_forward_ms"]["median"] / (B / out["kd_fused_samples_per_s"]["median"] * 1e3), 3)
            out["fused_over_composite"] = round(out["kd_fused_samples_per_s"]["median"] /
                                                out["kd_composite_samples_per_s"]["median"], 4)
            out["fused_over_student"] = round(out["kd_fused_samples_per_s"]["median"] /
                                              out["student_samples_per_s"]["median"], 4)
            print(json.dumps(out), flush=True)
            del engines, batches
            torch.cuda.empty_cache()
            break  # the largest batch that fits


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--shapes", type=lambda s: s.split(","), default=["65536x32128", "16384x50265"])
    ap.add_argument("--pairs", type=lambda s: s.split(";"), default=["t5-base:6,6", "t5-base:t5-small"],
                    help="teacher:student; a student E,D is built from the teacher (make_student)")
    ap.add_argument("--batches", type=lambda s: [int(x) for x in s.split(",")], default=[512, 384, 256, 128])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel-iters", type=int, default=8, help="fwd + bwd pairs inside one timed window of --kernel")
    ap.add_argument("--step-iters", type=int, default=2)
    ap.add_argument("--src-len", type=int, default=1024)
    ap.add_argument("--tgt-len", type=int, default=128)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("tools/kd_bench.py needs a GPU", file=sys.stderr)
        return 2
    if a.kernel:
        kernel_level(a)
    if a.step:
        step_level(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
