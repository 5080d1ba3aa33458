"""Microbenchmark of the attention kernels at T5/BART training shapes (fwd, bwd, TFLOP/s).

``--head-dim D`` runs the cases at another head dim (default 64: csrc/attn.hip; others: csrc/attn_hd.hip).
``--vs-composite B,H,S,bias,kpm,causal,p`` times forward + backward of the kernel and of the composite
(``A._reference`` on the same bf16 inputs) interleaved in one process, at ``--head-dim``.
``--window W --shape B,H,S[,bias,p]`` times forward + backward of three arms interleaved in one process: the windowed
kernels (csrc/attn_hd.hip, ``window=W``), the same kernels walking every block (``window=S``: masks and skips nothing,
bitwise the unwindowed call) and what a T5 encoder runs for full attention at that length (csrc/attn.hip at head dim
64: one call, or above ``attn_chunk_min`` tokens the chunked blocks of parallel/context.py).
``--window W --global-keys N --shape B,H,S[,bias,p]`` times the windowed call (LED's: scale d^-0.5) forward and
backward apart, with no global key, with key 0 global and with N global keys spread evenly over the sequence, the arms
interleaved in one process; per arm the median and the spread (min .. max) over the rounds."""
import argparse
import json
import time

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_llms_example_amd.ops import attention as A


def run(B, H, Sq, Sk, bias, kpm, causal, p, iters=20, sat=True, D=64):
    dev = "cuda"
    q = torch.randn(B, Sq, H, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(B, Sk, H, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(B, Sk, H, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    tab = torch.randn(32, H, device=dev, requires_grad=True) if bias else None
    mask = torch.ones(B, Sk, dtype=torch.bool, device=dev) if kpm else None
    lut = A.relative_bias_lut(tab, Sq, Sk, not causal, 32, 128) if bias else None
    if bias:  # sat=False: no saturated-bias ranges declared (every tile takes the LUT path)
        sat_r = lut._dllm_sat if sat else None
        lut = lut.detach()
        lut._dllm_sat = sat_r

    def fwd():
        return A.attention(q, k, v, scale=1.0, causal=causal, key_padding_mask=mask,
                           bias_lut=lut if bias else None, dropout_p=p, seed=1)
    o = fwd()
    g = torch.randn_like(o)
    for _ in range(3):
        fwd()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fwd()
    torch.cuda.synchronize()
    tf = (time.perf_counter() - t0) / iters
    lut2 = A.relative_bias_lut(tab, Sq, Sk, not causal, 32, 128) if bias else None
    if bias and not sat:
        lut2._dllm_sat = None
    def fb():
        o = A.attention(q, k, v, scale=1.0, causal=causal, key_padding_mask=mask, bias_lut=lut2, dropout_p=p, seed=1)
        o.backward(g, retain_graph=True)
    for _ in range(3):
        fb()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fb()
    torch.cuda.synchronize()
    tb = (time.perf_counter() - t0) / iters - tf
    fl = 4 * B * H * Sq * Sk * D * (0.5 if causal else 1.0)
    return {"B": B, "H": H, "Sq": Sq, "Sk": Sk, "bias": bias, "sat": bool(bias and sat), "kpm": kpm,
            "causal": causal, "p": p, **({"D": D} if D != 64 else {}),
            "fwd_ms": tf * 1e3, "bwd_ms": tb * 1e3, "fwd_tflops": fl / tf / 1e12, "bwd_tflops": 2.5 * fl / tb / 1e12}


def vs_composite(B, H, S, bias, kpm, causal, p, D, reps=3, iters=5):
    """Forward + backward time of ``A.attention`` (the kernel the route picks) and of the composite on the same bf16
    inputs, interleaved: warm-up, then ``reps`` rounds of ``iters`` calls each, timed with device events."""
    dev = "cuda"
    q, k, v = (torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16, requires_grad=True) for _ in range(3))
    tab = torch.randn(32, H, device=dev) if bias else None
    lut = A.relative_bias_lut(tab, S, S, not causal, 32, 128) if bias else None
    mask = torch.ones(B, S, dtype=torch.bool, device=dev) if kpm else None
    if kpm:
        mask[:, S - S // 8:] = False
    scale = 1.0 if bias else D ** -0.5
    g = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16)

    def kern():
        A.attention(q, k, v, scale=scale, causal=causal, key_padding_mask=mask, bias_lut=lut, dropout_p=p,
                    seed=1).backward(g)

    def comp():
        A._reference(q, k, v, scale, causal, mask, lut, p, 1).backward(g)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for fn in (kern, comp, kern, comp):
        fn()
    torch.cuda.synchronize()
    tk, tc = [], []
    for _ in range(reps):
        tk.append(timed(kern))
        tc.append(timed(comp))
    fl = 3.5 * 4 * B * H * S * S * D * (0.5 if causal else 1.0)
    route = A._route(q, k, v)
    return {"B": B, "H": H, "S": S, "D": D, "bias": bias, "kpm": kpm, "causal": causal, "p": p, "route": route,
            "kernel_ms": [round(t, 4) for t in tk], "composite_ms": [round(t, 4) for t in tc],
            "kernel_tflops": fl / (sorted(tk)[len(tk) // 2] * 1e-3) / 1e12,
            "composite_tflops": fl / (sorted(tc)[len(tc) // 2] * 1e-3) / 1e12}


def vs_window(B, H, S, W, bias, p, D, reps=5, iters=5):
    """Forward + backward of windowed against full attention on the same bf16 inputs: warm-up, then ``reps`` rounds of
    ``iters`` calls per arm, the arms interleaved within every round, device-event times, medians."""
    dev = "cuda"
    qkv = torch.randn(B, S, 3, H, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    tab = torch.randn(32, H, device=dev, requires_grad=True) if bias else None
    g = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16)

    def arm(window):
        def f():
            lut = A.relative_bias_lut(tab, S, S, True, 32, 128) if bias else None
            A.attention_qkv(qkv, scale=1.0, bias_lut=lut, dropout_p=p, seed=1, window=window).backward(g)
            qkv.grad = None
        return f

    from distributed_llms_example_amd.parallel.context import chunked_attention, long_sequence_chunk
    chunk = long_sequence_chunk(S, rows=B * H)

    def full():  # what models/t5.py does for a plain T5 encoder of this length
        if chunk is None:
            return arm(None)()
        chunked_attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], chunk=chunk, scale=1.0, bias_table=tab,
                          bidirectional=True, num_buckets=32, max_distance=128, dropout_p=p, seed=1).backward(g)
        qkv.grad = None

    arms = {"window": arm(W), "same_kernels_full": arm(S), "routed_full": full}
    routes = {"window": A._route(qkv, window=W), "same_kernels_full": A._route(qkv, window=S),
              "routed_full": A._route(qkv) + (f" in {chunk}-token blocks" if chunk else "")}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for _ in range(2):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in arms}
    for _ in range(reps):
        for n, fn in arms.items():
            ms[n].append(timed(fn))
    med = {n: sorted(t)[len(t) // 2] for n, t in ms.items()}
    nb = (S + 63) // 64
    band = 2 * ((W + 63) // 64) + 1
    return {"B": B, "H": H, "S": S, "D": D, "window": W, "bias": bias, "p": p, "routes": routes,
            "ms": {n: [round(x, 4) for x in t] for n, t in ms.items()},
            "median_ms": {n: round(x, 4) for n, x in med.items()},
            "key_blocks_per_query_block": {"window": min(band, nb), "full": nb},
            "speedup_vs_same_kernels_full": med["same_kernels_full"] / med["window"],
            "speedup_vs_routed_full": med["routed_full"] / med["window"]}


def vs_global(B, H, S, W, N, bias, p, D, reps=7, iters=5):
    """Forward and backward (timed apart) of the windowed call without global keys, with key 0 global and with ``N``
    global keys at multiples of S // N: warm-up, then ``reps`` rounds of ``iters`` calls per arm, the arms interleaved
    within every round, device-event times."""
    dev = "cuda"
    qkv = torch.randn(B, S, 3, H, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    tab = torch.randn(32, H, device=dev, requires_grad=True) if bias else None
    g = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16)

    def flags(keys):
        f = torch.zeros(B, S, dtype=torch.bool, device=dev)
        f[:, keys] = True
        return A.global_keys(f)

    spread = [i * (S // N) for i in range(N)]
    arms = {"window_only": None, "key0_global": flags([0]), f"{N}_global_keys": flags(spread)}

    def fwd(gk):
        lut = A.relative_bias_lut(tab, S, S, True, 32, 128) if bias else None
        return A.attention_qkv(qkv, scale=D ** -0.5, bias_lut=lut, dropout_p=p, seed=1, window=W, global_keys=gk)

    def timed(gk):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        tf = tb = 0.0
        for _ in range(iters):
            ev[0].record()
            o = fwd(gk)
            ev[1].record()
            o.backward(g)
            ev[2].record()
            torch.cuda.synchronize()
            tf += ev[0].elapsed_time(ev[1])
            tb += ev[1].elapsed_time(ev[2])
            qkv.grad = None
        return tf / iters, tb / iters

    for _ in range(2):
        for gk in arms.values():
            timed(gk)
    ms = {n: {"fwd": [], "bwd": []} for n in arms}
    for _ in range(reps):
        for n, gk in arms.items():
            f, b = timed(gk)
            ms[n]["fwd"].append(f)
            ms[n]["bwd"].append(b)
    stat = lambda t: {"median": round(sorted(t)[len(t) // 2], 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    nb = (S + 63) // 64
    band = min(2 * ((W + 63) // 64) + 1, nb)
    return {"B": B, "H": H, "S": S, "D": D, "window": W, "bias": bias, "p": p,
            "global_keys": {"key0": [0], "spread": spread},
            "route": A._route(qkv, window=W),
            "ms": {n: {k: stat(t) for k, t in v.items()} for n, v in ms.items()},
            "key_blocks_per_query_block": {"window_only": band, "key0_global": band + 1, f"{N}_global_keys": band + N}}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--ab", action="store_true", help="repeat every case 3x")
    ap.add_argument("--head-dim", type=int, default=64)
    ap.add_argument("--vs-composite", default="", help="B,H,S,bias,kpm,causal,p: kernel against the composite")
    ap.add_argument("--window", type=int, default=None, help="with --shape: windowed against full attention")
    ap.add_argument("--global-keys", type=int, default=None,
                    help="with --window and --shape: the windowed call without, with one and with N global keys")
    ap.add_argument("--shape", default="1,32,4096,1,0.1", help="B,H,S[,bias,p] of the --window run")
    a = ap.parse_args()
    if a.global_keys is not None:
        if a.window is None or a.global_keys < 1:
            ap.error("--global-keys N (N >= 1) goes with --window")
        f = a.shape.split(",")
        print(json.dumps(vs_global(int(f[0]), int(f[1]), int(f[2]), a.window, a.global_keys,
                                   f[3] == "1" if len(f) > 3 else False, float(f[4]) if len(f) > 4 else 0.0,
                                   a.head_dim)), flush=True)
        sys.exit(0)
    if a.window is not None:
        f = a.shape.split(",")
        print(json.dumps(vs_window(int(f[0]), int(f[1]), int(f[2]), a.window, f[3] == "1" if len(f) > 3 else True,
                                   float(f[4]) if len(f) > 4 else 0.1, a.head_dim)), flush=True)
        sys.exit(0)
    if a.vs_composite:
        f = a.vs_composite.split(",")
        print(json.dumps(vs_composite(int(f[0]), int(f[1]), int(f[2]), f[3] == "1", f[4] == "1", f[5] == "1",
                                      float(f[6]), a.head_dim)), flush=True)
        sys.exit(0)
    cases = [(32, 12, 1024, 1024, True, True, False, 0.1), (32, 12, 1024, 1024, True, True, False, 0.0),
             (32, 12, 1024, 1024, False, False, False, 0.0), (32, 12, 128, 128, True, False, True, 0.1),
             (32, 12, 128, 1024, False, True, False, 0.1), (16, 16, 1024, 1024, False, True, False, 0.0)]
    if a.quick:
        cases = cases[:1]
    ap2 = a
    for c in cases:
        for rep in range(3 if ap2.ab else 1):
            print(json.dumps(run(*c, D=a.head_dim)), flush=True)
