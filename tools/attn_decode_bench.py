"""Time one decode-step attention call: csrc/attn_decode.hip (``attention_decode``) against the training forward
kernels the same call took before (DLLM_ROUTE attn_decode=0), interleaved in one process.

    python tools/attn_decode_bench.py [--shapes B,nb,H,Hkv,Sk,D,splits ...] [--sweep] [--iters 200] [--kv fp8]
``nb`` query rows per batch entry (1: self-attention on the cache, 2 / 4: the beams of a shared cross-attention),
``splits`` 0 = the launcher's choice.  ``--sweep`` times every shape at splits 1, 2, 4, ... instead (the sweep that set
FILL_PER_CU and SPLIT_FLOOR in csrc/attn_decode.hip).  One JSON line per measurement: microseconds per call (device
events around ``iters`` calls after a warm-up) and the K/V bytes per second, 2 * B * Sk * Hkv * D * 2 bytes over that
time — the bytes the op has to read, whatever a kernel reads more.  ``--kv fp8``: the FP8 K/V instantiation (e4m3 codes
and per-row scales from ``quantize_kv``) against the bf16 arm of the same kernel instead, interleaved alike, each arm
with its own bytes (``2 * D + 8`` per key and K/V head against ``4 * D``), after one line for the quantise kernel; with
``--sweep`` the split sweep of the FP8 arm.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from distributed_llms_example_amd import _ext  # noqa: E402
from distributed_llms_example_amd.ops import attention as A  # noqa: E402

DEFAULT = (
    # self-attention on the cache: B * nb rows, H = 12, D = 64
    [(r, 1, 12, 12, sk, 64, 0) for r in (16, 128, 512) for sk in (64, 128)]
    # beam-shared cross-attention
    + [(b, nb, 12, 12, sk, 64, 0) for b in (8, 64, 256) for nb in (2, 4) for sk in (512, 1024)]
    + [(b, nb, 12, 12, 16384, 64, 0) for b in (8, 64) for nb in (2, 4)]
    # grouped K/V heads at head dim 256
    + [(b, 1, 8, 4, sk, 256, 0) for b in (8, 64) for sk in (128, 1024)]
)


def timed(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=None)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--kv", choices=("bf16", "fp8"), default="bf16")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(",")) for s in a.shapes] if a.shapes else DEFAULT
    C = _ext.native()
    for B, nb, H, Hkv, Sk, D, splits in shapes:
        torch.manual_seed(0)
        q = torch.randn(B, nb, H, D, device="cuda").to(torch.bfloat16)
        k, v = (torch.randn(B, Sk, Hkv, D, device="cuda").to(torch.bfloat16) for _ in range(2))
        scale, nbytes = D ** -0.5, 2 * B * Sk * Hkv * D * 2
        rec = dict(B=B, nb=nb, H=H, Hkv=Hkv, Sk=Sk, D=D)

        def emit(arm, us, nbytes=nbytes, **kw):
            print(json.dumps(dict(rec, arm=arm, us=round(us, 2), kv_TBps=round(nbytes / us * 1e-6, 3), **kw)), flush=True)

        if a.kv == "fp8":
            kv = torch.stack((k, v), 2)  # [B, Sk, 2, Hkv, D]: a projection's layout
            qk = A.quantize_kv(kv)
            k8, v8, ks, vs = qk.codes[:, :, 0], qk.codes[:, :, 1], qk.scales[:, :, 0], qk.scales[:, :, 1]
            n8 = B * Sk * Hkv * (2 * D + 8)

            def fp8(n):
                return C.attn_decode(q, k8, v8, None, None, scale, 0.0, n, False, ks, vs)

            if a.sweep:
                n = 1
                while n == 1 or Sk // n >= 128:
                    emit("decode-fp8", timed(lambda: fp8(n), a.iters), n8, splits=n)
                    n *= 2
                continue
            # the quantiser reads the bf16 rows and writes codes + scales
            emit("quantise", timed(lambda: C.kv_quant_fp8(kv), a.iters), nbytes + n8)
            for rep in range(2):
                emit("decode-fp8", timed(lambda: fp8(splits), a.iters), n8, splits=splits, rep=rep)
                emit("decode-bf16", timed(lambda: C.attn_decode(q, kv[:, :, 0], kv[:, :, 1], None, None, scale, 0.0,
                                                                splits), a.iters), splits=splits, rep=rep)
            continue
        if a.sweep:
            n = 1
            while n == 1 or Sk // n >= 128:
                emit("decode", timed(lambda: C.attn_decode(q, k, v, None, None, scale, 0.0, n), a.iters), splits=n)
                n *= 2
            continue
        for rep in range(2):  # the two arms alternate: drift shows as a difference between the repeats
            os.environ["DLLM_ROUTE"] = "attn_decode=1"
            emit("decode", timed(lambda: C.attn_decode(q, k, v, None, None, scale, 0.0, splits), a.iters), splits=splits,
                 rep=rep)
            os.environ["DLLM_ROUTE"] = "attn_decode=0"
            emit("training-fwd", timed(lambda: A.attention_decode(q, k, v, scale=scale), a.iters), rep=rep)
    os.environ.pop("DLLM_ROUTE", None)


if __name__ == "__main__":
    main()
