"""``embed_bwd`` (csrc/embed.hip: the sorted segment-sum of the embedding gradient) against fp64, bit for bit.

The operands are exact (loss_refs.embed_operands: dy and the prior of ``out`` are multiples of 2^-3 with |x| <= 4), so
every per-id sum of <= 4099 rows plus its prior is exact in fp32 in any order: an fp32 ``out`` must EQUAL the fp64
reference, a bf16 ``out`` the reference rounded once to bf16.  Shapes: T from below one 64-row window over its edges
(63, 64, 65) to a ragged last window (130, 4099); d = 8 (one lane), 520 (idle lanes in the last wave), 2048 (the
largest).  Id patterns place runs on, across and inside window boundaries; dy is a strided view with NaN in its gaps.
"""
import pytest
import torch

import gemm_refs as G
import loss_refs as L
from distributed_llms_example_amd import _ext

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
PATTERNS = ["one", "boundary", "continue", "distinct", "pad", "nopad", "oob"]


def _ids(pattern, T, gen):
    """(ids [T] in token order, V, padding_idx).  The runs are laid out in SORTED order (what the kernel walks), then
    the tokens are shuffled."""
    V, pad = 50, -1
    if pattern == "one":  # one id for all T: a run over every window
        s = [5] * T
    elif pattern == "boundary":  # a run ending exactly at sorted position 63, the next starting exactly at 64
        s = [2] * min(T, 64) + [7] * max(T - 64, 0)
    elif pattern == "continue":  # a run continuing into window 1 (ending at 93), followed there by other ids
        s = ([1] * 10 + [4] * 84 + [6, 6, 8, 9, 9, 9] + [11] * 40 + [12] * 200)[:T]
        s += [13 + i % 30 for i in range(T - len(s))]
    elif pattern == "distinct":
        V = T + 7
        s = (torch.randperm(V, device=DEV, generator=gen)[:T]).tolist()
    elif pattern in ("pad", "nopad"):  # the pad id present: dropped with padding_idx = 3, accumulated with -1
        s = torch.randint(0, V, (T,), device=DEV, generator=gen)
        s[torch.rand(T, device=DEV, generator=gen) < 0.4] = 3
        s[0] = 3
        s, pad = s.tolist(), 3 if pattern == "pad" else -1
    else:  # ids -1 and V among valid ones: dropped, nothing written
        s = torch.randint(-1, V + 1, (T,), device=DEV, generator=gen)
        s[0], s[T - 1] = -1, V
        s = s.tolist()
    ids = torch.tensor(sorted(s), device=DEV, dtype=torch.long)
    return ids[torch.randperm(T, device=DEV, generator=gen)], V, pad


@pytest.mark.parametrize("d", [8, 520, 2048])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 130, 4099])
def test_embed_bwd_exact(T, d):
    C = _ext.native()
    F = L.Figures(f"embed_bwd T={T} d={d}")
    for pi, pattern in enumerate(PATTERNS):
        gen = torch.Generator(device=DEV).manual_seed(T * 31 + d + pi)
        ids, V, pad = _ids(pattern, T, gen)
        dy, out0 = L.embed_operands(T, d, V, DEV, gen)
        assert L.embed_headroom(ids, dy, out0, V) < G.EXACT_LIMIT
        ref = L.embed_bwd_ref(ids, dy, V, pad, out0)
        if pattern == "one":  # a contiguous dy once; everywhere else a strided view with NaN in the gaps
            dyv = dy
        else:
            buf = torch.full((T, d + 8), NAN, device=DEV, dtype=BF16)
            buf[:, :d] = dy
            dyv = buf[:, :d]
            assert dyv.stride(0) == d + 8 and dyv.data_ptr() % 16 == 0
        srt, perm = torch.sort(ids, stable=True)
        hit = torch.zeros(V, dtype=torch.bool, device=DEV)
        ok = (ids >= 0) & (ids < V) & (ids != pad)
        hit[ids[ok]] = True
        for dtype in (F32, BF16):
            outs = []
            for _ in range(2):
                out = out0.to(dtype, copy=True)  # a nonzero prior (exact in bf16 too), accumulated onto
                C.embed_bwd(srt, perm, dyv, out, pad)
                outs.append(out)
            case = f"{pattern} {'fp32' if dtype == F32 else 'bf16'}"
            bad = G.exact_mismatch(outs[0], ref, dtype)
            F.check(f"[{case}] equals the fp64 reference rounded once: {bad}", bad is None)
            F.check(f"[{case}] rows of ids that never occur bit-identical to the prior",
                    torch.equal(outs[0][~hit], out0.to(dtype)[~hit]))
            F.check(f"[{case}] rerun bit-identical", torch.equal(outs[0], outs[1]))
        if pattern != "one":
            F.check(f"[{pattern}] dy and its gaps untouched",
                    torch.equal(buf[:, :d], dy) and bool(buf[:, d:].isnan().all()))
    print(f"[fig] embed_bwd T={T} d={d}: {len(PATTERNS)} id patterns x (fp32, bf16) exact: "
          f"{'ok' if not F.bad else 'FAILED'}")
    F.done()
