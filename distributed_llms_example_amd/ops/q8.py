"""Block-wise 8-bit optimizer state (Dettmers et al. 2022, "8-bit Optimizers via Block-wise Quantization"): the two
"dynamic" code books, and quantise / dequantise as torch composites.

The contract (this file states it exactly and runs on the CPU; csrc/adamw_q8.hip is tested against it):

* code books, 256 sorted fp32 entries each, built in fp64 and rounded once.  Signed (``exp_avg``): for ``i`` in 0..6
  the ``2**i`` midpoints of an even partition of [0.1, 1] into ``2**i`` intervals, times ``10**(i - 6)``, with both
  signs; plus ``0.0`` and ``1.0`` (so ``+1.0`` is an entry, ``-1.0`` is not: the lowest is about -0.99297).  Unsigned
  (``exp_avg_sq``): ``2**(i + 1)`` positive midpoints per ``i`` and no negative side; plus ``0.0`` and ``1.0``.
  Nobody has compared these tables with a state file serialised by bitsandbytes: no interchange is promised;
* a block is ``BLOCK`` = 64 consecutive flat elements with one fp32 scale ``absmax = max |x|`` per state;
* quantise: ``x = value / absmax`` (one fp32 division; an all-zero block has ``x = 0``); ``code`` = the number of fp32
  midpoints ``(T[i] + T[i+1]) / 2`` strictly below ``x``: the nearest entry, ties to the lower code;
* dequantise: ``T[code] * absmax``, one fp32 multiply.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

BLOCK = 64


def _book(signed: bool) -> np.ndarray:
    vals = [0.0, 1.0]
    for i in range(7):
        k = 2 ** i if signed else 2 ** (i + 1)
        edges = np.linspace(0.1, 1.0, k + 1, dtype=np.float64)
        mids = (edges[:-1] + edges[1:]) / 2.0 * 10.0 ** (i - 6)
        vals += mids.tolist()
        if signed:
            vals += (-mids).tolist()
    t = np.sort(np.asarray(vals, dtype=np.float64)).astype(np.float32)
    assert t.size == 256 and np.unique(t).size == 256 and np.all(np.diff(midpoints(t)) > 0), "code book construction"
    return t


def midpoints(book: np.ndarray) -> np.ndarray:
    """The 255 fp32 midpoints of a code book (the sum of two fp32 neighbours is exact in fp64: one rounding)."""
    return ((book[:-1].astype(np.float64) + book[1:].astype(np.float64)) / 2.0).astype(np.float32)


SIGNED = _book(True)
UNSIGNED = _book(False)


@functools.lru_cache(maxsize=None)
def tables(device: str) -> torch.Tensor:
    """fp32 [1024] on ``device``: signed book | unsigned book | signed midpoints | unsigned midpoints (each padded to
    256 with +inf) — what csrc/adamw_q8.hip stages in LDS, and what the composite indexes."""
    pad = np.array([np.inf], dtype=np.float32)
    return torch.from_numpy(np.concatenate([SIGNED, UNSIGNED, midpoints(SIGNED), pad, midpoints(UNSIGNED), pad])
                            ).to(device)


def _parts(signed: bool, device) -> tuple[torch.Tensor, torch.Tensor]:
    t = tables(str(device))
    return (t[0:256], t[512:767]) if signed else (t[256:512], t[768:1023])


def quantize(x: torch.Tensor, signed: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """``(codes uint8 [nblk, 64], absmax fp32 [nblk])`` of a flat fp32 ``x`` of whole blocks."""
    blocks = x.float().reshape(-1, BLOCK)
    absmax = blocks.abs().amax(-1)
    v = blocks / absmax.unsqueeze(-1)
    v = torch.where(absmax.unsqueeze(-1) == 0, torch.zeros_like(v), v)
    _, mid = _parts(signed, x.device)
    return torch.bucketize(v, mid).to(torch.uint8), absmax  # bucketize: the number of midpoints < v


def dequantize(codes: torch.Tensor, absmax: torch.Tensor, signed: bool) -> torch.Tensor:
    """Flat fp32 ``T[code] * absmax`` of ``codes [nblk, 64]`` and ``absmax [nblk]``."""
    book, _ = _parts(signed, codes.device)
    return (book[codes.reshape(-1, BLOCK).long()] * absmax.unsqueeze(-1)).reshape(-1)
