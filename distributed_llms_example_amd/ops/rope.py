"""Rotary position embedding (rotate-half RoPE: Gemma 2 / T5Gemma self-attention).

``rope_table(theta, D, max_pos)`` builds ``cos`` / ``sin`` ``[max_pos, D/2]`` in fp32 with transformers' arithmetic
(modeling_t5gemma.py T5GemmaRotaryEmbedding: ``inv_freq = 1 / theta ** (arange(0, D, 2) / D)``, the outer product with
the positions in fp32, then ``.cos()`` / ``.sin()``; its two concatenated halves are equal, so half the table is kept).

``rope(x, pos, cos, sin)`` rotates ``x [B, S, n, H, D]`` — the ``n`` listed slots of a packed projection output: q and
k of a fused qkv (``qkv[:, :, :2]``), or a lone q or k (``q.unsqueeze(2)``); v is left out of the view and so
untouched — by ``(x1, x2) -> (x1 c - x2 s, x2 c + x1 s)`` on the halves ``d`` and ``d + D/2`` with ``c`` / ``s`` the
table rows of ``pos`` (``[S]`` or ``[B, S]``, any integer dtype).  Products and sums are fp32 and the result is rounded
once to the tensor's dtype: the contract, and more exact than transformers' own bf16 products (it rounds cos / sin and
every product to the activation dtype).  The rotation is orthogonal, so the backward is the same op with ``-s``.

Kernel: csrc/rope.hip (``rope_fwd``, in place on a strided view; bf16 at ``D % 16 == 0``, fp32 at ``D % 8 == 0``).
The autograd op rotates a dense copy of the packed tensor, v included (its input stays as it is), and its backward a
dense copy of the incoming gradient: two extra passes over the packed tensor per self-attention, not yet removed by
rotating the projection's output in place.  On CPU tensors, with ``DLLM_REFERENCE_OPS=1`` and at other head dims
(one warning) the torch reference below runs; it is also the test oracle.
"""
from __future__ import annotations

import torch

from .. import _ext
from ..utils.logging import get_logger

_tables: dict = {}


def rope_table(theta: float, D: int, max_pos: int, device="cpu") -> tuple[torch.Tensor, torch.Tensor]:
    """``(cos, sin)`` fp32 ``[max_pos, D/2]`` on ``device``, built on the host once per (theta, D, max_pos, device)."""
    if D % 2 or D <= 0 or max_pos <= 0:
        raise ValueError(f"rope_table: head dim must be even and max_pos positive, got {D} and {max_pos}")
    key = (float(theta), int(D), int(max_pos), str(device))
    hit = _tables.get(key)
    if hit is None:
        inv_freq = 1.0 / (float(theta) ** (torch.arange(0, D, 2, dtype=torch.float) / D))
        freqs = torch.outer(torch.arange(max_pos, dtype=torch.float), inv_freq)
        hit = (freqs.cos().contiguous().to(device), freqs.sin().contiguous().to(device))
        if len(_tables) >= 64:  # the oldest entry only: tables in use (a captured step reads them by address) are
            _tables.pop(next(iter(_tables)))  # the recent ones, and their users hold them besides (models/t5gemma.py)
        _tables[key] = hit
    return hit


def _reference(x, pos, cos, sin, sign: float = 1.0):
    """The definition on ``x [B, S, n, H, D]``: fp32 arithmetic, rounded once to ``x.dtype``."""
    half = x.shape[-1] // 2
    idx = pos.long().to(cos.device)
    c = cos.index_select(0, idx.reshape(-1)).view(*idx.shape, half).to(x.device)
    s = sin.index_select(0, idx.reshape(-1)).view(*idx.shape, half).to(x.device) * sign
    if idx.dim() == 1:
        c, s = c[None], s[None]
    c, s = c[:, :, None, None, :], s[:, :, None, None, :]
    xf = x.float()
    x1, x2 = xf[..., :half], xf[..., half:]
    return torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), -1).to(x.dtype)


_warned: set = set()


def _native_ok(x) -> bool:
    if not _ext.use_native(x):
        return False
    e = 8 if x.dtype == torch.bfloat16 else 4
    ok = (x.dtype in (torch.bfloat16, torch.float32) and x.shape[-1] % (2 * e) == 0 and x.stride(-1) == 1
          and all(st % e == 0 for st in x.stride()[:-1]) and x.data_ptr() % 16 == 0)
    if not ok and "shape" not in _warned:
        _warned.add("shape")
        get_logger().warning("rope: no HIP kernel for head dim %d in %s with these strides; running the torch "
                             "reference (csrc/rope.hip takes 16-byte chunks per half)", x.shape[-1],
                             str(x.dtype).replace("torch.", ""))
    return ok


def _pos32(pos, device):
    return pos.to(device=device, dtype=torch.int32).contiguous()


class _RopeFn(torch.autograd.Function):
    """``packed`` with its first ``n`` slots (dim 2) rotated; the other slots (v) are copied as they are."""

    @staticmethod
    def forward(ctx, packed, n, pos, cos, sin):
        out = packed.clone(memory_format=torch.contiguous_format)
        _ext.native().rope_fwd(out[:, :, :n], pos, cos, sin, 1.0)
        ctx.save_for_backward(pos, cos, sin)
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx, g):
        pos, cos, sin = ctx.saved_tensors
        # the incoming gradient may be shared with other consumers of autograd's: always rotated on a dense copy
        g = g.clone(memory_format=torch.contiguous_format)
        _ext.native().rope_fwd(g[:, :, :ctx.n], pos, cos, sin, -1.0)
        return g, None, None, None, None


def rope(packed: torch.Tensor, pos: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, slots: int | None = None):
    """``packed [B, S, N, H, D]`` with its first ``slots`` slots (default: all ``N``) rotated by the positions ``pos``
    (``[S]`` or ``[B, S]``); the rest is returned unchanged.  ``cos`` / ``sin`` from :func:`rope_table`."""
    if packed.dim() != 5:
        raise ValueError(f"rope: expected [B, S, N, H, D], got {tuple(packed.shape)}")
    n = packed.shape[2] if slots is None else int(slots)
    if not 0 < n <= packed.shape[2]:
        raise ValueError(f"rope: slots must be in 1 .. {packed.shape[2]}, got {slots}")
    if cos.shape != sin.shape or cos.dim() != 2 or cos.shape[1] * 2 != packed.shape[-1]:
        raise ValueError(f"rope: cos / sin must be [max_pos, {packed.shape[-1] // 2}], got {tuple(cos.shape)}")
    if pos.dim() not in (1, 2) or pos.shape[-1] != packed.shape[1] or (pos.dim() == 2 and pos.shape[0] != packed.shape[0]):
        raise ValueError(f"rope: pos must be [S] or [B, S] for x {tuple(packed.shape)}, got {tuple(pos.shape)}")
    if _native_ok(packed):
        return _RopeFn.apply(packed, n, _pos32(pos, packed.device), cos, sin)
    rot = _reference(packed[:, :, :n], pos, cos, sin)
    return rot if n == packed.shape[2] else torch.cat((rot, packed[:, :, n:]), 2)
