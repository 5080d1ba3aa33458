"""Low-rank adapters (LoRA) on a frozen linear layer: ``y = mod(x)`` plus, per adapter, ``s · dropout(x) Aᵀ Bᵀ`` added
into the adapter's output column slice ``[c0, c0 + n)``.

The projections of this framework are fused (q|k|v in one weight, k|v, gate|up), so an adapter is defined on a column
slice of the fused output: ``q`` and ``v`` of a fused ``qkv`` are two adapters on one linear layer.  All adapters of a
layer share its input and ONE dropout seed per forward.

Semantics (the composite below states them exactly, the kernels of csrc/lora.hip are tested against it):

* ``keep = rowwise_keep_mask(seed, p, rows, in_features)`` (ops/rng.py, the row hash the FFN kernels use); the mask
  zeroes elements of ``x``; the ``1 / (1 - p)`` factor multiplies the fp32 product;
* ``t = (keep ⊙ x) Aᵀ / (1 - p)`` accumulated in fp32 and rounded to the activation dtype (as PEFT's ``lora_A``
  module output would be);
* ``y[:, c0:c0+n] += s · t Bᵀ`` accumulated in fp32 and added to ``y`` with one rounding;
* backward, with ``dY_s = dY[:, c0:c0+n]``: ``dt = s · dY_s B`` (rounded to the activation dtype),
  ``dB += s · dY_sᵀ t``, ``dA += dtᵀ (keep ⊙ x) / (1 - p)``, ``dx += keep ⊙ (dt A) / (1 - p)`` added into the base
  layer's input gradient with one rounding.  The mask is regenerated from the seed: nothing the size of the activation
  is saved besides ``x`` itself (and the ``[tokens, r]`` ``t``).

Routes (ops/routing.py ``lora``): ``fused`` = csrc/lora.hip (bf16 on the GPU; ``lora_down`` streams x once with the mask
applied to the loaded operand, ``lora_up`` reads and writes the output slice once, ``lora_wgrad`` reduces over tokens in
fixed splits summed in order, straight into the flat gradient buffer); ``lib`` = the composite on the GPU (torch matmuls
on hipBLASLt).  fp32 models, CPU tensors, ``DLLM_REFERENCE_OPS=1`` and shapes off the kernels' grid (feature counts or
slice offsets that are not multiples of 8) run the composite.

The base layer must be frozen (models/lora.py ``apply_lora`` freezes it): its forward runs through ``linear_fwd``, its
input gradient through ``linear_dgrad`` (ops/gemm.py), and it has no weight gradient.  Adapter gradients accumulate into
``_gbuf(p)`` with ``_use`` / ``_fire`` exactly as ops/linear.py ``_LinearAccumFn`` does, every micro-batch (deferred
weight gradients do not apply to them); without FlatParams they come back through autograd.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import _ext
from . import routing
from .gemm import linear_dgrad, linear_fwd
from .linear import _fire, _fusable, _gbuf, _use
from .rng import default_rng, rowwise_keep_mask

fused_calls = 0  # adapted linear forwards that ran on csrc/lora.hip (tests assert the kernels really ran)
lib_calls = 0    # ... that ran the composite


@dataclass
class Adapter:
    """One low-rank update of the output columns ``[c0, c0 + n)`` of a linear layer: ``A`` [r, in], ``B`` [n, r]."""
    name: str        # logical target (q, k, v, o, wi, wi_0, wi_1, wo)
    c0: int
    n: int
    A: torch.nn.Parameter
    B: torch.nn.Parameter
    scale: float


def _wide(t: torch.Tensor) -> torch.Tensor:
    """``t`` in the accumulation type: fp32 for 16-bit tensors, the tensor's own type otherwise."""
    return t.float() if t.dtype in (torch.bfloat16, torch.float16) else t


def _mm32(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """``a @ b`` accumulated and returned in fp32 (fp32 / fp64 operands: their own type): the library's fp32-output
    GEMM for bf16 GPU operands, else a matmul of the widened operands."""
    if a.is_cuda and a.dtype == torch.bfloat16 and not _ext.force_reference():
        return torch.mm(a, b, out_dtype=torch.float32)
    return torch.mm(_wide(a), _wide(b))


def _dropped(x2: torch.Tensor, p: float, seed: int) -> torch.Tensor:
    if p <= 0.0:
        return x2
    return x2 * rowwise_keep_mask(seed, p, x2.shape[0], x2.shape[1], x2.device).to(x2.dtype)


def composite_forward(x2, y2, slices, ab, p, seed):
    """The adapters' forward on the base output ``y2`` (updated in place); returns the ``t`` of every adapter."""
    inv = 1.0 / (1.0 - p)
    xd = _dropped(x2, p, seed)
    ts = []
    for i, (c0, n, s) in enumerate(slices):
        A, B = ab[2 * i], ab[2 * i + 1]
        t = (_mm32(xd, A.t()) * inv).to(x2.dtype)
        ys = y2[:, c0:c0 + n]
        ys.copy_((_wide(ys) + _mm32(t, B.t()) * s).to(y2.dtype))
        ts.append(t)
    return ts


def composite_backward(x2, dy2, dx2, slices, ab, ts, p, seed, sinks):
    """The adapters' backward: ``dx2`` (None: not wanted) updated in place, ``sinks[2i]`` / ``sinks[2i+1]`` (fp32 or
    parameter-dtype matrices) accumulated with dA / dB."""
    inv = 1.0 / (1.0 - p)
    keep = rowwise_keep_mask(seed, p, x2.shape[0], x2.shape[1], x2.device).to(x2.dtype) if p > 0.0 else None
    xd = x2 if keep is None else x2 * keep
    for i, (c0, n, s) in enumerate(slices):
        A, B = ab[2 * i], ab[2 * i + 1]
        dys = dy2[:, c0:c0 + n]
        dt = (_mm32(dys, B) * s).to(x2.dtype)
        gB, gA = sinks[2 * i + 1], sinks[2 * i]
        gB.add_((_mm32(dys.t(), ts[i]) * s).to(gB.dtype))
        gA.add_((_mm32(dt.t(), xd) * inv).to(gA.dtype))
        if dx2 is not None:
            upd = _mm32(dt, A)
            if keep is not None:
                upd = upd * keep
            dx2.copy_((_wide(dx2) + upd * inv).to(dx2.dtype))


def _kernel_ok(x2: torch.Tensor, out_features: int, slices) -> bool:
    """The csrc/lora.hip grid: bf16 on the GPU, feature counts and slice bounds multiples of 8, 16-B aligned rows."""
    if x2.dtype != torch.bfloat16 or not _ext.use_native(x2) or routing.get("lora") != "fused":
        return False
    if x2.shape[1] % 8 or out_features % 8 or x2.data_ptr() % 16 or not x2.is_contiguous():
        return False
    return all(c0 % 8 == 0 and n % 8 == 0 for c0, n, _ in slices)


def _rows16(t2: torch.Tensor) -> torch.Tensor:
    """``t2`` [N, C] as the kernels take a wide operand: unit inner stride, row stride % 8, 16-B aligned."""
    if t2.stride(1) == 1 and t2.stride(0) % 8 == 0 and t2.data_ptr() % 16 == 0:
        return t2
    return t2.contiguous()


def _forward(x, w, b, slices, p, seed, ab):
    """(x2, y2, [t per adapter], ran on csrc/lora.hip): the frozen base GEMM and the adapters' updates of its output."""
    global fused_calls, lib_calls
    x2 = x.reshape(-1, x.shape[-1])
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    y = linear_fwd(x2, w, b)  # a fresh [N, out] tensor: the adapters update it in place
    fused = _kernel_ok(x2, y.shape[1], slices)
    if fused:
        C = _ext.native()
        fused_calls += 1
        inv = 1.0 / (1.0 - p)
        ts = []
        for i, (c0, n, s) in enumerate(slices):
            t = C.lora_down(x2, ab[2 * i], inv, p, seed, 0)
            C.lora_up(t, ab[2 * i + 1], False, s, y, c0, n, 0.0, 0, 0)
            ts.append(t)
    else:
        lib_calls += 1
        ts = composite_forward(x2, y, slices, ab, p, seed)
    return x2, y, ts, fused


class _LoraLinearFn(torch.autograd.Function):
    """Frozen base linear + its adapters.  ``ab`` = (A0, B0, A1, B1, ...): detached when their gradients accumulate
    into the flat buffer (``params`` then carries the Parameters), else the Parameters themselves (autograd)."""

    @staticmethod
    def forward(ctx, x, w, b, slices, p, seed, params, *ab):
        x2, y, ts, fused = _forward(x, w, b, slices, p, seed, ab)
        ctx.save_for_backward(x2, w, *ts, *ab)
        ctx.cfg = (slices, p, seed, fused, x.shape)
        ctx.params = params
        for q in params or ():
            _use(q)
        return y.view(*x.shape[:-1], y.shape[1])

    @staticmethod
    def backward(ctx, dy):
        saved = ctx.saved_tensors
        slices, p, seed, fused, shape = ctx.cfg
        na = len(slices)
        x2, w = saved[0], saved[1]
        ts, ab = saved[2:2 + na], saved[2 + na:]
        params = ctx.params
        dy2 = dy.reshape(-1, dy.shape[-1])
        dx2 = linear_dgrad(dy2, w) if ctx.needs_input_grad[0] else None
        if dx2 is not None and not dx2.is_contiguous():
            dx2 = dx2.contiguous()
        with torch.no_grad():
            if params is not None:
                sinks = [_gbuf(q) for q in params]
            else:
                sinks = [torch.zeros(t.shape, dtype=_wide(t).dtype, device=t.device) for t in ab]
            if fused:
                C = _ext.native()
                inv = 1.0 / (1.0 - p)
                dyk = _rows16(dy2)
                for i, (c0, n, s) in enumerate(slices):
                    A, B = ab[2 * i], ab[2 * i + 1]
                    dys = dyk[:, c0:c0 + n]
                    dt = C.lora_down(dys, B.t().contiguous(), s, 0.0, 0, 0)
                    C.lora_wgrad(dys, ts[i], s, sinks[2 * i + 1], True, True, 0.0, 0, 0)
                    C.lora_wgrad(x2, dt, inv, sinks[2 * i], False, True, p, seed, 0)
                    if dx2 is not None:
                        C.lora_up(dt, A, True, inv, dx2, 0, x2.shape[1], p, seed, 0)
            else:
                composite_backward(x2, dy2, dx2, slices, ab, ts, p, seed, sinks)
        dx = None if dx2 is None else dx2.view(shape)
        if params is not None:
            for q in params:
                _fire(q)
            return (dx, None, None, None, None, None, None) + (None,) * len(ab)
        return (dx, None, None, None, None, None, None) + tuple(g.to(t.dtype) for g, t in zip(sinks, ab))


def lora_linear(x: torch.Tensor, mod, adapters, p: float = 0.0, seed: int = 0) -> torch.Tensor:
    """``mod(x)`` plus every adapter's ``scale · (keep ⊙ x / (1 - p)) Aᵀ Bᵀ`` added into its column slice (module
    docstring).  ``mod``: a linear layer with a frozen ``weight`` / ``bias``; ``adapters``: :class:`Adapter` list."""
    w, b = mod.weight, mod.bias
    if w.requires_grad or (b is not None and b.requires_grad):
        raise NotImplementedError("lora_linear needs a frozen base layer (models/lora.py apply_lora freezes it)")
    slices = tuple((ad.c0, ad.n, float(ad.scale)) for ad in adapters)
    plist = [q for ad in adapters for q in (ad.A, ad.B)]
    if not torch.is_grad_enabled():
        _, y, _, _ = _forward(x, w, b, slices, float(p), int(seed), [q.detach() for q in plist])
        return y.view(*x.shape[:-1], y.shape[1])
    if all(_fusable(q) for q in plist):
        # fresh leaves over the adapters' storage give the output a grad_fn even when x carries no gradient (the first
        # adapted layer of a frozen model) without an edge to the Parameters' AccumulateGrad (ops/embedding.py)
        return _LoraLinearFn.apply(x, w, b, slices, float(p), int(seed), tuple(plist),
                                   *[q.detach().requires_grad_(True) for q in plist])
    return _LoraLinearFn.apply(x, w, b, slices, float(p), int(seed), None, *plist)


def adapted_forward(mod, x: torch.Tensor) -> torch.Tensor:
    """``Linear.forward`` of a layer that carries adapters (``mod._lora``: (adapters, dropout p))."""
    adapters, p = mod._lora
    p = p if mod.training else 0.0
    seed = default_rng().next_seed() if p > 0 else 0
    return lora_linear(x, mod, adapters, p, seed)
