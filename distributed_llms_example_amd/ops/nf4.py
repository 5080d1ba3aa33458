"""NF4 (QLoRA, Dettmers et al. 2023) frozen base weights: 4-bit codes in blocks of 64 with one fp32 scale each.

The contract (the torch composite below states it exactly and runs on the CPU; the kernels of csrc/nf4.hip are tested
against it):

* code book ``NF4[16]`` (fp32) below;
* storage of ``W [N, K]`` (``nn.Linear`` layout, ``N % 64 == 0`` and ``K % 64 == 0``): ``codes`` uint8 ``[N, K/2]``,
  byte ``j`` of a row holding element ``2j`` in the high nibble and ``2j+1`` in the low one (bitsandbytes' documented
  nibble order); ``absmax`` fp32 ``[N, K/64]``, block ``b`` of a row covering elements ``64b .. 64b+63``.  The only
  layout: the kernels read it as it stands.  The scales are not quantised again (no double quantisation);
* ``quantize_nf4``: ``absmax`` = the block's max |w| in fp32; ``v = w / absmax`` (one fp32 division; a block with
  ``absmax == 0`` gets code 7 everywhere); code = the number of midpoints ``m_i = (NF4[i] + NF4[i+1]) * 0.5`` (fp32)
  with ``v > m_i``: the nearest entry, ties to the lower code.  Every step is one correctly rounded fp32 operation, so
  torch on the CPU and the kernel agree bit for bit;
* ``dequantize_nf4``: ``w' = round_to_dtype(NF4[code] * absmax)``, one fp32 multiply and one rounding.  The bf16 GEMM
  on a quantised layer IS the bf16 GEMM on ``dequantize_nf4(..., bf16)`` with fp32 accumulation.

Requantising a bf16 weight that came from ``dequantize_nf4`` returns the same codes and scales: the block's extreme
code is +-1, so ``absmax`` must itself be bf16-representable for that (it is, when the weight quantised was bf16), and
the bf16 rounding (2^-9 relative) is far below the code book's smallest half-gap.

Routes (ops/routing.py ``nf4``): ``fused`` = ``gemm_nf4`` of csrc/nf4.hip reads the codes in the GEMM (NT forward, NN
input gradient) for calls within ``nf4_fused_max_rows`` rows and ``nf4_fused_max_depth`` of reduction, where it was
measured faster (profiles/nf4_gemm.txt); beyond them, and under ``dequant``: ``nf4_dequant`` into a transient bf16
weight, then ``linear_fwd`` / ``linear_dgrad`` (ops/gemm.py).  fp32 models, CPU tensors, ``DLLM_REFERENCE_OPS=1`` and misaligned operands run the composite
(``dequantize_nf4`` + a torch matmul).  Autograd saves the code and scale buffers, never a dequantised weight.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import _ext
from . import routing
from .gemm import linear_dgrad, linear_fwd

NF4 = (-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635,
       -0.18477343022823334, -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725,
       0.24611230194568634, 0.33791524171829224, 0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0)
BLOCK = 64

fused_calls = 0    # quantised GEMMs that ran on csrc/nf4.hip's gemm_nf4 (tests assert the kernels really ran)
dequant_calls = 0  # ... that dequantised into a transient bf16 weight for the library GEMM


def quantizable(out_features: int, in_features: int) -> bool:
    return out_features % BLOCK == 0 and in_features % BLOCK == 0


def nbytes(out_features: int, in_features: int) -> int:
    """Bytes of a quantised ``[out, in]`` weight: 4-bit codes + one fp32 scale per 64."""
    return out_features * in_features // 2 + 4 * out_features * in_features // BLOCK


def _table(device) -> torch.Tensor:
    return torch.tensor(NF4, dtype=torch.float32, device=device)


def quantize_nf4(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``(codes uint8 [N, K/2], absmax fp32 [N, K/64])`` of ``w [N, K]`` (module docstring)."""
    N, K = w.shape
    if not quantizable(N, K):
        raise ValueError(f"quantize_nf4: N and K must be multiples of {BLOCK}, got {tuple(w.shape)}")
    if w.is_cuda and w.dtype in (torch.bfloat16, torch.float32) and w.is_contiguous() and _ext.use_native(w):
        codes, absmax = _ext.native().nf4_quantize(w.detach())
        return codes, absmax
    blocks = w.detach().float().reshape(N, K // BLOCK, BLOCK)
    absmax = blocks.abs().amax(-1)
    v = blocks / absmax.unsqueeze(-1)
    t = _table(w.device)
    code = torch.bucketize(v, (t[:-1] + t[1:]) * 0.5)  # number of midpoints < v
    code = torch.where(absmax.unsqueeze(-1) == 0, torch.full_like(code, 7), code).reshape(N, K // 2, 2)
    return ((code[..., 0] << 4) | code[..., 1]).to(torch.uint8), absmax


def dequantize_nf4(codes: torch.Tensor, absmax: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """``[N, K]`` in ``dtype``: ``NF4[code] * absmax`` in fp32, rounded once."""
    N, K = codes.shape[0], codes.shape[1] * 2
    idx = torch.stack((codes >> 4, codes & 15), dim=-1).reshape(N, K // BLOCK, BLOCK).long()
    return (_table(codes.device)[idx] * absmax.unsqueeze(-1)).reshape(N, K).to(dtype)


def _route(x2: torch.Tensor, bias) -> str:
    """``fused`` / ``dequant`` (csrc/nf4.hip: bf16 on the GPU) or ``composite``."""
    if x2.dtype != torch.bfloat16 or not _ext.use_native(x2):
        return "composite"
    if bias is not None and (bias.dtype != torch.bfloat16 or not bias.is_contiguous() or bias.data_ptr() % 8):
        return "composite"
    # fused where it was measured faster than dequant in every repetition (profiles/nf4_gemm.txt): up to 1024 rows and
    # a reduction (x2's columns) up to 1024 deep; past either the k-loop's per-step latency loses to the library GEMM
    if (routing.get("nf4") == "fused" and x2.shape[0] <= routing.get("nf4_fused_max_rows")
            and x2.shape[1] <= routing.get("nf4_fused_max_depth")):
        return "fused"
    return "dequant"


def _fwd2(x2: torch.Tensor, codes, absmax, bias) -> torch.Tensor:
    """``x2 [M, K] · deq(W)ᵀ (+ bias)``: a fresh ``[M, N]`` tensor."""
    global fused_calls, dequant_calls
    route = _route(x2, bias)
    if route == "composite":
        return F.linear(x2, dequantize_nf4(codes, absmax, x2.dtype), bias)
    C = _ext.native()
    if route == "fused":
        from .lora import _rows16
        fused_calls += 1
        return C.gemm_nf4(_rows16(x2), codes, absmax, bias, False)
    dequant_calls += 1
    return linear_fwd(x2, C.nf4_dequant(codes, absmax), bias)


def _dgrad2(dy2: torch.Tensor, codes, absmax) -> torch.Tensor:
    """``dy2 [M, N] · deq(W)``: a fresh ``[M, K]`` tensor."""
    global fused_calls, dequant_calls
    route = _route(dy2, None)
    if route == "composite":
        return dy2 @ dequantize_nf4(codes, absmax, dy2.dtype)
    C = _ext.native()
    if route == "fused":
        from .lora import _rows16
        fused_calls += 1
        return C.gemm_nf4(_rows16(dy2), codes, absmax, None, True)
    dequant_calls += 1
    return linear_dgrad(dy2, C.nf4_dequant(codes, absmax))


def nf4_linear_fwd(x: torch.Tensor, mod) -> torch.Tensor:
    """The forward of the quantised layer ``mod`` (buffers ``weight_nf4`` / ``weight_absmax``, bias as it was)."""
    y = _fwd2(x.reshape(-1, x.shape[-1]), mod.weight_nf4, mod.weight_absmax, mod.bias)
    return y.view(*x.shape[:-1], y.shape[1])


def nf4_linear_dgrad(dy: torch.Tensor, mod) -> torch.Tensor:
    """The input gradient of the quantised layer ``mod`` for the output gradient ``dy``."""
    dx = _dgrad2(dy.reshape(-1, dy.shape[-1]), mod.weight_nf4, mod.weight_absmax)
    return dx.view(*dy.shape[:-1], dx.shape[1])


class _Nf4LinearFn(torch.autograd.Function):
    """A quantised layer without adapters: forward and input gradient (ops/linear.py ``_FrozenLinearFn``'s shape);
    saves the code and scale buffers only."""

    @staticmethod
    def forward(ctx, x, codes, absmax, bias):
        ctx.save_for_backward(codes, absmax)
        y = _fwd2(x.reshape(-1, x.shape[-1]), codes, absmax, bias)
        return y.view(*x.shape[:-1], y.shape[1])

    @staticmethod
    def backward(ctx, dy):
        codes, absmax = ctx.saved_tensors
        dx = _dgrad2(dy.reshape(-1, dy.shape[-1]), codes, absmax)
        return dx.view(*dy.shape[:-1], dx.shape[1]), None, None, None


def nf4_forward(mod, x: torch.Tensor) -> torch.Tensor:
    """``Linear.forward`` of a quantised layer that carries no adapters."""
    if torch.is_grad_enabled() and x.requires_grad:
        return _Nf4LinearFn.apply(x, mod.weight_nf4, mod.weight_absmax, mod.bias)
    return nf4_linear_fwd(x, mod)
