"""Fused (label-smoothed) cross-entropy over the LM-head logits.

Matches ``CrossEntropyLoss(ignore_index=-100)`` used inside T5/BART (transformers
modeling_t5.py:1050-1054, modeling_bart.py:942-946) and the Trainer's LabelSmoother
``(1-eps)*nll + eps*mean_v(-logp_v)`` over non-ignored tokens (trainer_pt_utils.py:437-483).
BART's ``final_logits_bias`` (modeling_bart.py:940) is added inside the kernel instead of
materialising ``logits + bias``.

The forward kernel makes one online-softmax pass per row (fp32 math on bf16 logits) and keeps only
``lse`` per row; the backward kernel writes ``softmax - target`` straight into the logits buffer
(``inplace_grad=True``) so no second ``[N, V]`` tensor is allocated.  Kernels: csrc/ce.hip.

``softcap=c`` (Gemma 2 / T5Gemma ``final_logit_softcapping``): the loss is taken on ``c * tanh(x / c)`` (after the
bias), formed inside the kernels' one pass; the backward writes ``dx = dx' * (1 - tanh^2)``.
"""
from __future__ import annotations

import torch

from .. import _ext


def _check_softcap(softcap) -> float | None:
    if softcap is None:
        return None
    c = float(softcap)
    if not (c > 0.0 and c != float("inf")):
        raise ValueError(f"cross_entropy: softcap must be a finite number > 0 or None, got {softcap}")
    return c


def _reference(logits, labels, bias, smoothing, ignore_index, softcap=None):
    x = logits.float()
    if bias is not None:
        x = x + bias.float().view(1, -1)
    if softcap is not None:
        x = softcap * torch.tanh(x / softcap)
    return torch.nn.functional.cross_entropy(x, labels, ignore_index=ignore_index, label_smoothing=smoothing)


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, bias, smoothing, ignore_index, inplace_grad, softcap=None):
        C = _ext.native()
        cap = {} if softcap is None else {"softcap": float(softcap)}
        ctx.cap = cap
        loss_rows, lse = C.ce_fwd(logits, labels, bias, float(smoothing), int(ignore_index), **cap)
        valid = (labels != ignore_index)
        count = valid.sum().clamp_min(1).to(torch.float32)
        ctx.save_for_backward(logits, labels, bias, lse, count)
        ctx.cfg = (smoothing, ignore_index, inplace_grad)
        return loss_rows.sum() / count

    @staticmethod
    def backward(ctx, g):
        C = _ext.native()
        logits, labels, bias, lse, count = ctx.saved_tensors
        smoothing, ignore_index, inplace = ctx.cfg
        scale = (g.float() / count).reshape(1)
        dlogits = C.ce_bwd(scale, logits, labels, lse, bias, float(smoothing), int(ignore_index), bool(inplace),
                           **ctx.cap)
        return dlogits, None, None, None, None, None, None


def cross_entropy(logits, labels, *, bias=None, label_smoothing: float = 0.0, ignore_index: int = -100,
                  inplace_grad: bool = False, softcap: float | None = None):
    """Mean CE over rows with ``labels != ignore_index``.  logits ``[N, V]``, labels ``[N]``; ``softcap``: the loss
    of ``c * tanh(logits / c)`` (None: no cap)."""
    softcap = _check_softcap(softcap)
    if _ext.use_native(logits):
        return _CEFn.apply(logits.contiguous(), labels.contiguous(), bias, label_smoothing, ignore_index,
                           inplace_grad, softcap)
    return _reference(logits, labels, bias, label_smoothing, ignore_index, softcap)
