"""Knowledge-distillation loss over a student's and a frozen teacher's LM-head logits.

Per target row with student logits ``s`` (+ the student's logits bias), teacher logits ``t`` (+ the teacher's), label
``y``, smoothing ``eps``, temperature ``T > 0`` and weight ``alpha`` in [0, 1]::

    ce_r = lse(s) - (1-eps) s_y - eps mean_v(s_v)                          (ops/cross_entropy.py)
    kl_r = sum_v p_v (log p_v - log q_v),   p = softmax(t/T), q = softmax(s/T)
    loss = sum_{r: y_r != ignore} [(1-alpha) ce_r + alpha T^2 kl_r] / max(1, #non-ignored rows)

(Hinton et al. 2015: the T^2 keeps the soft-target gradients at the scale of the hard-target ones.)  The gradient
reaches the student logits only: ``(g / count) [(1-alpha)(softmax(s) - eps/V - (1-eps)[v==y]) + alpha T (q - p)]``.

GPU path (csrc/kd.hip, ops/routing.py ``kd`` = fused): ``kd_fwd`` makes ONE pass over both ``[N, V]`` tensors with
three online softmaxes per row and keeps ``{lse(s), lse(s/T), lse(t/T)}``; ``kd_bwd`` writes the gradient in the logits
dtype, in place over the student logits when asked.  ``g / count`` times ``(1-alpha)`` and ``alpha`` reach it as device
scalars: no host sync.  :func:`lm_head_distill_loss` is the no-materialised-logits form, built like ops/lm_head.py
``_LMHeadCEFn``: per vocabulary chunk one student and one teacher logits GEMM into two reused buffers, then
``kd_chunk_fwd`` merging an 8-float state per row; the backward recomputes both chunks.  The GEMM-epilogue CE of
ops/lm_head.py is not extended to this loss.

``_reference`` is the plain-torch composite of the definition: the CPU path, the ``DLLM_REFERENCE_OPS=1`` path, the
``kd`` = composite arm and the tests' oracle.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import _ext
from . import routing
from .gemm import wgrad_accumulate
from .linear import _fire, _fusable, _gbuf, _use
from .lm_head import _chunk_cols, _chunks, _dh_accumulate, _logits


def check_weights(alpha: float, temperature: float) -> None:
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"distillation alpha must lie in [0, 1], got {alpha}")
    if not float(temperature) > 0.0:
        raise ValueError(f"distillation temperature must be > 0, got {temperature}")


def _reference(student_logits, teacher_logits, labels, bias, teacher_bias, smoothing, ignore_index, alpha, temperature):
    """(loss, ce, kl) of the definition in plain torch (fp32 math; fp64 logits stay fp64).  ``-inf`` logits (a banned
    token in a logits bias): a column with ``p_v = 0`` adds nothing to ``kl`` whatever ``s_v`` is (``0 * -inf`` is
    never formed, forward or backward), ``p_v > 0`` with ``s_v = -inf`` gives ``kl = +inf``, and the gradient stays
    finite."""
    up = torch.float64 if student_logits.dtype == torch.float64 else torch.float32
    s = student_logits.to(up)
    t = teacher_logits.detach().to(up)
    if bias is not None:
        s = s + bias.to(up).view(1, -1)
    if teacher_bias is not None:
        t = t + teacher_bias.detach().to(up).view(1, -1)
    valid = labels != ignore_index
    count = valid.sum().clamp_min(1).to(up)
    ce_sum = F.cross_entropy(s, labels, ignore_index=ignore_index, label_smoothing=smoothing, reduction="sum")
    logp = F.log_softmax(t / temperature, dim=-1)
    logq = F.log_softmax(s / temperature, dim=-1)
    p = logp.exp()
    kl_rows = (p * torch.where(p > 0, logp - logq, torch.zeros_like(logp))).sum(-1)
    kl_sum = torch.where(valid, kl_rows, torch.zeros_like(kl_rows)).sum()
    ce = ce_sum / count
    kl = kl_sum / count
    loss = (1.0 - alpha) * ce + (alpha * temperature * temperature) * kl
    return loss, ce.detach(), kl.detach()


def _combine(ce_rows, kl_rows, count, alpha, temperature):
    ce = ce_rows.sum() / count
    kl = kl_rows.sum() / count
    return (1.0 - alpha) * ce + (alpha * temperature * temperature) * kl, ce, kl


def _weights(g, count, alpha):
    """``(w_ce, w_kl)`` = ``((1-alpha) g / count, alpha g / count)`` as fp32 device scalars."""
    gc = g.float() / count
    return ((1.0 - alpha) * gc).reshape(1), (alpha * gc).reshape(1)


class _KDFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, teacher, labels, bias, teacher_bias, smoothing, ignore_index, alpha, temperature,
                inplace_grad):
        C = _ext.native()
        ce_rows, kl_rows, stats = C.kd_fwd(student, teacher, labels, bias, teacher_bias, float(smoothing),
                                           int(ignore_index), float(temperature))
        count = (labels != ignore_index).sum().clamp_min(1).to(torch.float32)
        ctx.save_for_backward(student, teacher, labels, bias, teacher_bias, stats, count)
        ctx.cfg = (float(smoothing), int(ignore_index), float(alpha), float(temperature), bool(inplace_grad))
        loss, ce, kl = _combine(ce_rows, kl_rows, count, alpha, temperature)
        ctx.mark_non_differentiable(ce, kl)
        return loss, ce, kl

    @staticmethod
    def backward(ctx, g, _gce, _gkl):
        C = _ext.native()
        student, teacher, labels, bias, teacher_bias, stats, count = ctx.saved_tensors
        smoothing, ignore_index, alpha, temperature, inplace = ctx.cfg
        w_ce, w_kl = _weights(g, count, alpha)
        ds = C.kd_bwd(w_ce, w_kl, student, teacher, labels, stats, bias, teacher_bias, smoothing, ignore_index,
                      temperature, inplace)
        return ds, None, None, None, None, None, None, None, None, None


def use_fused(t: torch.Tensor) -> bool:
    """The csrc/kd.hip kernels (``kd`` = fused) on a GPU tensor; else the torch composite."""
    return _ext.use_native(t) and routing.get("kd") == "fused"


def distill_loss(student_logits, teacher_logits, labels, *, bias=None, teacher_bias=None, label_smoothing: float = 0.0,
                 ignore_index: int = -100, alpha: float, temperature: float, inplace_grad: bool = False):
    """``(loss, ce, kl)``: the combined loss (a mean over rows with ``labels != ignore_index``) and its two detached
    component means (``kl`` without the ``T^2``), for logging.  logits ``[N, V]`` of one dtype, labels ``[N]``."""
    check_weights(alpha, temperature)
    if student_logits.shape != teacher_logits.shape:
        raise ValueError(f"student logits {tuple(student_logits.shape)} and teacher logits "
                         f"{tuple(teacher_logits.shape)} differ in shape (teachers with another vocabulary are not "
                         "supported)")
    if use_fused(student_logits) and student_logits.dtype in (torch.bfloat16, torch.float32):
        t = teacher_logits.detach()
        if t.dtype != student_logits.dtype:
            t = t.to(student_logits.dtype)
        return _KDFn.apply(student_logits.contiguous(), t.contiguous(), labels.contiguous(), bias,
                           None if teacher_bias is None else teacher_bias.detach(), label_smoothing, ignore_index,
                           alpha, temperature, inplace_grad)
    return _reference(student_logits, teacher_logits, labels, bias, teacher_bias, label_smoothing, ignore_index,
                      alpha, temperature)


def use_chunked(N: int, V: int) -> bool:
    """The budget rule of ops/lm_head.py ``use_chunked`` with BOTH logits tensors counted."""
    lim = float(routing.get("lmhead_full_mb"))
    if lim < 0:
        return False
    return 2 * N * V * 2 > lim * 2**20


class _LMHeadKDFn(torch.autograd.Function):
    """LM heads + distillation loss over vocabulary chunks: neither ``[N, V]`` logits tensor exists."""

    @staticmethod
    def forward(ctx, h, w, bias, th, tw, teacher_bias, labels, smoothing, ignore_index, alpha, temperature, params):
        C = _ext.native()
        N = h.shape[0]
        V = w.shape[0]
        vc = _chunk_cols(N, V)
        dev = h.device
        buf_s = torch.empty(N * min(vc + 8, V), dtype=h.dtype, device=dev)
        buf_t = torch.empty(N * min(vc + 8, V), dtype=h.dtype, device=dev)
        state = torch.empty(N, 8, dtype=torch.float32, device=dev)
        ce_rows = torch.empty(N, dtype=torch.float32, device=dev)
        kl_rows = torch.empty(N, dtype=torch.float32, device=dev)
        stats = torch.empty(N, 3, dtype=torch.float32, device=dev)
        bias32 = bias.float().contiguous() if bias is not None else None
        tbias32 = teacher_bias.float().contiguous() if teacher_bias is not None else None
        chunks = _chunks(V, vc)
        for j, (c0, n, skip) in enumerate(chunks):
            ls, lt = buf_s[:N * n].view(N, n), buf_t[:N * n].view(N, n)
            _logits(h, w[c0:c0 + n], ls)
            _logits(th, tw[c0:c0 + n], lt)
            C.kd_chunk_fwd(ls, lt, labels, bias32, tbias32, state, ce_rows, kl_rows, stats, c0, V, float(smoothing),
                           int(ignore_index), float(temperature), j == 0, j + 1 == len(chunks), skip)
        count = (labels != ignore_index).sum().clamp_min(1).to(torch.float32)
        ctx.save_for_backward(h, w, th, tw, labels, stats, count)
        ctx.bias32, ctx.tbias32 = bias32, tbias32
        ctx.cfg = (float(smoothing), int(ignore_index), float(alpha), float(temperature), vc)
        ctx.params = params
        if params is not None:
            _use(params[0])
        loss, ce, kl = _combine(ce_rows, kl_rows, count, alpha, temperature)
        ctx.mark_non_differentiable(ce, kl)
        return loss, ce, kl

    @staticmethod
    def backward(ctx, g, _gce, _gkl):
        C = _ext.native()
        h, w, th, tw, labels, stats, count = ctx.saved_tensors
        smoothing, ignore_index, alpha, temperature, vc = ctx.cfg
        N, d = h.shape
        V = w.shape[0]
        w_ce, w_kl = _weights(g, count, alpha)
        p = ctx.params[0] if ctx.params is not None else None
        gw = _gbuf(p) if p is not None else None
        dw = torch.zeros_like(w, dtype=torch.float32) if (gw is None and ctx.needs_input_grad[1]) else None
        dh = torch.zeros(N, d, dtype=torch.float32, device=h.device)
        buf_s = torch.empty(N * min(vc + 8, V), dtype=h.dtype, device=h.device)
        buf_t = torch.empty(N * min(vc + 8, V), dtype=h.dtype, device=h.device)
        for c0, n, skip in _chunks(V, vc):
            ls, lt = buf_s[:N * n].view(N, n), buf_t[:N * n].view(N, n)
            wc = w[c0:c0 + n]
            _logits(h, wc, ls)
            _logits(th, tw[c0:c0 + n], lt)
            C.kd_chunk_bwd(w_ce, w_kl, ls, lt, labels, stats, ctx.bias32, ctx.tbias32, c0, V, smoothing, ignore_index,
                           temperature, skip)  # skipped columns -> 0
            _dh_accumulate(dh, ls, wc)
            with torch.no_grad():
                if gw is not None:
                    wgrad_accumulate(gw[c0:c0 + n], ls, h, async_ok=False, defer=False)  # tied: embed bwd adds too
                elif dw is not None:
                    dw[c0:c0 + n] += torch.mm(ls.t(), h)
        if p is not None:
            _fire(p)
        return (dh.to(h.dtype), (dw.to(w.dtype) if dw is not None else None), None, None, None, None, None, None,
                None, None, None, None)


def lm_head_distill_loss(hidden, weight, teacher_hidden, teacher_weight, labels, *, scale: float | None = None,
                         bias=None, teacher_bias=None, label_smoothing: float = 0.0, ignore_index: int = -100,
                         alpha: float, temperature: float):
    """``(loss, ce, kl)`` of the distillation loss between ``(hidden * scale) @ weightᵀ (+ bias)`` and
    ``teacher_hidden @ teacher_weightᵀ (+ teacher_bias)`` without materialising either logits tensor.
    ``hidden [..., d_s]``, ``teacher_hidden [..., d_t]`` (the teacher's own scale already applied; the widths may
    differ), ``labels [...]``."""
    check_weights(alpha, temperature)
    if weight.shape[0] != teacher_weight.shape[0]:
        raise ValueError(f"student vocabulary {weight.shape[0]} and teacher vocabulary {teacher_weight.shape[0]} "
                         "differ (teachers with another vocabulary are not supported)")
    h = hidden.reshape(-1, hidden.shape[-1])
    if scale is not None:
        h = h * scale
    th = teacher_hidden.detach().reshape(-1, teacher_hidden.shape[-1])
    tw = teacher_weight.detach()
    tb = None if teacher_bias is None else teacher_bias.detach()
    lab = labels.reshape(-1)
    if not use_fused(h) or h.dtype != torch.bfloat16:  # the chunk kernels take bf16 logits; fp32: composite
        s = F.linear(h.float(), weight.float())
        t = F.linear(th.float(), tw.float())
        return _reference(s, t, lab, bias, tb, label_smoothing, ignore_index, alpha, temperature)
    params = None
    w = weight
    if torch.is_grad_enabled() and _fusable(weight) and weight.requires_grad:
        params = (weight,)
        w = weight.detach()
    return _LMHeadKDFn.apply(h.contiguous(), w, bias, th.to(h.dtype).contiguous(), tw.to(h.dtype), tb,
                             lab.contiguous(), label_smoothing, ignore_index, alpha, temperature, params)
