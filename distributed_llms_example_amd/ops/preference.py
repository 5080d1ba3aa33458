"""Preference-optimisation loss (DPO and its IPO / hinge variants) over a policy's and a frozen reference's LM-head
logits.

A call holds ``P`` pairs as ``N = 2 P T`` logit rows: sequence ``s`` owns rows ``[s T, (s+1) T)``, pair ``i`` is the
sequences ``(2i, 2i+1)`` = (chosen, rejected).  With policy logits ``x`` (+ the policy's logits bias ``b``) and the rules
of the cross-entropy kernels (a row is valid iff its label is not ``ignore_index`` and lies in ``[0, V)``)::

    lp_r = (x_y + b_y) - lse(x + b)      on a valid row, else 0
    L_s  = sum_r lp_r                    over the sequence's rows, ascending, fp32
    n_s  = max(1, #valid rows)
    h_i  = beta [(L^pi_c - L^pi_r) - (L^ref_c - L^ref_r)]
    sigmoid:  l_i = -(1 - eps) log sigmoid(h_i) - eps log sigmoid(-h_i)
    hinge:    l_i = max(0, 1 - h_i)
    ipo:      l_i = (hbar_i - 1 / (2 beta))^2,   hbar_i = h_i / beta with every L_s replaced by L_s / n_s
    sft term: l_i += sft_alpha (-L^pi_c / n_c)
    loss = sum_i l_i / P_step

(Rafailov et al. 2023; Azar et al. 2023 for IPO; the hinge form of SLiC.)  ``P_step`` is the number of pairs the loss is
normalised by: the call's own ``P``, or with ``inv_pairs`` (a device scalar ``1 / P_step``) the pairs of the whole
optimizer step.  Every gradient is ``dx_v = c_r (softmax(x + b)_v - [v == y])`` with ``c_r = -G dloss/dL_s``; the
reference gets none.

GPU path (csrc/pref.hip, ops/routing.py ``pref`` = fused): ``pref_fwd`` makes ONE pass over both ``[N, V]`` tensors and
keeps ``lp_pi``, ``lp_ref``, ``lse_pi``; ``pref_pairs`` (one small launch) forms the sums, the pair losses, the logged
statistics and the row coefficients from device scalars (no host sync); ``pref_bwd`` writes the gradient in the logits
dtype, in place over the policy logits when asked.  :func:`lm_head_preference_loss` is the no-materialised-logits form,
built like ops/distill.py ``_LMHeadKDFn``: per vocabulary chunk one policy and one reference GEMM into two reused
buffers, then ``pref_chunk_fwd`` merging a 6-float state per row; the backward recomputes the policy chunk only.

``_reference`` is the plain-torch composite of the definition: the CPU path, the ``DLLM_REFERENCE_OPS=1`` path, the
``pref`` = composite arm and the tests' oracle.  ``stats`` (detached, means over the call's pairs) carries TRL's names:
``rewards/chosen``, ``rewards/rejected``, ``rewards/margins``, ``rewards/accuracies``, ``logps/chosen``,
``logps/rejected``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import _ext
from . import routing
from .gemm import wgrad_accumulate
from .linear import _fire, _fusable, _gbuf, _use
from .lm_head import _chunk_cols, _chunks, _dh_accumulate, _logits

KINDS = ("sigmoid", "hinge", "ipo")  # the order is csrc/pref.hip's `kind`
STAT_NAMES = ("rewards/chosen", "rewards/rejected", "rewards/margins", "rewards/accuracies", "logps/chosen",
              "logps/rejected")


def check_config(beta: float, kind: str = "sigmoid", label_smoothing: float = 0.0) -> None:
    if not float(beta) > 0.0:
        raise ValueError(f"preference beta (--dpo-beta) must be > 0, got {beta}")
    if kind not in KINDS:
        raise ValueError(f"preference loss kind (--dpo-loss) must be one of {', '.join(KINDS)}, got {kind!r}")
    if not 0.0 <= float(label_smoothing) < 0.5:
        raise ValueError(f"preference label smoothing (--dpo-label-smoothing) must lie in [0, 0.5), got "
                         f"{label_smoothing}")


def check_rows(N: int, T: int) -> int:
    """The number of pairs ``P`` of ``N = 2 P T`` rows."""
    if T <= 0 or N <= 0 or N % (2 * T) != 0:
        raise ValueError(f"preference loss: {N} logit rows are not 2 P T interleaved (chosen, rejected) sequences of "
                         f"T = {T} rows")
    return N // (2 * T)


def row_logps(logits, labels, bias, ignore_index):
    """(lp [N], valid [N]) of the definition in plain torch (fp32 math; fp64 logits stay fp64)."""
    up = torch.float64 if logits.dtype == torch.float64 else torch.float32
    x = logits.to(up)
    if bias is not None:
        x = x + bias.to(up).view(1, -1)
    V = x.shape[-1]
    valid = (labels != ignore_index) & (labels >= 0) & (labels < V)
    xy = x.gather(1, labels.clamp(0, V - 1).view(-1, 1)).view(-1)
    lp = xy - torch.logsumexp(x, dim=-1)
    return torch.where(valid, lp, torch.zeros_like(lp)), valid


def pair_loss(lp_pi, lp_ref, valid, T, beta, kind, label_smoothing, sft_alpha, inv_pairs=None):
    """(loss, stats) from the per-row log-probabilities, in plain torch: steps two and three of the definition."""
    up = lp_pi.dtype
    P = check_rows(lp_pi.numel(), T)
    Lp = lp_pi.view(2 * P, T).sum(-1).view(P, 2)
    Lr = lp_ref.view(2 * P, T).sum(-1).view(P, 2)
    n = valid.view(2 * P, T).sum(-1).clamp_min(1).to(up).view(P, 2)
    h = beta * ((Lp[:, 0] - Lp[:, 1]) - (Lr[:, 0] - Lr[:, 1]))
    if kind == "sigmoid":
        l = -(1.0 - label_smoothing) * F.logsigmoid(h) - label_smoothing * F.logsigmoid(-h)
    elif kind == "hinge":
        l = torch.relu(1.0 - h)
    else:
        hb = (Lp[:, 0] / n[:, 0] - Lp[:, 1] / n[:, 1]) - (Lr[:, 0] / n[:, 0] - Lr[:, 1] / n[:, 1])
        l = (hb - 1.0 / (2.0 * beta)) ** 2
    if sft_alpha != 0.0:
        l = l - sft_alpha * Lp[:, 0] / n[:, 0]
    loss = l.sum() * (inv_pairs.to(up).reshape(()) if inv_pairs is not None else 1.0 / P)
    with torch.no_grad():
        rc, rr = beta * (Lp[:, 0] - Lr[:, 0]), beta * (Lp[:, 1] - Lr[:, 1])
        stats = {"rewards/chosen": rc.mean(), "rewards/rejected": rr.mean(), "rewards/margins": (rc - rr).mean(),
                 "rewards/accuracies": (rc > rr).to(up).mean(), "logps/chosen": Lp[:, 0].mean(),
                 "logps/rejected": Lp[:, 1].mean()}
    return loss, stats


def _reference(policy_logits, ref_logits, labels, T, bias, ref_bias, beta, kind, label_smoothing, sft_alpha,
               ignore_index=-100, inv_pairs=None):
    """(loss, stats) of the definition in plain torch.  ``ref_logits`` None: the reference log-probabilities are 0."""
    lp_pi, valid = row_logps(policy_logits, labels, bias, ignore_index)
    if ref_logits is not None:
        with torch.no_grad():
            lp_ref, _ = row_logps(ref_logits.detach(), labels, None if ref_bias is None else ref_bias.detach(),
                                  ignore_index)
        lp_ref = lp_ref.to(lp_pi.dtype)
    else:
        lp_ref = torch.zeros_like(lp_pi)
    return pair_loss(lp_pi, lp_ref, valid, T, beta, kind, label_smoothing, sft_alpha, inv_pairs)


def _stats(out):
    return {name: out[k + 1] for k, name in enumerate(STAT_NAMES)}


def _inv_pairs(inv_pairs, P, device):
    if inv_pairs is None:
        return torch.full((1,), 1.0 / P, dtype=torch.float32, device=device)
    return inv_pairs.detach().to(torch.float32).reshape(1)


class _PrefFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, policy, ref, labels, bias, ref_bias, inv_pairs, T, ignore_index, beta, kind, smoothing, sft_alpha,
                inplace_grad):
        C = _ext.native()
        V = policy.shape[1]
        lp_pi, lp_ref, lse = C.pref_fwd(policy, ref, labels, bias, ref_bias, int(ignore_index))
        cfg = (int(T), int(V), int(ignore_index), float(beta), KINDS.index(kind), float(smoothing), float(sft_alpha))
        out, _, _ = C.pref_pairs(lp_pi, lp_ref, labels, None, inv_pairs, *cfg)
        ctx.save_for_backward(policy, labels, bias, lse, lp_pi, lp_ref, inv_pairs)
        ctx.cfg, ctx.inplace = cfg, bool(inplace_grad)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, g, _gout):
        C = _ext.native()
        policy, labels, bias, lse, lp_pi, lp_ref, inv_pairs = ctx.saved_tensors
        _, _, coef = C.pref_pairs(lp_pi, lp_ref, labels, g.float().reshape(1), inv_pairs, *ctx.cfg)
        dx = C.pref_bwd(coef, policy, labels, lse, bias, ctx.inplace)
        return (dx,) + (None,) * 12


def use_fused(t: torch.Tensor) -> bool:
    """The csrc/pref.hip kernels (``pref`` = fused) on a GPU tensor; else the torch composite."""
    return _ext.use_native(t) and routing.get("pref") == "fused"


def preference_loss(policy_logits, ref_logits, labels, T: int, *, bias=None, ref_bias=None, beta: float,
                    kind: str = "sigmoid", label_smoothing: float = 0.0, sft_alpha: float = 0.0,
                    inplace_grad: bool = False, ignore_index: int = -100, inv_pairs=None):
    """``(loss, stats)``: the preference loss of ``P = N / (2 T)`` interleaved (chosen, rejected) pairs and the six
    detached statistics (a dict of scalars, means over the call's pairs).  logits ``[N, V]`` of one dtype
    (``ref_logits`` None: the policy alone, reference log-probabilities 0), labels ``[N]``.  ``inv_pairs``: a device
    scalar ``1 / P_step`` when the loss is normalised by more pairs than the call holds (default ``1 / P``)."""
    check_config(beta, kind, label_smoothing)
    N = policy_logits.shape[0]
    P = check_rows(N, int(T))
    if labels.numel() != N:
        raise ValueError(f"preference loss: {labels.numel()} labels for {N} logit rows")
    if ref_logits is not None and ref_logits.shape != policy_logits.shape:
        raise ValueError(f"policy logits {tuple(policy_logits.shape)} and reference logits {tuple(ref_logits.shape)} "
                         "differ in shape (a reference with another vocabulary is not supported)")
    if use_fused(policy_logits) and policy_logits.dtype in (torch.bfloat16, torch.float32):
        r = None
        if ref_logits is not None:
            r = ref_logits.detach()
            r = (r if r.dtype == policy_logits.dtype else r.to(policy_logits.dtype)).contiguous()
        loss, out = _PrefFn.apply(policy_logits.contiguous(), r, labels.reshape(-1).contiguous(), bias,
                                  None if ref_bias is None else ref_bias.detach(),
                                  _inv_pairs(inv_pairs, P, policy_logits.device), int(T), ignore_index, beta, kind,
                                  label_smoothing, sft_alpha, inplace_grad)
        return loss, _stats(out)
    return _reference(policy_logits, ref_logits, labels.reshape(-1), int(T), bias, ref_bias, beta, kind,
                      label_smoothing, sft_alpha, ignore_index, inv_pairs)


def use_chunked(N: int, V: int) -> bool:
    """The budget rule of ops/lm_head.py ``use_chunked`` with BOTH logits tensors counted."""
    lim = float(routing.get("lmhead_full_mb"))
    if lim < 0:
        return False
    return 2 * N * V * 2 > lim * 2**20


class _LMHeadPrefFn(torch.autograd.Function):
    """LM heads + preference loss over vocabulary chunks: neither ``[N, V]`` logits tensor exists."""

    @staticmethod
    def forward(ctx, h, w, bias, rh, rw, ref_bias, labels, inv_pairs, T, ignore_index, beta, kind, smoothing,
                sft_alpha, params, vc):
        C = _ext.native()
        N = h.shape[0]
        V = w.shape[0]
        vc = int(vc) if vc else _chunk_cols(N, V)
        dev = h.device
        buf_p = torch.empty(N * min(vc + 8, V), dtype=h.dtype, device=dev)
        buf_r = torch.empty(N * min(vc + 8, V), dtype=h.dtype, device=dev)
        state = torch.empty(N, 6, dtype=torch.float32, device=dev)
        lp_pi, lp_ref, lse = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(3))
        bias32 = bias.float().contiguous() if bias is not None else None
        rbias32 = ref_bias.float().contiguous() if ref_bias is not None else None
        chunks = _chunks(V, vc)
        for j, (c0, n, skip) in enumerate(chunks):
            lp, lr = buf_p[:N * n].view(N, n), buf_r[:N * n].view(N, n)
            _logits(h, w[c0:c0 + n], lp)
            _logits(rh, rw[c0:c0 + n], lr)
            C.pref_chunk_fwd(lp, lr, labels, bias32, rbias32, state, lp_pi, lp_ref, lse, c0, V, int(ignore_index),
                             j == 0, j + 1 == len(chunks), skip)
        cfg = (int(T), int(V), int(ignore_index), float(beta), KINDS.index(kind), float(smoothing), float(sft_alpha))
        out, _, _ = C.pref_pairs(lp_pi, lp_ref, labels, None, inv_pairs, *cfg)
        ctx.save_for_backward(h, w, labels, lse, lp_pi, lp_ref, inv_pairs)
        ctx.bias32, ctx.cfg, ctx.vc, ctx.params = bias32, cfg, vc, params
        if params is not None:
            _use(params[0])
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, g, _gout):
        C = _ext.native()
        h, w, labels, lse, lp_pi, lp_ref, inv_pairs = ctx.saved_tensors
        N, d = h.shape
        V = w.shape[0]
        vc = ctx.vc
        _, _, coef = C.pref_pairs(lp_pi, lp_ref, labels, g.float().reshape(1), inv_pairs, *ctx.cfg)
        p = ctx.params[0] if ctx.params is not None else None
        gw = _gbuf(p) if p is not None else None
        dw = torch.zeros_like(w, dtype=torch.float32) if (gw is None and ctx.needs_input_grad[1]) else None
        dh = torch.zeros(N, d, dtype=torch.float32, device=h.device)
        buf_p = torch.empty(N * min(vc + 8, V), dtype=h.dtype, device=h.device)
        for c0, n, skip in _chunks(V, vc):
            lp = buf_p[:N * n].view(N, n)
            wc = w[c0:c0 + n]
            _logits(h, wc, lp)  # the policy chunk only: the reference gets no gradient
            C.pref_chunk_bwd(coef, lp, labels, lse, ctx.bias32, c0, V, skip)  # skipped columns -> 0
            _dh_accumulate(dh, lp, wc)
            with torch.no_grad():
                if gw is not None:
                    wgrad_accumulate(gw[c0:c0 + n], lp, h, async_ok=False, defer=False)  # tied: embed bwd adds too
                elif dw is not None:
                    dw[c0:c0 + n] += torch.mm(lp.t(), h)
        if p is not None:
            _fire(p)
        return (dh.to(h.dtype), (dw.to(w.dtype) if dw is not None else None)) + (None,) * 14


def lm_head_preference_loss(hidden, weight, ref_hidden, ref_weight, labels, T: int, *, scale: float | None = None,
                            bias=None, ref_bias=None, beta: float, kind: str = "sigmoid",
                            label_smoothing: float = 0.0, sft_alpha: float = 0.0, ignore_index: int = -100,
                            inv_pairs=None, chunk_cols: int | None = None):
    """``(loss, stats)`` of the preference loss between ``(hidden * scale) @ weightᵀ (+ bias)`` and ``ref_hidden @
    ref_weightᵀ (+ ref_bias)`` without materialising either logits tensor.  ``hidden [..., d]``, ``ref_hidden
    [..., d_ref]`` (the reference's own scale already applied; the widths may differ), ``labels [...]`` with
    ``labels.numel() = 2 P T``.  ``chunk_cols``: the vocabulary columns per chunk (default: ops/lm_head.py's budget)."""
    check_config(beta, kind, label_smoothing)
    if weight.shape[0] != ref_weight.shape[0]:
        raise ValueError(f"policy vocabulary {weight.shape[0]} and reference vocabulary {ref_weight.shape[0]} differ "
                         "(a reference with another vocabulary is not supported)")
    h = hidden.reshape(-1, hidden.shape[-1])
    P = check_rows(h.shape[0], int(T))
    if scale is not None:
        h = h * scale
    rh = ref_hidden.detach().reshape(-1, ref_hidden.shape[-1])
    rw = ref_weight.detach()
    rb = None if ref_bias is None else ref_bias.detach()
    lab = labels.reshape(-1)
    if not use_fused(h) or h.dtype != torch.bfloat16:  # the chunk kernels take bf16 logits; fp32: composite
        s = F.linear(h.float(), weight.float())
        t = F.linear(rh.float(), rw.float())
        return _reference(s, t, lab, int(T), bias, rb, beta, kind, label_smoothing, sft_alpha, ignore_index, inv_pairs)
    params = None
    w = weight
    if torch.is_grad_enabled() and _fusable(weight) and weight.requires_grad:
        params = (weight,)
        w = weight.detach()
    loss, out = _LMHeadPrefFn.apply(h.contiguous(), w, bias, rh.to(h.dtype).contiguous(), rw.to(h.dtype), rb,
                                    lab.contiguous(), _inv_pairs(inv_pairs, P, h.device), int(T), ignore_index, beta,
                                    kind, label_smoothing, sft_alpha, params, chunk_cols)
    return loss, _stats(out)
