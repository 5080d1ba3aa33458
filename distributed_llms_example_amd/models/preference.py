"""Preference optimisation (DPO and its IPO / hinge variants) at the model level: the frozen reference policy's LM-head
operands a policy's ``forward`` takes (``preference=``) and the loss routing both families share.

A batch holds ``P`` prompts (``input_ids [P, S]``: the encoder runs once per prompt) and ``2P`` interleaved target rows
(``labels [2P, T]``: row ``2i`` the chosen, row ``2i + 1`` the rejected target of prompt ``i``).  The decoder runs on
the ``2P`` rows; its cross-attention reads each prompt's K/V once (the ``kv.shape[0] != B`` path beam search uses).  The
reference runs outside the policy (train/engine.py: frozen, ``eval()``, under ``no_grad``) and hands over its decoder
hidden states and output embedding — its logits are formed next to the policy's, or never (vocabulary chunks).  The
loss is ops/preference.py's.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn.functional as F

from ..ops import preference as pref_ops
from ..ops.linear import linear
from .output import Seq2SeqLMOutput


@dataclass
class Preference:
    """What a policy's ``forward(preference=...)`` needs of the reference: decoder hidden states ``[2P, T, d_ref]`` with
    the reference's own output scale applied, its output embedding ``[V, d_ref]``, its logits bias (or None), and the
    loss settings.  ``inv_pairs``: a device scalar ``1 / P_step`` (None: the batch's own pairs)."""
    ref_hidden: torch.Tensor
    ref_weight: torch.Tensor
    ref_bias: torch.Tensor | None = None
    beta: float = 0.1
    kind: str = "sigmoid"
    label_smoothing: float = 0.0
    sft_alpha: float = 0.0
    inv_pairs: torch.Tensor | None = None


def check_batch(input_ids, labels) -> None:
    """``labels [2P, T]`` against ``input_ids [P, S]`` (or an encoder output ``[P, S, d]``): one encoder row per
    prompt.  ``[2P, S]`` inputs (the prompt repeated per target row) are taken too."""
    if labels is None or labels.dim() != 2 or labels.shape[0] % 2:
        raise ValueError("preference= needs labels [2P, T]: interleaved (chosen, rejected) target rows")
    if input_ids is not None and labels.shape[0] not in (2 * input_ids.shape[0], input_ids.shape[0]):
        raise ValueError(f"preference= needs two target rows (chosen, rejected) per prompt: got {labels.shape[0]} "
                         f"label rows for {input_ids.shape[0]} prompts")


def lm_output(dec, weight, labels, pref: Preference, *, enc, scale=None, bias=None,
              return_logits: bool = False) -> Seq2SeqLMOutput:
    """The LM head + preference loss of a policy's forward: vocabulary chunks when both logits tensors together exceed
    the full-logits budget (ops/preference.py use_chunked), else full logits with the gradient written in place over
    the policy's.  ``return_logits`` keeps the policy logits: full-logits path, out of place."""
    check_batch(None, labels)
    V = weight.shape[0]
    if pref.ref_weight.shape[0] != V:
        raise ValueError(f"reference vocabulary {pref.ref_weight.shape[0]} and policy vocabulary {V} differ (a "
                         "reference with another vocabulary is not supported)")
    T = labels.shape[-1]
    kw = dict(bias=bias, ref_bias=pref.ref_bias, beta=pref.beta, kind=pref.kind, label_smoothing=pref.label_smoothing,
              sft_alpha=pref.sft_alpha, inv_pairs=pref.inv_pairs)
    if not return_logits and pref_ops.use_chunked(labels.numel(), V):
        loss, stats = pref_ops.lm_head_preference_loss(dec, weight, pref.ref_hidden, pref.ref_weight, labels, T,
                                                       scale=scale, **kw)
        return Seq2SeqLMOutput(loss=loss, logits=None, encoder_last_hidden_state=enc, pref_stats=stats)
    raw = linear(dec * scale if scale is not None else dec, weight)
    with torch.no_grad():
        r = F.linear(pref.ref_hidden.to(raw.dtype), pref.ref_weight.to(raw.dtype))
    loss, stats = pref_ops.preference_loss(raw.view(-1, V), r.view(-1, V), labels.reshape(-1), T,
                                           inplace_grad=not return_logits, **kw)
    logits = None
    if return_logits:
        logits = raw + bias.to(raw.dtype) if bias is not None else raw
    return Seq2SeqLMOutput(loss=loss, logits=logits, encoder_last_hidden_state=enc, pref_stats=stats)
