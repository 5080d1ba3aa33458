"""Knowledge distillation at the model level: the teacher's LM-head operands a student's ``forward`` takes
(``distill=``), the loss routing both families share, and :func:`make_student` (a shallower copy of the teacher).

The loss is ops/distill.py's: label-smoothed CE on the labels plus temperature-scaled KL to the teacher's distribution.
The teacher runs outside the student (train/engine.py: frozen, ``eval()``, under ``no_grad``) and hands over its
decoder hidden states and output embedding — its logits are formed next to the student's, or never (vocabulary chunks).
"""
from __future__ import annotations

import re
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from ..ops import distill as kd_ops
from ..ops.linear import linear
from .output import Seq2SeqLMOutput


@dataclass
class Distill:
    """What a student's ``forward(distill=...)`` needs of the teacher: decoder hidden states ``[B, T, d_t]`` with the
    teacher's own output scale applied, its output embedding ``[V, d_t]``, its logits bias (or None), and the loss
    weights."""
    teacher_hidden: torch.Tensor
    teacher_weight: torch.Tensor
    teacher_bias: torch.Tensor | None = None
    alpha: float = 0.5
    temperature: float = 2.0


def lm_output(dec, weight, labels, distill: Distill, *, enc, scale=None, bias=None, label_smoothing: float = 0.0,
              return_logits: bool = False) -> Seq2SeqLMOutput:
    """The LM head + distillation loss of a student's forward: vocabulary chunks when both logits tensors together
    exceed the full-logits budget (ops/distill.py use_chunked), else full logits with the gradient written in place
    over the student's.  ``return_logits`` keeps the student logits: full-logits path, out of place."""
    if labels is None:
        raise ValueError("distill= needs labels")
    V = weight.shape[0]
    if distill.teacher_weight.shape[0] != V:
        raise ValueError(f"teacher vocabulary {distill.teacher_weight.shape[0]} and student vocabulary {V} differ "
                         "(teachers with another vocabulary are not supported)")
    kw = dict(bias=bias, teacher_bias=distill.teacher_bias, label_smoothing=label_smoothing, alpha=distill.alpha,
              temperature=distill.temperature)
    if not return_logits and kd_ops.use_chunked(labels.numel(), V):
        loss, ce, kl = kd_ops.lm_head_distill_loss(dec, weight, distill.teacher_hidden, distill.teacher_weight, labels,
                                                   scale=scale, **kw)
        return Seq2SeqLMOutput(loss=loss, logits=None, encoder_last_hidden_state=enc, ce_loss=ce, kd_loss=kl)
    raw = linear(dec * scale if scale is not None else dec, weight)
    with torch.no_grad():
        t = F.linear(distill.teacher_hidden.to(raw.dtype), distill.teacher_weight.to(raw.dtype))
    loss, ce, kl = kd_ops.distill_loss(raw.view(-1, V), t.view(-1, V), labels.reshape(-1),
                                       inplace_grad=not return_logits, **kw)
    logits = None
    if return_logits:
        logits = raw + bias.to(raw.dtype) if bias is not None else raw
    return Seq2SeqLMOutput(loss=loss, logits=logits, encoder_last_hidden_state=enc, ce_loss=ce, kd_loss=kl)


# --------------------------------------------------------------------------------------------------------- student
def layer_picks(total: int, keep: int) -> list[int]:
    """The teacher layers a ``keep``-layer student copies out of ``total``: student layer ``i`` takes teacher layer
    ``floor(i (L-1) / (k-1) + 0.5)`` (``k = 1``: layer 0).  Layer 0 is always kept — T5's relative-bias table lives
    there.  12 -> 6: [0, 2, 4, 7, 9, 11]; 12 -> 3: [0, 6, 11]."""
    if not 1 <= keep <= total:
        raise ValueError(f"a student keeps 1 .. {total} of the teacher's {total} layers, got {keep}")
    if keep == 1:
        return [0]
    # integer form of floor(i (L-1) / (k-1) + 1/2)
    return [(2 * i * (total - 1) + (keep - 1)) // (2 * (keep - 1)) for i in range(keep)]


def student_config(cfg, encoder_layers: int, decoder_layers: int):
    """The teacher's config with the student's layer counts; per-layer lists follow :func:`layer_picks`."""
    enc = layer_picks(cfg.num_layers, int(encoder_layers))
    kw = dict(num_layers=len(enc), num_decoder_layers=len(layer_picks(cfg.num_decoder_layers, int(decoder_layers))))
    if isinstance(cfg.attention_window, (list, tuple)):
        kw["attention_window"] = [cfg.attention_window[i] for i in enc]
    return cfg.replace(**kw)


_LAYER_KEY = re.compile(r"^(.*\b(encoder|decoder)\.(?:block|layers)\.)(\d+)(\..*)$")


def make_student(teacher, encoder_layers: int, decoder_layers: int):
    """A student with the teacher's config but ``encoder_layers`` / ``decoder_layers`` layers, initialised from the
    teacher: the picked layers (:func:`layer_picks`), embeddings, final norms, LM head and ``final_logits_bias`` are
    copied; per-layer config lists (LED's ``attention_window``) follow the same picks."""
    from .hf_io import build_model
    cfg = teacher.config
    picks = {"encoder": layer_picks(cfg.num_layers, int(encoder_layers)),
             "decoder": layer_picks(cfg.num_decoder_layers, int(decoder_layers))}
    p0 = next(teacher.parameters())
    student = build_model(student_config(cfg, encoder_layers, decoder_layers), dtype=p0.dtype, device=p0.device)
    src = teacher.state_dict()
    out = {}
    for k in student.state_dict():
        m = _LAYER_KEY.match(k)
        out[k] = src[f"{m.group(1)}{picks[m.group(2)][int(m.group(3))]}{m.group(4)}" if m else k]
    student.load_state_dict(out, strict=True)
    return student
