"""Model output container (the fields of transformers' Seq2SeqLMOutput the runtime uses)."""
from __future__ import annotations

from dataclasses import dataclass

import torch


@dataclass
class Seq2SeqLMOutput:
    loss: torch.Tensor | None = None
    logits: torch.Tensor | None = None
    encoder_last_hidden_state: torch.Tensor | None = None
    # distillation (forward(distill=...), models/distill.py): the detached CE and KL means of the combined loss
    ce_loss: torch.Tensor | None = None
    kd_loss: torch.Tensor | None = None
    # preference optimisation (forward(preference=...), models/preference.py): the six detached statistics
    pref_stats: dict | None = None

    def __getitem__(self, i):
        return (self.loss, self.logits)[i]
