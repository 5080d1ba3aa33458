"""LoRA fine-tuning: freeze the base model and train low-rank adapters on its projections (ops/lora.py).

    cfg = LoraConfig(r=8, alpha=16, dropout=0.05, targets=("q", "v"))
    apply_lora(model, cfg)            # before TrainEngine / FlatParams: they then hold the adapters only
    ...train...
    save_adapter(model, out_dir)      # models/hf_io.py: PEFT's adapter_config.json + adapter_model.safetensors
    merge_lora(model)                 # W += scale · B A; a plain model again, save_pretrained writes an HF checkpoint

``targets`` are logical names — ``q``, ``k``, ``v``, ``o`` (self- and cross-attention alike), ``wi``, ``wo`` (BART's
``fc1`` / ``fc2``) — because the projections are fused here: ``qkv`` / ``qkv_proj`` = q|k|v, ``kv`` / ``kv_proj`` = k|v,
a gated ``wi`` = gate|up.  An adapter therefore lives on an output column slice of the fused weight: ``q`` and ``v``
on a fused ``qkv`` are two adapters on one layer (slices 0 and 2), ``wi`` on a gated FFN adapts both halves.
Embeddings, the LM head, norms and LED's ``q_global`` / ``kv_global`` are never adapted.  Init as PEFT: ``lora_A``
Kaiming-uniform (a = √5), ``lora_B`` zeros, so the adapted model starts as the base model.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn as nn

from ..ops.linear import Linear
from ..ops.lora import Adapter

TARGETS = ("q", "k", "v", "o", "wi", "wo")

# attribute name of a projection -> the logical target of each of its equal output slices
_SLICES = {
    "qkv": ("q", "k", "v"), "qkv_proj": ("q", "k", "v"), "kv": ("k", "v"), "kv_proj": ("k", "v"),
    "q": ("q",), "q_proj": ("q",), "o": ("o",), "out_proj": ("o",),
    "wi": ("wi",), "fc1": ("wi",), "wo": ("wo",), "fc2": ("wo",),
}


@dataclass(frozen=True)
class LoraConfig:
    r: int = 8
    alpha: float = 16
    dropout: float = 0.0
    targets: tuple = ("q", "v")

    def __post_init__(self):
        object.__setattr__(self, "targets", tuple(self.targets))
        unknown = [t for t in self.targets if t not in TARGETS]
        if unknown:
            raise ValueError(f"unknown LoRA targets {unknown}; known: {', '.join(TARGETS)}")
        if not 1 <= int(self.r) <= 64:
            raise ValueError(f"LoRA rank must be 1 .. 64, got {self.r}")
        if not 0.0 <= float(self.dropout) < 1.0:
            raise ValueError(f"LoRA dropout must be in [0, 1), got {self.dropout}")

    @property
    def scale(self) -> float:
        return float(self.alpha) / int(self.r)


def _layer_slices(model, name: str, mod: Linear):
    """The logical target of each output slice of the projection ``name``, or None when it is never adapted."""
    leaf = name.rsplit(".", 1)[-1]
    if leaf not in _SLICES or name == "lm_head":
        return None
    names = _SLICES[leaf]
    cfg = model.config
    if leaf == "wi" and cfg.model_type == "t5" and cfg.is_gated:
        names = ("wi", "wi")
    return names


def adapted_layers(model):
    """[(module name, Linear)] of the layers that carry adapters."""
    return [(n, m) for n, m in model.named_modules() if isinstance(m, Linear) and m._lora is not None]


def has_lora(model) -> bool:
    return getattr(model, "_lora_cfg", None) is not None


def apply_lora(model: nn.Module, cfg: LoraConfig) -> nn.Module:
    """Freeze every parameter of ``model`` and attach trainable adapters to the projections ``cfg.targets`` names.
    Call it before ``TrainEngine`` / ``FlatParams`` are built (they collect the trainable parameters)."""
    if getattr(getattr(model, "config", None), "model_type", None) == "t5gemma":
        raise NotImplementedError("T5Gemma: LoRA (--lora-r) is not implemented: its fused qkv projection has unequal "
                                  "q and k / v parts with grouped K/V heads")
    if has_lora(model):
        raise RuntimeError("apply_lora: the model already carries adapters (merge_lora removes them)")
    if any(getattr(p, "_dllm_fused_wgrad", False) for p in model.parameters()):
        raise RuntimeError("apply_lora must be called before TrainEngine / FlatParams are built: they already hold "
                           "this model's parameters")
    model._lora_trainable = [n for n, p in model.named_parameters() if p.requires_grad]
    for p in model.parameters():
        p.requires_grad_(False)
    r = int(cfg.r)
    count = 0
    for name, mod in list(model.named_modules()):
        if not isinstance(mod, Linear):
            continue
        names = _layer_slices(model, name, mod)
        if names is None or not any(t in cfg.targets for t in names):
            continue
        n = mod.out_features // len(names)
        adapters = []
        for i, target in enumerate(names):
            if target not in cfg.targets:
                continue
            A = nn.Parameter(torch.empty(r, mod.in_features, dtype=mod.weight.dtype, device=mod.weight.device))
            B = nn.Parameter(torch.zeros(n, r, dtype=mod.weight.dtype, device=mod.weight.device))
            nn.init.kaiming_uniform_(A, a=math.sqrt(5))
            mod.register_parameter(f"lora_A_{i}", A)
            mod.register_parameter(f"lora_B_{i}", B)
            adapters.append(Adapter(target, i * n, n, A, B, cfg.scale))
            count += 1
        mod._lora = (adapters, float(cfg.dropout))
    if count == 0:
        raise ValueError(f"apply_lora: no projection of this model matches the targets {cfg.targets}")
    model._lora_cfg = cfg
    return model


def adapter_slice_index(ad: Adapter) -> int:
    return ad.c0 // ad.n


@torch.no_grad()
def merge_lora(model: nn.Module) -> nn.Module:
    """Fold every adapter into its base weight — ``W[c0:c0+n] += scale · B A``, computed in fp32 and rounded once —
    and remove the adapters: a plain model (parameters trainable as before ``apply_lora``)."""
    if not has_lora(model):
        raise RuntimeError("merge_lora: the model carries no adapters")
    for _, mod in adapted_layers(model):
        adapters, _ = mod._lora
        for ad in adapters:
            rows = mod.weight[ad.c0:ad.c0 + ad.n]
            rows.copy_((rows.float() + ad.scale * (ad.B.float() @ ad.A.float())).to(rows.dtype))
            i = adapter_slice_index(ad)
            delattr(mod, f"lora_A_{i}")
            delattr(mod, f"lora_B_{i}")
        del mod._lora  # back to the class default: no adapters
    trainable = set(model._lora_trainable)
    for n, p in model.named_parameters():
        p.requires_grad_(n in trainable)
    del model._lora_cfg, model._lora_trainable
    return model


def param_counts(model) -> tuple[int, int]:
    """(trainable, total) parameter counts (tied parameters once)."""
    seen, train, total = set(), 0, 0
    for p in model.parameters():
        if id(p) in seen:
            continue
        seen.add(id(p))
        total += p.numel()
        train += p.numel() if p.requires_grad else 0
    return train, total
