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

``LoraConfig(quantize="nf4")`` (QLoRA): after freezing, every projection with one of the names above — adapted or not
— whose sides are multiples of 64 is held as NF4 codes (ops/nf4.py): ``weight`` None, buffers ``weight_nf4`` /
``weight_absmax``.  ``merge_lora`` dequantises them again; docs/MODELS.md has the rest.

``LoraConfig(dora=True)`` (DoRA): every adapter also carries a trainable magnitude ``lora_m_{i}`` [n], initialised to
the row norms of its weight slice, and the slice's output is ``m / ‖W_s + s B A‖ ⊙ (x W_sᵀ + s t Bᵀ) + b_s``
(ops/lora.py).  Not together with ``quantize``.
"""
from __future__ import annotations

import logging
import math
from dataclasses import dataclass

import torch
import torch.nn as nn

from ..ops import nf4
from ..ops.linear import Linear
from ..ops.lora import Adapter, dora_norm

_log = logging.getLogger(__name__)

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
    quantize: str | None = None  # "nf4": QLoRA, the frozen projections held as 4-bit codes (ops/nf4.py)
    dora: bool = False           # weight-decomposed adapters: a trainable magnitude per output row (ops/lora.py)

    def __post_init__(self):
        object.__setattr__(self, "targets", tuple(self.targets))
        object.__setattr__(self, "dora", bool(self.dora))
        if self.dora and self.quantize is not None:
            raise NotImplementedError(f"dora=True with quantize={self.quantize!r} is not implemented: the row norms "
                                      "would need the dequantised weight every step")
        if self.quantize not in (None, "nf4"):
            raise ValueError(f"unknown LoRA base quantisation {self.quantize!r}; known: nf4")
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
            m = None
            if cfg.dora:  # B = 0: the norm of the weight rows themselves, so c = 1 at the start
                with torch.no_grad():
                    m = nn.Parameter(dora_norm(mod.weight[i * n:(i + 1) * n], A, B, cfg.scale).to(mod.weight.dtype))
                mod.register_parameter(f"lora_m_{i}", m)
            adapters.append(Adapter(target, i * n, n, A, B, cfg.scale, m))
            count += 1
        mod._lora = (adapters, float(cfg.dropout))
    if count == 0:
        raise ValueError(f"apply_lora: no projection of this model matches the targets {cfg.targets}")
    model._lora_cfg = cfg
    if cfg.quantize == "nf4":
        before = frozen_bytes(model)
        skipped = quantize_base(model)
        model._nf4_report = {"frozen_bytes_before": before, "frozen_bytes": frozen_bytes(model),
                             "nf4_skipped": skipped}
        _log.info("nf4: frozen bytes %d -> %d; not a multiple of 64 on both sides, kept as they are: %s", before,
                  model._nf4_report["frozen_bytes"], ", ".join(skipped) or "none")
    return model


def quantized_layers(model):
    """[(module name, Linear)] of the layers whose frozen weight is held as NF4 codes."""
    return [(n, m) for n, m in model.named_modules() if isinstance(m, Linear) and m._nf4 is not None]


@torch.no_grad()
def quantize_base(model) -> list[str]:
    """Quantise the frozen weight of every projection whose leaf name is in ``_SLICES`` (attention projections and FFN
    layers, cross-attention K/V included; adapted or not) to NF4: ``weight`` becomes None, the buffers ``weight_nf4``
    / ``weight_absmax`` hold it.  Never the LM head, embeddings, norms, bias tables or LED's ``q_global`` /
    ``kv_global``.  Returns the names of the layers left as they are because a side is no multiple of 64."""
    skipped = []
    for name, mod in list(model.named_modules()):
        if not isinstance(mod, Linear) or _layer_slices(model, name, mod) is None or mod._nf4 is not None:
            continue
        if not nf4.quantizable(mod.out_features, mod.in_features):
            skipped.append(name)
            continue
        codes, absmax = nf4.quantize_nf4(mod.weight)
        mod.weight = None
        mod.register_buffer("weight_nf4", codes)
        mod.register_buffer("weight_absmax", absmax)
        mod._nf4 = True
    return skipped


def frozen_bytes(model) -> int:
    """Bytes of the parameters that take no gradient plus the NF4 buffers (tied parameters once)."""
    seen, total = set(), 0
    for p in model.parameters():
        if id(p) not in seen and not p.requires_grad:
            seen.add(id(p))
            total += p.numel() * p.element_size()
    for _, m in quantized_layers(model):
        total += m.weight_nf4.numel() + 4 * m.weight_absmax.numel()
    return total


def adapter_slice_index(ad: Adapter) -> int:
    return ad.c0 // ad.n


@torch.no_grad()
def merge_lora(model: nn.Module) -> nn.Module:
    """Fold every adapter into its base weight — ``W[c0:c0+n] += scale · B A``, with a DoRA magnitude
    ``W[c0:c0+n] = (m / ‖W[c0:c0+n] + scale · B A‖) ⊙ (W[c0:c0+n] + scale · B A)``, computed in fp32 and rounded once —
    and remove the adapters: a plain model (parameters trainable as before ``apply_lora``).  A layer held as NF4 codes
    is dequantised in fp32 first, so its merged weight is rounded to the model dtype once."""
    if not has_lora(model):
        raise RuntimeError("merge_lora: the model carries no adapters")
    dtype = next(model.parameters()).dtype
    dequantized = [mod for _, mod in quantized_layers(model)]
    for mod in dequantized:  # back to an ordinary weight: fp32 until the adapters are folded in, so ONE rounding
        w = nf4.dequantize_nf4(mod.weight_nf4, mod.weight_absmax, torch.float32)
        mod.weight = nn.Parameter(w, requires_grad=False)
        del mod.weight_nf4, mod.weight_absmax, mod._nf4
    model.__dict__.pop("_nf4_report", None)
    for _, mod in adapted_layers(model):
        adapters, _ = mod._lora
        for ad in adapters:
            rows = mod.weight[ad.c0:ad.c0 + ad.n]
            merged = rows.float() + ad.scale * (ad.B.float() @ ad.A.float())
            if ad.m is not None:
                merged = merged * (ad.m.float() / torch.linalg.vector_norm(merged, dim=1)).unsqueeze(1)
            rows.copy_(merged.to(rows.dtype))
            i = adapter_slice_index(ad)
            delattr(mod, f"lora_A_{i}")
            delattr(mod, f"lora_B_{i}")
            if ad.m is not None:
                delattr(mod, f"lora_m_{i}")
        del mod._lora  # back to the class default: no adapters
        mod.__dict__.pop("_dora_c", None)
    for mod in dequantized:
        mod.weight.data = mod.weight.data.to(dtype)
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
