"""HF-compatible checkpoint I/O: ``config.json`` + ``generation_config.json`` + ``model.safetensors``.

The reference saves with ``model.save_pretrained(output_dir)`` (ref/helpers.py:13); the files it
writes are reproduced here so ``transformers.AutoModelForSeq2SeqLM.
from_pretrained(our_output)`` loads our checkpoints and we load theirs.  Internally q/k/v,
cross-attention k/v and gated wi_0/wi_1 are fused weights (models/t5.py, models/bart.py); this module
splits/concatenates them.  Tied weights are stored once (``shared.weight`` /
``model.shared.weight``), as safetensors de-duplication does in ``save_pretrained``.
Loading uses safetensors only — nothing that can execute code from the file.
"""
from __future__ import annotations

import json
import os

import torch
from safetensors.torch import load_file, save_file

from .bart import BartForConditionalGeneration
from .config import Seq2SeqConfig, resolve_config
from .t5 import T5ForConditionalGeneration
from .t5gemma import T5GemmaForConditionalGeneration

_FUSED_T5 = {".qkv.weight": [".q.weight", ".k.weight", ".v.weight"], ".kv.weight": [".k.weight", ".v.weight"]}
_FUSED_BART = {".qkv_proj.": [".q_proj.", ".k_proj.", ".v_proj."], ".kv_proj.": [".k_proj.", ".v_proj."]}
# LED's encoder self-attention (modeling_led.py LEDEncoderAttention: longformer_self_attn + output), tried first
_LS = ".self_attn.longformer_self_attn."
_FUSED_LED = {".self_attn.qkv_proj.": [_LS + "query.", _LS + "key.", _LS + "value."],
              ".self_attn.kv_global.": [_LS + "key_global.", _LS + "value_global."],
              ".self_attn.q_global.": [_LS + "query_global."],
              ".self_attn.out_proj.": [".self_attn.output."]}
# BigBird-Pegasus (modeling_bigbird_pegasus.py): the encoder's self-attention is BigBirdPegasusEncoderAttention (self.
# {query, key, value} + output), and each stack's FINAL LayerNorm is called layernorm_embedding
_BS = ".self_attn.self."
_FUSED_BIGBIRD_ENC = {".self_attn.qkv_proj.": [_BS + "query.", _BS + "key.", _BS + "value."],
                      ".self_attn.out_proj.": [".self_attn.output."]}


def _t5gemma_names(cfg, name):
    """T5Gemma (modeling_t5gemma.py): ``(transformers' names, rows of each)`` of our parameter ``name`` — the fused
    ``qkv_proj`` is q (H D rows), k and v (H_kv D rows each); ``kv_proj`` and the gated ``mlp.wi`` split in halves
    (None: equal parts); ``mlp.wo`` is ``down_proj``."""
    if ".self_attn.qkv_proj." in name:
        hd, kd = cfg.num_heads * cfg.d_kv, cfg.num_kv_heads * cfg.d_kv
        return [name.replace(".qkv_proj.", p) for p in (".q_proj.", ".k_proj.", ".v_proj.")], [hd, kd, kd]
    if ".cross_attn.kv_proj." in name:
        return [name.replace(".kv_proj.", p) for p in (".k_proj.", ".v_proj.")], None
    if ".mlp.wi." in name:
        return [name.replace(".mlp.wi.", p) for p in (".mlp.gate_proj.", ".mlp.up_proj.")], None
    if ".mlp.wo." in name:
        return [name.replace(".mlp.wo.", ".mlp.down_proj.")], None
    return [name], None


def _split_rows(t, names, sizes):
    return t.split(sizes, 0) if sizes is not None else t.chunk(len(names), 0)


def _hf_names(cfg, name):
    """(transformers' parameter names that our ``name`` is the concatenation of, along dim 0) — or None when it maps
    to itself.  LED: transformers' prefix is ``led.`` and its encoder self-attention has names of its own."""
    if cfg.model_type == "led":
        if name.startswith("model."):
            name = "led." + name[len("model."):]
        if name.startswith("led.encoder."):
            for key, parts in _FUSED_LED.items():
                if key in name:
                    return [name.replace(key, p) for p in parts]
    if cfg.model_type == "bigbird_pegasus":
        for stack in ("model.encoder.", "model.decoder."):
            if name.startswith(stack + "layer_norm."):
                return [name.replace(stack + "layer_norm.", stack + "layernorm_embedding.")]
        if name.startswith("model.encoder."):
            for key, parts in _FUSED_BIGBIRD_ENC.items():
                if key in name:
                    return [name.replace(key, p) for p in parts]
    for key, parts in _FUSED_BART.items():
        if key in name:
            return [name.replace(key, p) for p in parts]
    return [name] if cfg.model_type == "led" else None


def build_model(cfg_or_name, dtype=torch.float32, device="cpu"):
    cfg = cfg_or_name if isinstance(cfg_or_name, Seq2SeqConfig) else resolve_config(cfg_or_name)
    cls = (T5ForConditionalGeneration if cfg.model_type == "t5" else
           T5GemmaForConditionalGeneration if cfg.model_type == "t5gemma" else BartForConditionalGeneration)
    with torch.device(device):
        model = cls(cfg)
    return model.to(dtype=dtype)


def to_hf_state_dict(model) -> dict[str, torch.Tensor]:
    cfg: Seq2SeqConfig = model.config
    out = {}
    for name, t in model.state_dict().items():
        t = t.detach()
        if _is_adapter_key(name):  # adapters have a checkpoint of their own (save_adapter)
            continue
        if cfg.model_type == "t5gemma":
            names, sizes = _t5gemma_names(cfg, name)
            for part, piece in zip(names, _split_rows(t, names, sizes)):
                out[part] = piece
        elif cfg.model_type == "t5":
            if name.endswith(".wi.weight") and cfg.is_gated:
                a, b = t.chunk(2, dim=0)
                out[name.replace(".wi.weight", ".wi_0.weight")] = a
                out[name.replace(".wi.weight", ".wi_1.weight")] = b
                continue
            done = False
            for suf, parts in _FUSED_T5.items():
                if name.endswith(suf):
                    for part, piece in zip(parts, t.chunk(len(parts), dim=0)):
                        out[name[: -len(suf)] + part] = piece
                    done = True
            if not done:
                out[name] = t
        else:
            names = _hf_names(cfg, name)
            if names is None:
                out[name] = t
            else:
                for part, piece in zip(names, t.chunk(len(names), dim=0)):
                    out[part] = piece
    if cfg.local_encoder and not cfg.tie_word_embeddings:
        # transformers' LongT5 ties encoder / decoder embed_tokens to `shared` only under tie_word_embeddings, so an
        # untied checkpoint carries them (as the published LongT5 checkpoints do); without them it would load random
        # embeddings.  Copies: safetensors refuses tensors that share memory
        for stack in ("encoder", "decoder"):
            out[f"{stack}.embed_tokens.weight"] = out["shared.weight"].clone()
    return {k: v.contiguous() for k, v in out.items()}


def from_hf_state_dict(model, sd: dict[str, torch.Tensor], strict: bool = True):
    cfg: Seq2SeqConfig = model.config
    own = model.state_dict()
    new = {}
    for name in own:
        if _is_adapter_key(name):
            continue
        if cfg.model_type == "t5gemma":
            names, _ = _t5gemma_names(cfg, name)
            if all(p in sd for p in names):
                new[name] = torch.cat([sd[p] for p in names], 0) if len(names) > 1 else sd[names[0]]
            elif name == "lm_head.out_proj.weight" and "model.decoder.embed_tokens.weight" in sd:
                new[name] = sd["model.decoder.embed_tokens.weight"]
            elif name == "model.decoder.embed_tokens.weight" and "lm_head.out_proj.weight" in sd:
                new[name] = sd["lm_head.out_proj.weight"]  # a tied checkpoint that kept the head's name
        elif cfg.model_type == "t5":
            if name.endswith(".wi.weight") and cfg.is_gated:
                new[name] = torch.cat([sd[name.replace(".wi.weight", ".wi_0.weight")],
                                       sd[name.replace(".wi.weight", ".wi_1.weight")]], 0)
                continue
            hit = None
            for suf, parts in _FUSED_T5.items():
                if name.endswith(suf):
                    hit = torch.cat([sd[name[: -len(suf)] + p] for p in parts], 0)
            if hit is not None:
                new[name] = hit
            elif name in sd:
                new[name] = sd[name]
            elif name == "lm_head.weight" and "shared.weight" in sd:
                new[name] = sd["shared.weight"]
        else:
            names = _hf_names(cfg, name)
            if names is not None and all(p in sd for p in names):
                new[name] = torch.cat([sd[p] for p in names], 0) if len(names) > 1 else sd[names[0]]
            elif names is not None and len(names) > 1:
                raise KeyError(f"missing keys in checkpoint: {[p for p in names if p not in sd]}")
            elif names is None and name in sd:
                new[name] = sd[name]
            elif name.endswith("shared.weight") and "lm_head.weight" in sd:
                new[name] = sd["lm_head.weight"]
    # fixed sinusoidal position tables are a function of (max_position_embeddings, d_model): transformers' Marian drops
    # them on save (_keys_to_ignore_on_save) and our module already holds the exact table, so their absence is not an
    # error (Pegasus checkpoints do carry them and they are loaded like any other key)
    derived = {n + ".weight" for n, m in model.named_modules() if getattr(m, "derived_table", False)}
    missing = [k for k in own if k not in new and k not in derived and not _is_adapter_key(k)]
    if strict and missing:
        raise KeyError(f"missing keys in checkpoint: {missing[:8]}{'...' if len(missing) > 8 else ''}")
    with torch.no_grad():
        for k, v in new.items():
            own[k].copy_(v.to(own[k].dtype))
    return missing


def save_pretrained(model, output_dir: str, dtype=torch.float32) -> list[str]:
    """Write config.json, generation_config.json, model.safetensors.  Returns written file names."""
    os.makedirs(output_dir, exist_ok=True)
    model.config.save(output_dir)
    sd = {k: v.to("cpu", dtype=dtype if v.is_floating_point() else v.dtype) for k, v in to_hf_state_dict(model).items()}
    save_file(sd, os.path.join(output_dir, "model.safetensors"), metadata={"format": "pt"})
    return ["config.json", "generation_config.json", "model.safetensors"]


def from_pretrained(name_or_path: str, dtype=torch.float32, device="cpu"):
    """Build a model from a preset name / HF id (random init, HF init rules) or from a directory
    written by us or by ``transformers`` (``model.safetensors``)."""
    cfg = resolve_config(name_or_path)
    model = build_model(cfg, dtype=torch.float32, device="cpu")
    if name_or_path and os.path.isdir(name_or_path):
        st = os.path.join(name_or_path, "model.safetensors")
        if os.path.exists(st):
            from_hf_state_dict(model, load_file(st))
    return model.to(device=device, dtype=dtype)


# ------------------------------------------------------------------------------------------------ LoRA adapters
# PEFT's checkpoint layout, written from its documented format (peft is not installed where this was developed):
# adapter_config.json (peft_type LORA, task_type SEQ_2_SEQ_LM, r, lora_alpha, lora_dropout, target_modules) and
# adapter_model.safetensors with keys base_model.model.<HF module path>.lora_A.weight [r, in] / .lora_B.weight [out, r],
# where the module path is transformers' name of the UNFUSED projection (the mapping of to_hf_state_dict).


def _is_adapter_key(name: str) -> bool:
    leaf = name.rsplit(".", 1)[-1]
    return leaf.startswith("lora_A_") or leaf.startswith("lora_B_")


def hf_param_names(cfg, name: str) -> list[str]:
    """transformers' names of the parameters our parameter ``name`` is the concatenation of (along dim 0)."""
    if cfg.model_type == "t5gemma":
        return _t5gemma_names(cfg, name)[0]
    if cfg.model_type == "t5":
        if name.endswith(".wi.weight") and cfg.is_gated:
            return [name.replace(".wi.weight", ".wi_0.weight"), name.replace(".wi.weight", ".wi_1.weight")]
        for suf, parts in _FUSED_T5.items():
            if name.endswith(suf):
                return [name[: -len(suf)] + p for p in parts]
        return [name]
    names = _hf_names(cfg, name)
    return [name] if names is None else names


def hf_param_parts(cfg, name: str):
    """How our parameter ``name`` splits along dim 0 into transformers' parameters: their number when the slices are
    equal, else the list of their dim-0 sizes (T5Gemma's ``qkv_proj`` with grouped K/V heads: q is longer than k and
    v).  What a per-transformers-parameter rule such as Adafactor's factored moments takes (ops/optim.py)."""
    if cfg.model_type == "t5gemma":
        names, sizes = _t5gemma_names(cfg, name)
        return list(sizes) if sizes is not None and len(set(sizes)) > 1 else len(names)
    return len(hf_param_names(cfg, name))


# leaf module names of transformers' projections -> our logical LoRA targets (models/lora.py)
_LEAF_TARGET = {"q": "q", "q_proj": "q", "query": "q", "k": "k", "k_proj": "k", "key": "k", "v": "v", "v_proj": "v",
                "value": "v", "o": "o", "out_proj": "o", "output": "o", "wi": "wi", "wi_0": "wi", "wi_1": "wi",
                "fc1": "wi", "wo": "wo", "fc2": "wo"}


def adapter_keys(model) -> dict:
    """{PEFT key: parameter} of every adapter matrix of ``model``."""
    from .lora import adapted_layers, adapter_slice_index
    out = {}
    for name, mod in adapted_layers(model):
        paths = [n[: -len(".weight")] for n in hf_param_names(model.config, name + ".weight")]
        for ad in mod._lora[0]:
            path = paths[adapter_slice_index(ad)]
            out[f"base_model.model.{path}.lora_A.weight"] = ad.A
            out[f"base_model.model.{path}.lora_B.weight"] = ad.B
    return out


def save_adapter(model, output_dir: str) -> list[str]:
    """Write the adapters of a model under ``apply_lora`` in PEFT's layout.  Returns the written file names."""
    from .lora import has_lora
    if not has_lora(model):
        raise RuntimeError("save_adapter: the model carries no adapters (models/lora.py apply_lora)")
    os.makedirs(output_dir, exist_ok=True)
    cfg = model._lora_cfg
    keys = adapter_keys(model)
    leaves = sorted({k.split(".")[-3] for k in keys})
    conf = {"peft_type": "LORA", "task_type": "SEQ_2_SEQ_LM", "r": int(cfg.r), "lora_alpha": cfg.alpha,
            "lora_dropout": float(cfg.dropout), "target_modules": leaves, "bias": "none", "fan_in_fan_out": False,
            "inference_mode": True, "base_model_name_or_path": None}
    with open(os.path.join(output_dir, "adapter_config.json"), "w") as f:
        json.dump(conf, f, indent=2, sort_keys=True)
    sd = {k: v.detach().to("cpu").contiguous().clone() for k, v in keys.items()}
    save_file(sd, os.path.join(output_dir, "adapter_model.safetensors"), metadata={"format": "pt"})
    return ["adapter_config.json", "adapter_model.safetensors"]


def load_adapter(model, adapter_dir: str):
    """Load an adapter checkpoint written by ``save_adapter`` (or PEFT) into ``model``; a model without adapters gets
    them first (``apply_lora`` with the checkpoint's rank, alpha, dropout and targets)."""
    from .lora import TARGETS, LoraConfig, apply_lora, has_lora
    with open(os.path.join(adapter_dir, "adapter_config.json")) as f:
        conf = json.load(f)
    if conf.get("peft_type") != "LORA":
        raise ValueError(f"load_adapter: peft_type {conf.get('peft_type')!r} is not LORA")
    if not has_lora(model):
        unknown = [m for m in conf["target_modules"] if m not in _LEAF_TARGET]
        if unknown:
            raise ValueError(f"load_adapter: target modules {unknown} have no counterpart here")
        named = {_LEAF_TARGET[m] for m in conf["target_modules"]}
        targets = tuple(t for t in TARGETS if t in named)
        apply_lora(model, LoraConfig(r=int(conf["r"]), alpha=conf["lora_alpha"], dropout=float(conf["lora_dropout"]),
                                     targets=targets))
    sd = load_file(os.path.join(adapter_dir, "adapter_model.safetensors"))
    keys = adapter_keys(model)
    missing = [k for k in keys if k not in sd]
    extra = [k for k in sd if k not in keys]
    if missing or extra:
        raise KeyError(f"load_adapter: missing keys {missing[:4]}, unexpected keys {extra[:4]}")
    with torch.no_grad():
        for k, p in keys.items():
            if tuple(sd[k].shape) != tuple(p.shape):
                raise ValueError(f"load_adapter: {k} has shape {tuple(sd[k].shape)}, the model's is {tuple(p.shape)}")
            p.copy_(sd[k].to(p.dtype))
    return model
