"""Model configurations for the seq2seq families the reference fine-tunes.

The reference loads every model through ``AutoModelForSeq2SeqLM.from_pretrained(model_ckpt)``
(ref/train-torchrun.py:35, ref/train-accelerator.py:41, ref/train-task.py:83); the default
checkpoint is ``facebook/bart-large-cnn`` (ref/valohai.yaml:10,36,65) and the benchmark family is
T5 (BASELINE.json).  There is no network here, so the public configs are encoded as presets and
weights are random-initialised with the HF initialisation rules (SURVEY.md §7.3 "Offline
environment").  ``Seq2SeqConfig.to_hf_dict`` / ``from_hf_dict`` read and write an HF
``config.json`` so checkpoints round-trip with ``transformers``.
"""
from __future__ import annotations

import copy
import dataclasses
import json
import os
from dataclasses import dataclass, field


@dataclass
class Seq2SeqConfig:
    # "t5" | BART family: "bart" | "mbart" | "pegasus" | "marian" | "m2m_100" | "plbart" | "blenderbot" | "led" |
    # "bigbird_pegasus" | "t5gemma"
    model_type: str = "t5"
    # T5 implementation variants: "t5" / "mt5" (same layers), "umt5" (every self-attention layer owns its
    # relative-position bias table: modeling_umt5.py UMT5LayerSelfAttention, has_relative_attention_bias=True),
    # "longt5" (T5 v1.1 layers whose ENCODER self-attention is a sliding window: modeling_longt5.py)
    t5_flavor: str = "t5"
    vocab_size: int = 32128
    d_model: int = 512
    d_kv: int = 64
    d_ff: int = 2048
    num_layers: int = 6
    num_decoder_layers: int = 6
    num_heads: int = 8
    # T5 relative position bias (modeling_t5.py:217-279)
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    # LongT5 (t5_flavor="longt5"): "local" = every encoder query sees the keys within local_radius on either side.
    # "transient-global" (global aggregate tokens of global_block_size inputs) is not implemented; global_block_size
    # is only passed through config.json
    encoder_attention_type: str = "local"
    local_radius: int = 127
    global_block_size: int = 16
    # "relu" (T5 v1.0), "gated-gelu" (flan / v1.1, gelu_new), "gelu" (BART, erf)
    feed_forward_proj: str = "relu"
    dropout_rate: float = 0.1
    attention_dropout: float = 0.1  # T5 applies dropout_rate to probs; BART uses attention_dropout
    activation_dropout: float = 0.0  # BART only (T5 uses dropout_rate inside the FFN)
    layer_norm_epsilon: float = 1e-6
    initializer_factor: float = 1.0  # T5
    init_std: float = 0.02  # BART
    tie_word_embeddings: bool = True
    # recompute each transformer block in backward (O(layers) less activation memory; long sequences)
    gradient_checkpointing: bool = False
    scale_decoder_outputs: bool = True  # T5: scale by d_model**-0.5 before lm_head when tied
    # BART specifics
    max_position_embeddings: int = 1024
    scale_embedding: bool = False
    final_logits_bias: bool = False
    # BART-family variants (transformers modeling_mbart.py / modeling_pegasus.py / modeling_marian.py):
    # pre-LN layers with a final LayerNorm per stack (mBART, Pegasus) vs post-LN (BART, Marian); LayerNorm after
    # the embeddings (BART, mBART); learned positions with offset 2 (BART, mBART) vs fixed sinusoidal (Pegasus,
    # Marian); decoder start token = the last non-pad label token (mBART's language id) vs a fixed id
    normalize_before: bool = False
    layernorm_embedding: bool = True
    position_embedding: str = "learned"  # "learned" (offset 2) | "learned0" | "sinusoidal" | "sinusoidal_m2m"
    shift_mode: str = "standard"  # "standard" | "mbart"
    # LED (model_type="led", modeling_led.py): BART layers whose ENCODER self-attention is Longformer's — a sliding
    # window of attention_window[layer] // 2 keys on either side plus global tokens (models/bart.py).  One even,
    # positive window per encoder layer (an int is expanded); the encoder's learned positions have a table of their
    # own size, and max_position_embeddings stays the decoder's (config.json: max_decoder_position_embeddings)
    attention_window: list | int | None = None
    max_encoder_position_embeddings: int | None = None
    # BigBird-Pegasus (model_type="bigbird_pegasus", modeling_bigbird_pegasus.py): Pegasus-like pre-LN layers whose
    # ENCODER self-attention is BigBird's block-sparse pattern (models/bigbird.py) when attention_type is
    # "block_sparse" and the input is longer than (5 + 2 num_random_blocks) block_size tokens, full attention
    # otherwise ("original_full": always); use_bias: the attention projections carry a bias (false in the public
    # checkpoints)
    attention_type: str = "block_sparse"
    block_size: int = 64
    num_random_blocks: int = 3
    use_bias: bool = True
    # T5Gemma (model_type="t5gemma", modeling_t5gemma.py; models/t5gemma.py): Gemma 2 layers in both stacks.  d_kv is
    # Gemma's head_dim, d_ff its intermediate_size, layer_norm_epsilon its rms_norm_eps, init_std its
    # initializer_range, max_position_embeddings the encoder's; decoder_start_token_id is decoder.bos_token_id.
    # num_kv_heads: K/V heads (None: num_heads), each serving num_heads / num_kv_heads query heads; scores are
    # attn_logit_softcapping * tanh(q.k * query_pre_attn_scalar**-0.5 / attn_logit_softcapping) (None: no cap) and the
    # logits final_logit_softcapping * tanh(x / final_logit_softcapping); rotate-half RoPE with rope_theta;
    # layer_types / decoder_layer_types: per layer "sliding_attention" (keys within sliding_window /
    # decoder_sliding_window) or "full_attention" (None: alternating, sliding first)
    num_kv_heads: int | None = None
    query_pre_attn_scalar: int = 256
    attn_logit_softcapping: float | None = None
    final_logit_softcapping: float | None = None
    rope_theta: float = 10000.0
    sliding_window: int | None = None
    decoder_sliding_window: int | None = None
    layer_types: list | None = None
    decoder_layer_types: list | None = None
    decoder_max_position_embeddings: int | None = None
    # special tokens
    pad_token_id: int = 0
    eos_token_id: int = 1
    bos_token_id: int | None = None
    decoder_start_token_id: int = 0
    forced_bos_token_id: int | None = None
    forced_eos_token_id: int | None = None
    # generation defaults written to generation_config.json
    generation: dict = field(default_factory=dict)
    name: str = ""

    def __post_init__(self):
        if self.model_type == "t5gemma":
            kv = self.num_kv_heads if self.num_kv_heads is not None else self.num_heads
            if kv < 1 or self.num_heads % kv:
                raise ValueError(f"T5Gemma: num_heads ({self.num_heads}) must be a multiple of num_kv_heads ({kv})")
            self.num_kv_heads = kv
            for attr, n in (("layer_types", self.num_layers), ("decoder_layer_types", self.num_decoder_layers)):
                lt = getattr(self, attr)
                if lt is None:  # T5GemmaModuleConfig's default
                    lt = ["sliding_attention" if (i + 1) % 2 else "full_attention" for i in range(n)]
                lt = list(lt)
                if len(lt) != n or any(t not in ("sliding_attention", "full_attention") for t in lt):
                    raise ValueError(f"T5Gemma: {attr} needs one of 'sliding_attention' / 'full_attention' per layer "
                                     f"({n}), got {lt}")
                setattr(self, attr, lt)
            for attr, lt in (("sliding_window", self.layer_types), ("decoder_sliding_window", self.decoder_layer_types)):
                w = getattr(self, attr)
                if "sliding_attention" in lt and (not isinstance(w, int) or w < 1):
                    raise ValueError(f"T5Gemma: {attr} must be a positive int with sliding_attention layers, got {w}")
            if self.decoder_max_position_embeddings is None:
                self.decoder_max_position_embeddings = self.max_position_embeddings
            if self.d_kv % 2:
                raise ValueError(f"T5Gemma: head_dim must be even (rotary halves), got {self.d_kv}")
        if self.model_type == "led":
            w = self.attention_window if self.attention_window is not None else 512
            w = [w] * self.num_layers if isinstance(w, int) else list(w)
            if len(w) != self.num_layers:
                raise ValueError(f"LED: attention_window needs one value per encoder layer ({self.num_layers}), got "
                                 f"{len(w)}")
            if any((not isinstance(x, int)) or x <= 0 or x % 2 for x in w):
                raise ValueError(f"LED: every attention_window value must be even and positive, got {w}")
            self.attention_window = w
            if self.max_encoder_position_embeddings is None:
                self.max_encoder_position_embeddings = 16384
        if self.model_type == "bigbird_pegasus":
            if self.attention_type not in ("block_sparse", "original_full"):
                raise ValueError(f"BigBird-Pegasus: attention_type must be 'block_sparse' or 'original_full', got "
                                 f"{self.attention_type!r}")
            if self.block_size < 1 or self.num_random_blocks < 0:
                raise ValueError(f"BigBird-Pegasus: block_size must be >= 1 and num_random_blocks >= 0, got "
                                 f"{self.block_size} and {self.num_random_blocks}")

    @property
    def inner_dim(self) -> int:
        return self.num_heads * self.d_kv

    @property
    def is_gated(self) -> bool:
        return self.feed_forward_proj.startswith("gated")

    @property
    def per_layer_position_bias(self) -> bool:
        return self.model_type == "t5" and self.t5_flavor == "umt5"

    @property
    def local_encoder(self) -> bool:
        return self.model_type == "t5" and self.t5_flavor == "longt5"

    @property
    def act(self) -> str:
        a = self.feed_forward_proj.split("-")[-1]
        if self.feed_forward_proj == "gated-gelu":
            return "gelu_new"
        if a == "swish":  # Marian's name for SiLU
            return "silu"
        return a

    def replace(self, **kw) -> "Seq2SeqConfig":
        """A copy with the fields of ``kw`` set, validated again by ``__post_init__``.  For LED that means
        ``attention_window`` must fit the copy's ``num_layers``: ``replace(num_layers=2)`` on a 6-layer preset raises
        unless ``attention_window`` (a list of 2, or an int, which is expanded) is given with it."""
        c = copy.deepcopy(self)
        for k, v in kw.items():
            if not hasattr(c, k):
                raise AttributeError(k)
            setattr(c, k, v)
        c.__post_init__()
        return c

    # ---------------------------------------------------------------- HF config.json I/O
    def _t5gemma_module(self, decoder: bool) -> dict:
        """One stack's T5GemmaModuleConfig as config.json holds it."""
        return {
            "model_type": "t5_gemma_module",
            "vocab_size": self.vocab_size,
            "hidden_size": self.d_model,
            "intermediate_size": self.d_ff,
            "num_hidden_layers": self.num_decoder_layers if decoder else self.num_layers,
            "num_attention_heads": self.num_heads,
            "num_key_value_heads": self.num_kv_heads,
            "head_dim": self.d_kv,
            "hidden_activation": _GEMMA_ACT_OUT[self.feed_forward_proj],
            "max_position_embeddings": self.decoder_max_position_embeddings if decoder else self.max_position_embeddings,
            "initializer_range": self.init_std,
            "rms_norm_eps": self.layer_norm_epsilon,
            "pad_token_id": self.pad_token_id,
            "eos_token_id": self.eos_token_id,
            "bos_token_id": self.bos_token_id,
            "rope_parameters": {"rope_type": "default", "rope_theta": self.rope_theta},
            "attention_bias": False,
            "attention_dropout": self.attention_dropout,
            "dropout_rate": self.dropout_rate,
            "query_pre_attn_scalar": self.query_pre_attn_scalar,
            "sliding_window": self.decoder_sliding_window if decoder else self.sliding_window,
            "layer_types": list(self.decoder_layer_types if decoder else self.layer_types),
            "final_logit_softcapping": self.final_logit_softcapping,
            "attn_logit_softcapping": self.attn_logit_softcapping,
            "is_decoder": decoder,
            "tie_word_embeddings": self.tie_word_embeddings,
        }

    def to_hf_dict(self) -> dict:
        if self.model_type == "t5gemma":
            return {
                "architectures": ["T5GemmaForConditionalGeneration"],
                "model_type": "t5gemma",
                "encoder": self._t5gemma_module(False),
                "decoder": self._t5gemma_module(True),
                "is_encoder_decoder": True,
                "dropout_rate": self.dropout_rate,
                "attention_dropout": self.attention_dropout,
                "tie_word_embeddings": self.tie_word_embeddings,
                "vocab_size": self.vocab_size,
                # the width under the name every other family's config.json has.  transformers keeps a key it does not
                # know as an attribute, so `AutoConfig.for_model(...).d_model` answers for this family as for the
                # others: tests/test_model_parity.py test_every_preset_round_trips_through_config_json reads it off
                # every preset's transformers config
                "d_model": self.d_model,
                "initializer_range": self.init_std,
                "pad_token_id": self.pad_token_id,
                "eos_token_id": self.eos_token_id,
                "bos_token_id": self.bos_token_id,
                "torch_dtype": "float32",
            }
        if self.model_type == "t5":
            d = {
                "architectures": [{"t5": "T5ForConditionalGeneration", "mt5": "MT5ForConditionalGeneration",
                                   "umt5": "UMT5ForConditionalGeneration",
                                   "longt5": "LongT5ForConditionalGeneration"}[self.t5_flavor]],
                "model_type": self.t5_flavor,
                "vocab_size": self.vocab_size,
                "d_model": self.d_model,
                "d_kv": self.d_kv,
                "d_ff": self.d_ff,
                "num_layers": self.num_layers,
                "num_decoder_layers": self.num_decoder_layers,
                "num_heads": self.num_heads,
                "relative_attention_num_buckets": self.relative_attention_num_buckets,
                "relative_attention_max_distance": self.relative_attention_max_distance,
                "dropout_rate": self.dropout_rate,
                "layer_norm_epsilon": self.layer_norm_epsilon,
                "initializer_factor": self.initializer_factor,
                "feed_forward_proj": self.feed_forward_proj,
                "is_encoder_decoder": True,
                "pad_token_id": self.pad_token_id,
                "eos_token_id": self.eos_token_id,
                "decoder_start_token_id": self.decoder_start_token_id,
                "tie_word_embeddings": self.tie_word_embeddings,
            }
            if self.local_encoder:
                d.update(encoder_attention_type=self.encoder_attention_type, local_radius=self.local_radius,
                         global_block_size=self.global_block_size)
        else:
            arch = {"bart": "BartForConditionalGeneration", "mbart": "MBartForConditionalGeneration",
                    "pegasus": "PegasusForConditionalGeneration", "marian": "MarianMTModel",
                    "m2m_100": "M2M100ForConditionalGeneration", "plbart": "PLBartForConditionalGeneration",
                    "blenderbot": "BlenderbotForConditionalGeneration",
                    "led": "LEDForConditionalGeneration",
                    "bigbird_pegasus": "BigBirdPegasusForConditionalGeneration"}[self.model_type]
            d = {
                "architectures": [arch],
                "model_type": self.model_type,
                "vocab_size": self.vocab_size,
                "d_model": self.d_model,
                "encoder_layers": self.num_layers,
                "decoder_layers": self.num_decoder_layers,
                "encoder_attention_heads": self.num_heads,
                "decoder_attention_heads": self.num_heads,
                "encoder_ffn_dim": self.d_ff,
                "decoder_ffn_dim": self.d_ff,
                "activation_function": self.feed_forward_proj,
                "dropout": self.dropout_rate,
                "attention_dropout": self.attention_dropout,
                "activation_dropout": self.activation_dropout,
                "init_std": self.init_std,
                "max_position_embeddings": self.max_position_embeddings,
                "scale_embedding": self.scale_embedding,
                "is_encoder_decoder": True,
                "pad_token_id": self.pad_token_id,
                "bos_token_id": self.bos_token_id,
                "eos_token_id": self.eos_token_id,
                "decoder_start_token_id": self.decoder_start_token_id,
                "forced_bos_token_id": self.forced_bos_token_id,
                "forced_eos_token_id": self.forced_eos_token_id,
                "tie_word_embeddings": True,
                "encoder_layerdrop": 0.0,
                "decoder_layerdrop": 0.0,
            }
            if self.model_type == "marian":
                d["decoder_vocab_size"] = self.vocab_size
                d["share_encoder_decoder_embeddings"] = True
            if self.model_type == "led":  # LEDConfig: two position tables, no scale_embedding
                del d["max_position_embeddings"], d["scale_embedding"]
                d.update(attention_window=list(self.attention_window),
                         max_encoder_position_embeddings=self.max_encoder_position_embeddings,
                         max_decoder_position_embeddings=self.max_position_embeddings)
            if self.model_type == "bigbird_pegasus":
                d.update(attention_type=self.attention_type, block_size=self.block_size,
                         num_random_blocks=self.num_random_blocks, use_bias=self.use_bias)
        d["torch_dtype"] = "float32"
        return d

    @classmethod
    def _from_t5gemma(cls, d: dict) -> "Seq2SeqConfig":
        """config.json of a T5Gemma checkpoint: nested ``encoder`` / ``decoder`` Gemma 2 module configs
        (configuration_t5gemma.py; a missing key takes T5GemmaModuleConfig's default).  The two stacks share one head
        geometry here, so they must agree in it; layer counts, layer types, windows and position limits may differ."""
        enc, dec = dict(d.get("encoder") or {}), dict(d.get("decoder") or {})
        dflt = {"vocab_size": 256000, "hidden_size": 2304, "intermediate_size": 9216, "num_hidden_layers": 26,
                "num_attention_heads": 8, "num_key_value_heads": 4, "head_dim": 256,
                "hidden_activation": "gelu_pytorch_tanh", "max_position_embeddings": 8192, "initializer_range": 0.02,
                "rms_norm_eps": 1e-6, "pad_token_id": 0, "eos_token_id": 1, "bos_token_id": 2,
                "query_pre_attn_scalar": 256, "sliding_window": 4096, "layer_types": None,
                "final_logit_softcapping": 30.0, "attn_logit_softcapping": 50.0, "attention_bias": False}
        e, c = {**dflt, **enc}, {**dflt, **dec}
        for k in ("hidden_size", "head_dim", "num_attention_heads", "num_key_value_heads", "intermediate_size",
                  "vocab_size", "hidden_activation", "rms_norm_eps", "query_pre_attn_scalar",
                  "attn_logit_softcapping"):
            if e[k] != c[k]:
                raise ValueError(f"T5Gemma: encoder and decoder differ in {k} ({e[k]} and {c[k]}): unbalanced "
                                 "encoder / decoder sizes (such as t5gemma-9b-2b) are not implemented")
        if e["attention_bias"] or c["attention_bias"]:
            raise ValueError("T5Gemma: attention_bias is not implemented")
        if e["hidden_activation"] not in _GEMMA_ACT_IN:
            raise ValueError(f"T5Gemma: unsupported hidden_activation {e['hidden_activation']!r}")

        def theta(m):
            rp = m.get("rope_parameters") or {}
            if rp.get("rope_type", "default") != "default":
                raise ValueError(f"T5Gemma: rope_type {rp.get('rope_type')!r} is not implemented")
            return float(rp.get("rope_theta", m.get("rope_theta", 10000.0)))

        if theta(e) != theta(c):
            raise ValueError(f"T5Gemma: encoder and decoder differ in rope_theta ({theta(e)} and {theta(c)})")
        return cls(
            model_type="t5gemma", vocab_size=d.get("vocab_size", c["vocab_size"]), d_model=e["hidden_size"],
            d_kv=e["head_dim"], d_ff=e["intermediate_size"], num_layers=e["num_hidden_layers"],
            num_decoder_layers=c["num_hidden_layers"], num_heads=e["num_attention_heads"],
            num_kv_heads=e["num_key_value_heads"], feed_forward_proj=_GEMMA_ACT_IN[e["hidden_activation"]],
            dropout_rate=d.get("dropout_rate", 0.0), attention_dropout=d.get("attention_dropout", 0.0),
            layer_norm_epsilon=e["rms_norm_eps"], init_std=d.get("initializer_range", c["initializer_range"]),
            tie_word_embeddings=d.get("tie_word_embeddings", True), scale_decoder_outputs=False,
            max_position_embeddings=e["max_position_embeddings"],
            decoder_max_position_embeddings=c["max_position_embeddings"],
            query_pre_attn_scalar=e["query_pre_attn_scalar"], attn_logit_softcapping=e["attn_logit_softcapping"],
            final_logit_softcapping=c["final_logit_softcapping"], rope_theta=theta(e),
            sliding_window=e["sliding_window"], decoder_sliding_window=c["sliding_window"],
            layer_types=e["layer_types"], decoder_layer_types=c["layer_types"],
            pad_token_id=c["pad_token_id"], eos_token_id=_first(c["eos_token_id"]), bos_token_id=c["bos_token_id"],
            decoder_start_token_id=c["bos_token_id"],
        )

    @classmethod
    def from_hf_dict(cls, d: dict) -> "Seq2SeqConfig":
        mt = d.get("model_type", "t5")
        if mt == "t5gemma":
            return cls._from_t5gemma(d)
        if mt in ("t5", "mt5", "umt5", "longt5"):
            extra = {}
            if mt == "longt5":
                eat = d.get("encoder_attention_type", "local")
                if eat != "local":
                    raise ValueError(f"unsupported LongT5 encoder_attention_type {eat!r}: only 'local' is implemented "
                                     "(transient-global needs global aggregate tokens)")
                extra = dict(encoder_attention_type=eat, local_radius=d.get("local_radius", 127),
                             global_block_size=d.get("global_block_size", 16))
            ff = d.get("feed_forward_proj", "relu")
            nl = d.get("num_layers", 6)
            tie = d.get("tie_word_embeddings", True)
            return cls(
                model_type="t5", t5_flavor=mt, vocab_size=d.get("vocab_size", 32128), d_model=d.get("d_model", 512),
                d_kv=d.get("d_kv", 64), d_ff=d.get("d_ff", 2048), num_layers=nl,
                num_decoder_layers=d.get("num_decoder_layers") or nl, num_heads=d.get("num_heads", 8),
                relative_attention_num_buckets=d.get("relative_attention_num_buckets", 32),
                relative_attention_max_distance=d.get("relative_attention_max_distance", 128),
                feed_forward_proj=ff, dropout_rate=d.get("dropout_rate", 0.1),
                attention_dropout=d.get("dropout_rate", 0.1),
                layer_norm_epsilon=d.get("layer_norm_epsilon", 1e-6),
                initializer_factor=d.get("initializer_factor", 1.0),
                tie_word_embeddings=tie, scale_decoder_outputs=tie,
                pad_token_id=d.get("pad_token_id", 0), eos_token_id=_first(d.get("eos_token_id", 1)),
                decoder_start_token_id=d.get("decoder_start_token_id", 0) or 0, **extra,
            )
        if mt in _FAMILY:
            fam = {"final_logits_bias": True, **_FAMILY[mt]}
            if mt == "led":
                fam.update(attention_window=d.get("attention_window", 512),
                           max_encoder_position_embeddings=d.get("max_encoder_position_embeddings", 16384))
                d = {**d, "max_position_embeddings": d.get("max_decoder_position_embeddings", 1024)}
            if mt == "bigbird_pegasus":  # BigBirdPegasusConfig's defaults where the file is silent
                fam.update(attention_type=d.get("attention_type", "block_sparse"), block_size=d.get("block_size", 64),
                           num_random_blocks=d.get("num_random_blocks", 3), use_bias=d.get("use_bias", False))
                d = {"vocab_size": 96103, "encoder_layers": 16, "decoder_layers": 16, "activation_function": "gelu_new",
                     "max_position_embeddings": 4096, "scale_embedding": True, "pad_token_id": 0, "eos_token_id": 1,
                     "bos_token_id": 2, "decoder_start_token_id": 2, "forced_eos_token_id": None, **d}
            return cls(
                model_type=mt, vocab_size=d.get("vocab_size", 50265), d_model=d.get("d_model", 1024),
                d_kv=d.get("d_model", 1024) // d.get("encoder_attention_heads", 16),
                d_ff=d.get("encoder_ffn_dim", 4096), num_layers=d.get("encoder_layers", 12),
                num_decoder_layers=d.get("decoder_layers", 12), num_heads=d.get("encoder_attention_heads", 16),
                feed_forward_proj=d.get("activation_function", "gelu"), dropout_rate=d.get("dropout", 0.1),
                attention_dropout=d.get("attention_dropout", 0.0),
                activation_dropout=d.get("activation_dropout", 0.0), layer_norm_epsilon=1e-5,
                init_std=d.get("init_std", 0.02), max_position_embeddings=d.get("max_position_embeddings", 1024),
                scale_embedding=d.get("scale_embedding", False),
                tie_word_embeddings=True, scale_decoder_outputs=False,
                pad_token_id=d.get("pad_token_id", 1), eos_token_id=_first(d.get("eos_token_id", 2)),
                bos_token_id=d.get("bos_token_id", 0 if mt in ("bart", "mbart", "led") else None),
                decoder_start_token_id=d.get("decoder_start_token_id") if d.get("decoder_start_token_id") is not None
                else (d.get("pad_token_id", 1) if mt not in ("bart", "led") else 2),
                forced_bos_token_id=d.get("forced_bos_token_id"), forced_eos_token_id=d.get("forced_eos_token_id", 2),
                **fam,
            )
        raise ValueError(f"unsupported model_type {mt!r}")

    def save(self, path: str) -> None:
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(self.to_hf_dict(), f, indent=2, sort_keys=True)
        with open(os.path.join(path, "generation_config.json"), "w") as f:
            json.dump(self.generation_config_dict(), f, indent=2, sort_keys=True)

    def generation_config_dict(self) -> dict:
        g = {"decoder_start_token_id": self.decoder_start_token_id, "eos_token_id": self.eos_token_id,
             "pad_token_id": self.pad_token_id}
        if self.bos_token_id is not None:
            g["bos_token_id"] = self.bos_token_id
        if self.forced_bos_token_id is not None:
            g["forced_bos_token_id"] = self.forced_bos_token_id
        if self.forced_eos_token_id is not None:
            g["forced_eos_token_id"] = self.forced_eos_token_id
        g.update(self.generation)
        return g

    def to_dict(self) -> dict:
        return dataclasses.asdict(self)


def _first(x):
    return x[0] if isinstance(x, (list, tuple)) else x


# Gemma's hidden_activation <-> feed_forward_proj (the gated FFN's activation, ops/ffn.py)
_GEMMA_ACT_IN = {"gelu_pytorch_tanh": "gated-gelu", "gelu_new": "gated-gelu"}
_GEMMA_ACT_OUT = {"gated-gelu": "gelu_pytorch_tanh"}


# structural switches of the BART-family model types (see the Seq2SeqConfig fields)
_FAMILY = {
    "bart": dict(normalize_before=False, layernorm_embedding=True, position_embedding="learned", shift_mode="standard"),
    "mbart": dict(normalize_before=True, layernorm_embedding=True, position_embedding="learned", shift_mode="mbart"),
    "pegasus": dict(normalize_before=True, layernorm_embedding=False, position_embedding="sinusoidal",
                    shift_mode="standard"),
    "marian": dict(normalize_before=False, layernorm_embedding=False, position_embedding="sinusoidal",
                   shift_mode="standard"),
    # PLBart: BART layers with mBART's language-id decoder start (modeling_plbart.py)
    "plbart": dict(normalize_before=False, layernorm_embedding=True, position_embedding="learned", shift_mode="mbart"),
    # Blenderbot: pre-LN, learned positions without offset, no embedding LayerNorm (modeling_blenderbot.py)
    "blenderbot": dict(normalize_before=True, layernorm_embedding=False, position_embedding="learned0",
                       shift_mode="standard"),
    # LED: BART layers, learned positions without offset (modeling_led.py LEDLearnedPositionalEmbedding)
    "led": dict(normalize_before=False, layernorm_embedding=True, position_embedding="learned0", shift_mode="standard"),
    # BigBird-Pegasus: pre-LN with a final LayerNorm per stack (transformers names it layernorm_embedding, models/
    # hf_io.py), no embedding LayerNorm, learned positions without offset (modeling_bigbird_pegasus.py)
    "bigbird_pegasus": dict(normalize_before=True, layernorm_embedding=False, position_embedding="learned0",
                            shift_mode="standard"),
    # M2M100 / NLLB: pre-LN, padding-aware sinusoidal positions (modeling_m2m_100.py), no final_logits_bias
    "m2m_100": dict(normalize_before=True, layernorm_embedding=False, position_embedding="sinusoidal_m2m",
                    shift_mode="standard", final_logits_bias=False),
}


def _bartlike(mt, name, vocab, d_model, layers, heads, d_ff, act, max_pos, scale_emb, pad, eos, bos, start,
              dropout=0.1, attn_dropout=0.0, act_dropout=0.0, forced_bos=None, forced_eos=None, dec_layers=None,
              **extra):
    return Seq2SeqConfig(
        model_type=mt, name=name, vocab_size=vocab, d_model=d_model, d_kv=d_model // heads, d_ff=d_ff,
        num_layers=layers, num_decoder_layers=dec_layers or layers, num_heads=heads, feed_forward_proj=act, dropout_rate=dropout,
        attention_dropout=attn_dropout, activation_dropout=act_dropout, layer_norm_epsilon=1e-5,
        scale_decoder_outputs=False, max_position_embeddings=max_pos,
        scale_embedding=scale_emb, pad_token_id=pad, eos_token_id=eos, bos_token_id=bos, decoder_start_token_id=start,
        forced_bos_token_id=forced_bos, forced_eos_token_id=forced_eos,
        **{"final_logits_bias": True, **_FAMILY[mt], **extra})


def _t5(name, d_model, d_ff, layers, heads, ff="relu", tie=True, vocab=32128, d_kv=64, flavor="t5"):
    return Seq2SeqConfig(model_type="t5", t5_flavor=flavor, name=name, vocab_size=vocab, d_model=d_model, d_kv=d_kv,
                         d_ff=d_ff,
                         num_layers=layers, num_decoder_layers=layers, num_heads=heads, feed_forward_proj=ff,
                         tie_word_embeddings=tie, scale_decoder_outputs=tie)


# Public architecture hyper-parameters (SURVEY.md §2.4 "Model sizes").
PRESETS: dict[str, Seq2SeqConfig] = {
    "t5-small": _t5("t5-small", 512, 2048, 6, 8),
    "t5-base": _t5("t5-base", 768, 3072, 12, 12),
    "t5-large": _t5("t5-large", 1024, 4096, 24, 16),
    "flan-t5-small": _t5("flan-t5-small", 512, 1024, 8, 6, ff="gated-gelu", tie=False),
    "flan-t5-base": _t5("flan-t5-base", 768, 2048, 12, 12, ff="gated-gelu", tie=False),
    "flan-t5-large": _t5("flan-t5-large", 1024, 2816, 24, 16, ff="gated-gelu", tie=False),
    "flan-t5-xl": _t5("flan-t5-xl", 2048, 5120, 24, 32, ff="gated-gelu", tie=False),
    # T5 v1.1 and mT5 (multilingual: 250K SentencePiece vocabulary): the FLAN-T5 architecture
    "t5-v1_1-base": _t5("t5-v1_1-base", 768, 2048, 12, 12, ff="gated-gelu", tie=False),
    "t5-v1_1-large": _t5("t5-v1_1-large", 1024, 2816, 24, 16, ff="gated-gelu", tie=False),
    "mt5-small": _t5("mt5-small", 512, 1024, 8, 6, ff="gated-gelu", tie=False, vocab=250112, flavor="mt5"),
    "mt5-base": _t5("mt5-base", 768, 2048, 12, 12, ff="gated-gelu", tie=False, vocab=250112, flavor="mt5"),
    "mt5-large": _t5("mt5-large", 1024, 2816, 24, 16, ff="gated-gelu", tie=False, vocab=250112, flavor="mt5"),
    # UMT5: the mT5 architecture with a relative-position bias table in every self-attention layer
    "umt5-small": _t5("umt5-small", 512, 1024, 8, 6, ff="gated-gelu", tie=False, vocab=256384, flavor="umt5"),
    "umt5-base": _t5("umt5-base", 768, 2048, 12, 12, ff="gated-gelu", tie=False, vocab=256384, flavor="umt5"),
    "umt5-xl": _t5("umt5-xl", 2048, 5120, 24, 32, ff="gated-gelu", tie=False, vocab=256384, flavor="umt5"),
    # LongT5-local: the T5 v1.1 shapes, encoder self-attention windowed to local_radius = 127 (LongT5Config's default).
    # Shapes as published for google/long-t5-local-{base,large}; a checkpoint directory's config.json overrides them
    "long-t5-local-base": _t5("long-t5-local-base", 768, 2048, 12, 12, ff="gated-gelu", tie=False, flavor="longt5"),
    "long-t5-local-large": _t5("long-t5-local-large", 1024, 2816, 24, 16, ff="gated-gelu", tie=False, flavor="longt5"),
    "bart-base": Seq2SeqConfig(
        model_type="bart", name="bart-base", vocab_size=50265, d_model=768, d_kv=64, d_ff=3072, num_layers=6,
        num_decoder_layers=6, num_heads=12, feed_forward_proj="gelu", dropout_rate=0.1, attention_dropout=0.0,
        activation_dropout=0.0, layer_norm_epsilon=1e-5, final_logits_bias=True, scale_decoder_outputs=False,
        pad_token_id=1, eos_token_id=2, bos_token_id=0, decoder_start_token_id=2, forced_bos_token_id=0,
        forced_eos_token_id=2),
    "bart-large": Seq2SeqConfig(
        model_type="bart", name="bart-large", vocab_size=50265, d_model=1024, d_kv=64, d_ff=4096, num_layers=12,
        num_decoder_layers=12, num_heads=16, feed_forward_proj="gelu", dropout_rate=0.1, attention_dropout=0.0,
        activation_dropout=0.0, layer_norm_epsilon=1e-5, final_logits_bias=True, scale_decoder_outputs=False,
        pad_token_id=1, eos_token_id=2, bos_token_id=0, decoder_start_token_id=2, forced_bos_token_id=0,
        forced_eos_token_id=2),
}
# bart-large-cnn: vocab 50264 and CNN/DM generation defaults.
PRESETS["bart-large-cnn"] = PRESETS["bart-large"].replace(
    name="bart-large-cnn", vocab_size=50264,
    generation={"min_length": 56, "max_length": 142, "length_penalty": 2.0, "no_repeat_ngram_size": 3,
                "num_beams": 4, "early_stopping": True})
# other AutoModelForSeq2SeqLM families on the BART implementation (models/bart.py; public config.json values)
PRESETS["mbart-large-cc25"] = _bartlike("mbart", "mbart-large-cc25", 250027, 1024, 12, 16, 4096, "gelu", 1024, True,
                                        pad=1, eos=2, bos=0, start=2, forced_eos=2)
PRESETS["mbart-large-50"] = PRESETS["mbart-large-cc25"].replace(name="mbart-large-50", vocab_size=250054)
PRESETS["pegasus-large"] = _bartlike("pegasus", "pegasus-large", 96103, 1024, 16, 16, 4096, "relu", 1024, True,
                                     pad=0, eos=1, bos=None, start=0, attn_dropout=0.1, act_dropout=0.1, forced_eos=1)
PRESETS["pegasus-xsum"] = PRESETS["pegasus-large"].replace(
    name="pegasus-xsum", max_position_embeddings=512,
    generation={"max_length": 64, "length_penalty": 0.6, "num_beams": 8})
PRESETS["opus-mt-en-de"] = _bartlike("marian", "opus-mt-en-de", 58101, 512, 6, 8, 2048, "swish", 512, True,
                                     pad=58100, eos=0, bos=None, start=58100, forced_eos=0)
PRESETS["m2m100_418m"] = _bartlike("m2m_100", "m2m100_418m", 128112, 1024, 12, 16, 4096, "relu", 1024, True,
                                   pad=1, eos=2, bos=0, start=2, attn_dropout=0.1, forced_eos=2)
PRESETS["plbart-base"] = _bartlike("plbart", "plbart-base", 50005, 768, 6, 12, 3072, "gelu", 1024, True, pad=1, eos=2,
                                   bos=0, start=2, forced_eos=2)
PRESETS["blenderbot-400m-distill"] = _bartlike("blenderbot", "blenderbot-400m-distill", 8008, 1280, 2, 32, 5120,
                                               "gelu", 128, True, pad=0, eos=2, bos=1, start=1, forced_eos=2,
                                               dec_layers=12)
PRESETS["nllb-200-distilled-600m"] = PRESETS["m2m100_418m"].replace(name="nllb-200-distilled-600m", vocab_size=256206)
# LED (allenai/led-{base,large}-16384): the BART shapes with a 16384-position windowed encoder.  Written down without
# the published config.json at hand; a checkpoint directory's own config.json overrides them
PRESETS["led-base-16384"] = _bartlike("led", "led-base-16384", 50265, 768, 6, 12, 3072, "gelu", 1024, False, pad=1,
                                      eos=2, bos=0, start=2, attention_window=1024,
                                      max_encoder_position_embeddings=16384)
PRESETS["led-large-16384"] = _bartlike("led", "led-large-16384", 50265, 1024, 12, 16, 4096, "gelu", 1024, False, pad=1,
                                       eos=2, bos=0, start=2, attention_window=1024,
                                       max_encoder_position_embeddings=16384)
# BigBird-Pegasus (google/bigbird-pegasus-large-{arxiv,pubmed,bigpatent}): BigBirdPegasusConfig's defaults, which are
# the large checkpoints' values; a checkpoint directory's own config.json overrides them
PRESETS["bigbird-pegasus-large-arxiv"] = _bartlike(
    "bigbird_pegasus", "bigbird-pegasus-large-arxiv", 96103, 1024, 16, 16, 4096, "gelu_new", 4096, True, pad=0, eos=1,
    bos=2, start=2, attention_type="block_sparse", block_size=64, num_random_blocks=3, use_bias=False)
for _n in ("pubmed", "bigpatent"):
    PRESETS[f"bigbird-pegasus-large-{_n}"] = PRESETS["bigbird-pegasus-large-arxiv"].replace(
        name=f"bigbird-pegasus-large-{_n}")
# tiny configs for CPU tests
# block 8, 2 random blocks: block-sparse above 72 tokens, full attention up to there
PRESETS["bigbird-tiny"] = _bartlike("bigbird_pegasus", "bigbird-tiny", 512, 64, 2, 4, 128, "gelu_new", 256, True, pad=0,
                                    eos=1, bos=2, start=2, attention_type="block_sparse", block_size=8,
                                    num_random_blocks=2, use_bias=False)
# T5Gemma tiny configs for the tests: head dim 16, encoder window 4 (a 23-token input spans several), caps that bite.
# No preset for the published sizes: a checkpoint directory's own config.json is read instead
PRESETS["t5gemma-tiny"] = Seq2SeqConfig(
    model_type="t5gemma", name="t5gemma-tiny", vocab_size=512, d_model=64, d_kv=16, d_ff=128, num_layers=2,
    num_decoder_layers=2, num_heads=4, num_kv_heads=4, feed_forward_proj="gated-gelu", dropout_rate=0.0,
    attention_dropout=0.0, layer_norm_epsilon=1e-6, init_std=0.02, tie_word_embeddings=True,
    scale_decoder_outputs=False, max_position_embeddings=128, query_pre_attn_scalar=16, attn_logit_softcapping=2.0,
    final_logit_softcapping=3.0, rope_theta=10000.0, sliding_window=4, decoder_sliding_window=64,
    layer_types=["sliding_attention", "full_attention"], decoder_layer_types=["sliding_attention", "full_attention"],
    pad_token_id=0, eos_token_id=1, bos_token_id=2, decoder_start_token_id=2)
PRESETS["t5gemma-tiny-gqa"] = PRESETS["t5gemma-tiny"].replace(name="t5gemma-tiny-gqa", num_kv_heads=2)
PRESETS["t5-tiny"] = _t5("t5-tiny", 64, 128, 2, 4, vocab=512, d_kv=16)
# the policy / reference of the preference-optimisation tests and of a --dpo-beta smoke run
PRESETS["dpo-tiny"] = PRESETS["t5-tiny"].replace(name="dpo-tiny")
PRESETS["t5-tiny-gated"] = _t5("t5-tiny-gated", 64, 96, 2, 4, ff="gated-gelu", tie=False, vocab=512, d_kv=16)
PRESETS["umt5-tiny"] = _t5("umt5-tiny", 64, 96, 2, 4, ff="gated-gelu", tie=True, vocab=512, d_kv=16, flavor="umt5")
# radius 5: a 23-token input spans several windows
PRESETS["longt5-tiny"] = _t5("longt5-tiny", 64, 128, 2, 4, vocab=512, d_kv=16, flavor="longt5").replace(local_radius=5)
PRESETS["longt5-tiny-gated"] = _t5("longt5-tiny-gated", 64, 96, 2, 4, ff="gated-gelu", tie=False, vocab=512, d_kv=16,
                                   flavor="longt5").replace(local_radius=5)
# window 8 (4 keys on either side): a 23-token input spans several windows
PRESETS["led-tiny"] = _bartlike("led", "led-tiny", 512, 64, 2, 4, 128, "gelu", 64, False, pad=1, eos=2, bos=0, start=2,
                                attention_window=8, max_encoder_position_embeddings=256)
PRESETS["bart-tiny"] = PRESETS["bart-base"].replace(name="bart-tiny", vocab_size=512, d_model=64, d_kv=16, d_ff=128,
                                                    num_layers=2, num_decoder_layers=2, num_heads=4,
                                                    max_position_embeddings=256)
PRESETS["mbart-tiny"] = _bartlike("mbart", "mbart-tiny", 512, 64, 2, 4, 128, "gelu", 256, True, pad=1, eos=2, bos=0,
                                  start=2, forced_eos=2)
PRESETS["pegasus-tiny"] = _bartlike("pegasus", "pegasus-tiny", 512, 64, 2, 4, 128, "relu", 256, True, pad=0, eos=1,
                                    bos=None, start=0, attn_dropout=0.1, act_dropout=0.1, forced_eos=1)
PRESETS["m2m100-tiny"] = _bartlike("m2m_100", "m2m100-tiny", 512, 64, 2, 4, 128, "relu", 256, True, pad=1, eos=2,
                                   bos=0, start=2, attn_dropout=0.1, forced_eos=2)
PRESETS["plbart-tiny"] = _bartlike("plbart", "plbart-tiny", 512, 64, 2, 4, 128, "gelu", 256, True, pad=1, eos=2, bos=0,
                                   start=2, forced_eos=2)
PRESETS["blenderbot-tiny"] = _bartlike("blenderbot", "blenderbot-tiny", 512, 64, 1, 4, 128, "gelu", 256, True, pad=0,
                                       eos=2, bos=1, start=1, forced_eos=2, dec_layers=2)
PRESETS["marian-tiny"] = _bartlike("marian", "marian-tiny", 512, 64, 2, 4, 128, "swish", 256, True, pad=511, eos=0,
                                   bos=None, start=511, forced_eos=0)


def resolve_config(name_or_path: str) -> Seq2SeqConfig:
    """Map an HF checkpoint id (``google-t5/t5-base``, ``facebook/bart-large-cnn``) or a local
    directory with ``config.json`` to a config."""
    if name_or_path and os.path.isdir(name_or_path) and os.path.exists(os.path.join(name_or_path, "config.json")):
        with open(os.path.join(name_or_path, "config.json")) as f:
            cfg = Seq2SeqConfig.from_hf_dict(json.load(f))
        cfg.name = name_or_path
        gpath = os.path.join(name_or_path, "generation_config.json")
        if os.path.exists(gpath):
            with open(gpath) as f:
                g = json.load(f)
            keep = {"min_length", "max_length", "length_penalty", "no_repeat_ngram_size", "num_beams",
                    "early_stopping", "do_sample", "temperature", "top_k", "top_p", "repetition_penalty",
                    # not implemented: generate() names them in a warning (models/generation.py)
                    "encoder_no_repeat_ngram_size", "bad_words_ids", "num_return_sequences"}
            cfg.generation = {k: v for k, v in g.items() if k in keep}
        return cfg
    key = (name_or_path or "t5-small").split("/")[-1].lower()
    if key not in PRESETS:
        raise KeyError(f"unknown model {name_or_path!r}; presets: {sorted(PRESETS)}")
    return copy.deepcopy(PRESETS[key])
