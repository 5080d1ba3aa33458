"""T5Gemma encoder-decoder (Gemma 2 layers in both stacks), written for the fused-op library.

Behaviour follows transformers' T5GemmaForConditionalGeneration (models/t5gemma/modeling_t5gemma.py), the one
encoder-decoder family ``AutoModelForSeq2SeqLM`` gained after 2022 (``google/t5gemma-*``, ``model_type: "t5gemma"``):

* module paths mirror transformers (``model.encoder.layers.{i}.self_attn`` ...), with this project's fused layouts: one
  ``qkv_proj`` weight ``[(H + 2 H_kv) D, d]`` (q rows, then k, then v), one cross-attention ``kv_proj`` and one gated
  ``mlp.wi`` (gate rows, then up); models/hf_io.py splits and joins them to ``q_proj`` / ``k_proj`` / ``v_proj``,
  ``gate_proj`` / ``up_proj`` / ``down_proj``.  The two stacks own an embedding matrix each; the LM head is tied to the
  decoder's (``lm_head.out_proj.weight``) unless ``tie_word_embeddings`` is off;
* embeddings are multiplied by ``hidden_size ** 0.5`` rounded to the model dtype first (as transformers' tensor
  ``normalizer``), then dropped out;
* every sub-layer is a sandwich ``h + drop(post_norm(f(pre_norm(h))))``.  RMSNorm scales by ``1 + w`` in fp32 with ``w``
  stored zero-centred (ops/norms.py ``offset=1.0``).  The post-norm is a plain ``rms_norm``; the residual + dropout +
  NEXT pre-norm is the fused ``add_dropout_rms_norm``, so the residual stream is read and written once per sub-layer;
* self-attention: rotate-half RoPE on q and k (ops/rope.py, csrc/rope.hip: fp32 arithmetic, one rounding), scores
  ``cap * tanh(q.k * query_pre_attn_scalar**-0.5 / cap)`` (ops/attention.py ``softcap``; csrc/attn_hd.hip /
  csrc/attn_f32.hip).  Encoder ``sliding_attention`` layers see the keys with ``|i - j| <= sliding_window`` — exactly
  the kernels' ``window`` — and ``full_attention`` layers everything; the decoder is causal, and its sliding layers
  (``j > i - sliding_window``) are plain causal calls while the decoder length stays within ``decoder_sliding_window``
  (longer raises: the kernels have no causal window).  Cross-attention: the same cap, no RoPE, encoder key padding;
* grouped K/V heads (``num_kv_heads < num_heads``): query head ``h`` reads K/V head ``h // (H / H_kv)``; the model
  materialises the repeat (``repeat_interleave`` over the head axis) and autograd sums it back — not a kernel feature;
* default masks, as transformers: without ``attention_mask`` the encoder masks the keys whose id is the pad id (and
  cross-attention then masks nothing); without a decoder mask and without a cache the decoder masks the keys whose
  INPUT id is the pad id, which after ``shift_right`` includes the ``-100`` labels.  transformers' decoder makes
  itself a cache whenever it is not in training mode (``use_cache`` defaults to true), so that default is a
  training-mode one there, and it is here: ``decode`` applies it only while ``self.training``;
* logits ``cap_f * tanh(x / cap_f)`` and plain mean CE: in training the cap lives in the CE kernels' pass
  (ops/cross_entropy.py / ops/lm_head.py ``softcap``); ``lm_logits`` (generation) applies it in torch to the step's
  ``[rows, V]`` logits.

Not implemented, each raising ``NotImplementedError`` that names T5Gemma: LoRA, a teacher (distillation), preference
optimisation, packed inputs and context parallelism; unbalanced encoder / decoder sizes (9b-2b) are refused by the
config.  Head dims outside 32 .. 128 (the tiny test configs' 16, the 2b / 9b checkpoints' 256) run attention on the
composite with its one-time warning.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..ops import activations, attention as attn_ops, norms
from ..ops.cross_entropy import cross_entropy
from ..ops.embedding import embedding
from ..ops.ffn import gated_ffn
from ..ops.linear import Linear, linear
from ..ops.lm_head import lm_head_loss, wants_lm_head_loss
from ..ops.rng import default_rng
from ..ops.rope import rope, rope_table
from .blocks import run_block
from .config import Seq2SeqConfig
from .output import Seq2SeqLMOutput

_OFF = 1.0  # RMSNorm scales by 1 + w


def _unsupported(what: str):
    return NotImplementedError(f"T5Gemma: {what} is not implemented")


class T5GemmaRMSNorm(nn.Module):
    def __init__(self, d, eps):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(d))
        self.eps = eps


class T5GemmaAttention(nn.Module):
    def __init__(self, cfg: Seq2SeqConfig, cross: bool, window: int | None = None):
        super().__init__()
        self.cross = cross
        self.window = window  # encoder sliding_attention layers: keys within this distance only
        self.n_heads, self.n_kv, self.d_kv = cfg.num_heads, cfg.num_kv_heads, cfg.d_kv
        self.scale = float(cfg.query_pre_attn_scalar) ** -0.5
        self.softcap = cfg.attn_logit_softcapping
        H, K, D = self.n_heads, self.n_kv, self.d_kv
        if cross:
            self.q_proj = Linear(cfg.d_model, H * D, bias=False)
            self.kv_proj = Linear(cfg.d_model, 2 * K * D, bias=False)
        else:
            self.qkv_proj = Linear(cfg.d_model, (H + 2 * K) * D, bias=False)
        self.o_proj = Linear(H * D, cfg.d_model, bias=False)

    def project_kv(self, kv_in):
        B, S, _ = kv_in.shape
        return self.kv_proj(kv_in).view(B, S, 2, self.n_kv, self.d_kv)

    def _rep(self, t):
        """K or V ``[B, S, H_kv, D]`` with every head repeated for the query heads it serves."""
        return t if self.n_kv == self.n_heads else t.repeat_interleave(self.n_heads // self.n_kv, 2)

    def forward(self, x, kv_in=None, mask=None, causal=False, p=0.0, cache=None, kv=None, rot=None):
        B, S, _ = x.shape
        H, K, D = self.n_heads, self.n_kv, self.d_kv
        seed = default_rng().next_seed() if p > 0 else 0
        kw = dict(scale=self.scale, causal=causal, key_padding_mask=mask, dropout_p=p, seed=seed, softcap=self.softcap)
        if self.cross:
            q = self.q_proj(x).view(B, S, H, D)
            kv = kv if kv is not None else self.project_kv(kv_in)
            if kv.shape[0] != B:  # beam search: the nb hypotheses of a batch entry share its encoder K/V (read once)
                q = q.reshape(kv.shape[0], (B // kv.shape[0]) * S, H, D)
            if K == H:
                o = attn_ops.attention_q_kv(q, kv, **kw)
            else:
                o = attn_ops.attention(q, self._rep(kv[:, :, 0]), self._rep(kv[:, :, 1]), **kw)
            return self.o_proj(o.reshape(B, S, H * D))
        pos, cos, sin = rot
        if self.window is not None:
            kw["window"] = self.window
        qkv = self.qkv_proj(x)
        if K == H and cache is None:
            packed = rope(qkv.view(B, S, 3, H, D), pos, cos, sin, slots=2)
            o = attn_ops.attention_qkv(packed, **kw)
        else:
            # q and k heads side by side as one slot of H + K heads: one rotation for both, v left where it is
            qk = rope(qkv[..., :(H + K) * D].view(B, S, 1, H + K, D), pos, cos, sin)
            q, k = qk[:, :, 0, :H], qk[:, :, 0, H:]
            v = qkv[..., (H + K) * D:].view(B, S, K, D)
            if cache is not None:
                k, v = cache.append(k, v)
            o = attn_ops.attention(q, self._rep(k), self._rep(v), **kw)
        return self.o_proj(o.reshape(B, S, H * D))


class T5GemmaMLP(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.wi = Linear(cfg.d_model, 2 * cfg.d_ff, bias=False)  # gate rows, then up rows
        self.wo = Linear(cfg.d_ff, cfg.d_model, bias=False)
        self.act = cfg.act

    def forward(self, x, p):
        seed = default_rng().next_seed() if p > 0 else 0
        return gated_ffn(x, self.wi, self.wo, self.act, p, seed)


class T5GemmaLayer(nn.Module):
    def __init__(self, cfg: Seq2SeqConfig, i: int, is_decoder: bool):
        super().__init__()
        d, eps = cfg.d_model, cfg.layer_norm_epsilon
        sliding = (cfg.decoder_layer_types if is_decoder else cfg.layer_types)[i] == "sliding_attention"
        self.sliding = sliding
        self.self_attn = T5GemmaAttention(cfg, cross=False,
                                          window=cfg.sliding_window if sliding and not is_decoder else None)
        self.pre_self_attn_layernorm = T5GemmaRMSNorm(d, eps)
        self.post_self_attn_layernorm = T5GemmaRMSNorm(d, eps)
        if is_decoder:
            self.cross_attn = T5GemmaAttention(cfg, cross=True)
            self.pre_cross_attn_layernorm = T5GemmaRMSNorm(d, eps)
            self.post_cross_attn_layernorm = T5GemmaRMSNorm(d, eps)
        self.mlp = T5GemmaMLP(cfg)
        self.pre_feedforward_layernorm = T5GemmaRMSNorm(d, eps)
        self.post_feedforward_layernorm = T5GemmaRMSNorm(d, eps)


class T5GemmaStack(nn.Module):
    def __init__(self, cfg: Seq2SeqConfig, is_decoder: bool):
        super().__init__()
        self.cfg = cfg
        self.is_decoder = is_decoder
        self.embed_tokens = nn.Embedding(cfg.vocab_size, cfg.d_model, padding_idx=cfg.pad_token_id)
        n = cfg.num_decoder_layers if is_decoder else cfg.num_layers
        self.layers = nn.ModuleList([T5GemmaLayer(cfg, i, is_decoder) for i in range(n)])
        self.norm = T5GemmaRMSNorm(cfg.d_model, cfg.layer_norm_epsilon)

    @property
    def max_positions(self) -> int:
        return self.cfg.decoder_max_position_embeddings if self.is_decoder else self.cfg.max_position_embeddings

    def _rot(self, B, S, offset, position_ids, device):
        """(positions, cos, sin) of this call: ``position_ids`` [B, S] or arange(S) + offset."""
        cfg = self.cfg
        need = S + offset
        if position_ids is not None:
            if position_ids.dim() == 1:
                position_ids = position_ids[None].expand(B, -1)
            need = max(need, int(position_ids.max()) + 1)
            pos = position_ids.to(device=device, dtype=torch.int32).contiguous()
        else:
            pos = torch.arange(offset, offset + S, device=device, dtype=torch.int32)
        # max_positions rows, or the next multiple of it that holds the call: few distinct tables however far a
        # generation runs past the limit
        n = -(-need // self.max_positions) * self.max_positions
        cos, sin = rope_table(cfg.rope_theta, cfg.d_kv, n, device)
        self._rope = getattr(self, "_rope", {})
        self._rope[(n, str(device))] = (cos, sin)  # held here too: a captured step reads them by address
        return pos, cos, sin

    def forward(self, input_ids, attention_mask=None, enc_out=None, enc_mask=None, caches=None, q_offset=0,
                cross_kv=None, position_ids=None):
        cfg = self.cfg
        p = cfg.dropout_rate if self.training else 0.0
        pa = cfg.attention_dropout if self.training else 0.0
        eps = cfg.layer_norm_epsilon
        rng = default_rng()
        B, S = input_ids.shape
        if self.is_decoder and cfg.decoder_sliding_window is not None and S + q_offset > cfg.decoder_sliding_window \
                and any(lyr.sliding for lyr in self.layers):
            raise NotImplementedError(
                f"T5Gemma: a decoder length of {S + q_offset} exceeds decoder.sliding_window = "
                f"{cfg.decoder_sliding_window}; the attention kernels have no causal window")
        x = embedding(input_ids, self.embed_tokens.weight, self.embed_tokens.padding_idx)
        # transformers multiplies by a tensor of the activation dtype: hidden_size ** 0.5 rounded to it
        x = x * float(torch.tensor(cfg.d_model ** 0.5, dtype=x.dtype))
        rot = self._rot(B, S, q_offset, position_ids, x.device)
        layers = list(self.layers)
        normed, h = norms.dropout_rms_norm(x, layers[0].pre_self_attn_layernorm.weight, eps, p,
                                           rng.next_seed() if p > 0 else 0, offset=_OFF)
        for i, lyr in enumerate(layers):
            nxt = layers[i + 1].pre_self_attn_layernorm.weight if i + 1 < len(layers) else self.norm.weight
            ckv = cross_kv[i] if cross_kv is not None else None
            cache = caches[i] if caches is not None else None

            def run(normed, h, lyr=lyr, nxt=nxt, ckv=ckv, cache=cache):
                return self._layer(lyr, nxt, normed, h, attention_mask, enc_out, enc_mask, ckv, cache, p, pa, eps, rot)

            normed, h = run_block(run, normed, h, checkpoint=cfg.gradient_checkpointing and self.training and
                                  caches is None)
        # `normed` is now norm(h); transformers applies dropout after it
        return activations.dropout(normed, p, rng.next_seed() if p > 0 else 0)

    def _layer(self, lyr, next_norm, normed, h, mask, enc_out, enc_mask, ckv, cache, p, pa, eps, rot):
        """One layer on (pre_norm(h), h) -> (next pre_norm(h'), h'): every sub-layer's output goes through its
        post-norm, then the residual update fused with the following pre-norm."""
        rng = default_rng()

        def seed():
            return rng.next_seed() if p > 0 else 0

        a = lyr.self_attn(normed, mask=mask, causal=self.is_decoder, p=pa, cache=cache, rot=rot)
        a = norms.rms_norm(a, lyr.post_self_attn_layernorm.weight, eps, offset=_OFF)
        if self.is_decoder:
            normed, h = norms.add_dropout_rms_norm(h, a, lyr.pre_cross_attn_layernorm.weight, eps, p, seed(),
                                                   offset=_OFF)
            c = lyr.cross_attn(normed, kv_in=enc_out, mask=enc_mask, p=pa, kv=ckv)
            a = norms.rms_norm(c, lyr.post_cross_attn_layernorm.weight, eps, offset=_OFF)
        normed, h = norms.add_dropout_rms_norm(h, a, lyr.pre_feedforward_layernorm.weight, eps, p, seed(), offset=_OFF)
        f = lyr.mlp(normed, p)
        f = norms.rms_norm(f, lyr.post_feedforward_layernorm.weight, eps, offset=_OFF)
        return norms.add_dropout_rms_norm(h, f, next_norm, eps, p, seed(), offset=_OFF)


class _Stacks(nn.Module):
    """transformers' ``model`` level: the two stacks."""

    def __init__(self, cfg):
        super().__init__()
        self.encoder = T5GemmaStack(cfg, False)
        self.decoder = T5GemmaStack(cfg, True)


class _LMHead(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.out_proj = Linear(cfg.d_model, cfg.vocab_size, bias=False)


class T5GemmaForConditionalGeneration(nn.Module):
    model_type = "t5gemma"

    def __init__(self, cfg: Seq2SeqConfig):
        super().__init__()
        self.config = cfg
        self.model = _Stacks(cfg)
        if not cfg.tie_word_embeddings:
            self.lm_head = _LMHead(cfg)
        self.reset_parameters()

    @property
    def encoder(self) -> T5GemmaStack:
        return self.model.encoder

    @property
    def decoder(self) -> T5GemmaStack:
        return self.model.decoder

    # ---------------------------------------------------------------------------------- init
    @torch.no_grad()
    def reset_parameters(self):
        """transformers' T5GemmaPreTrainedModel._init_weights: normal(0, initializer_range) for every projection and
        embedding (the padding row zero), zeros for the zero-centred norm weights; an untied LM head is scaled by
        ``vocab_size ** -0.5``."""
        std = self.config.init_std
        for m in self.modules():
            if isinstance(m, Linear):
                m.weight.normal_(0.0, std)
            elif isinstance(m, nn.Embedding):
                m.weight.normal_(0.0, std)
                if m.padding_idx is not None:
                    m.weight[m.padding_idx].zero_()
            elif isinstance(m, T5GemmaRMSNorm):
                m.weight.zero_()
        if not self.config.tie_word_embeddings:
            self.lm_head.out_proj.weight.normal_(0.0, std * self.config.vocab_size ** -0.5)

    # ---------------------------------------------------------------------------------- API
    def shift_right(self, labels):
        """modeling_t5gemma.py _shift_right: start with decoder.bos_token_id, -100 becomes the pad id."""
        out = labels.new_zeros(labels.shape)
        out[..., 1:] = labels[..., :-1]
        out[..., 0] = self.config.decoder_start_token_id
        out.masked_fill_(out == -100, self.config.pad_token_id)
        return out

    prepare_decoder_input_ids_from_labels = shift_right

    def encode(self, input_ids, attention_mask=None, position_ids=None):
        if attention_mask is None:  # transformers' make_default_2d_attention_mask
            attention_mask = input_ids != self.config.pad_token_id
        return self.encoder(input_ids, attention_mask=attention_mask, position_ids=position_ids)

    def decode(self, decoder_input_ids, enc_out, enc_mask=None, caches=None, q_offset=0, cross_kv=None,
               decoder_attention_mask=None, position_ids=None):
        # the same default on the decoder's input ids — where transformers has no cache: in training mode only
        if decoder_attention_mask is None and caches is None and self.training:
            decoder_attention_mask = decoder_input_ids != self.config.pad_token_id
        return self.decoder(decoder_input_ids, attention_mask=decoder_attention_mask, enc_out=enc_out,
                            enc_mask=enc_mask, caches=caches, q_offset=q_offset, cross_kv=cross_kv,
                            position_ids=position_ids)

    def output_embedding(self):
        return self.decoder.embed_tokens.weight if self.config.tie_word_embeddings else self.lm_head.out_proj.weight

    def _cap(self, logits):
        c = self.config.final_logit_softcapping
        return logits if c is None else (c * torch.tanh(logits.float() / c)).to(logits.dtype)

    def lm_logits(self, hidden):
        """The capped logits (generation: the step's ``[rows, V]`` rows, capped in torch)."""
        return self._cap(linear(hidden, self.output_embedding()))

    def logits_bias(self):
        return None

    def cross_attention_modules(self):
        return [lyr.cross_attn for lyr in self.decoder.layers]

    def project_cross_kv(self, enc_out):
        return [m.project_kv(enc_out) for m in self.cross_attention_modules()]

    def generate(self, input_ids, attention_mask=None, **kw):
        from .generation import generate
        cfg = self.config
        L = kw.get("max_length")
        L = L if L is not None else cfg.generation.get("max_length", 20)
        if kw.get("max_new_tokens") is not None:
            L = kw["max_new_tokens"] + 1
        if cfg.decoder_sliding_window is not None and L > cfg.decoder_sliding_window and \
                any(lyr.sliding for lyr in self.decoder.layers):
            raise NotImplementedError(
                f"T5Gemma: max_length = {L} exceeds decoder.sliding_window = {cfg.decoder_sliding_window}; the "
                "attention kernels have no causal window")
        return generate(self, input_ids, attention_mask=attention_mask, **kw)

    def gradient_checkpointing_enable(self, enable: bool = True):
        self.config.gradient_checkpointing = bool(enable)
        for st in (self.encoder, self.decoder):
            st.cfg = self.config

    def enable_context_parallel(self, group=None, enable: bool = True):
        if enable:
            raise _unsupported("context parallelism (--context-parallel: ring attention has neither RoPE offsets nor "
                               "a soft cap)")
        return self

    def lm_head_operands(self, *a, **kw):
        raise _unsupported("a teacher or a student of distillation (--teacher-ckpt: the distillation loss has no "
                           "logit soft cap)")

    def forward(self, input_ids=None, attention_mask=None, decoder_input_ids=None, labels=None,
                label_smoothing: float = 0.0, return_logits: bool = False, encoder_outputs=None, segment_ids=None,
                decoder_segment_ids=None, position_ids=None, decoder_position_ids=None, distill=None,
                preference=None, decoder_attention_mask=None):
        if distill is not None:
            raise _unsupported("distillation (--teacher-ckpt: the distillation loss has no logit soft cap)")
        if preference is not None:
            raise _unsupported("preference optimisation (--dpo-beta: the sequence log-prob kernels have no logit soft "
                               "cap)")
        if segment_ids is not None or decoder_segment_ids is not None:
            raise _unsupported("packed inputs (--pack-sequences, segment ids: the kernels have no soft cap with "
                               "segments)")
        enc = encoder_outputs if encoder_outputs is not None else self.encode(input_ids, attention_mask, position_ids)
        if decoder_input_ids is None:
            decoder_input_ids = self.shift_right(labels)
        # cross-attention masks what the caller masked: nothing without an attention_mask (as transformers)
        dec = self.decode(decoder_input_ids, enc, attention_mask, decoder_attention_mask=decoder_attention_mask,
                          position_ids=decoder_position_ids)
        return self._lm_output(dec, enc, labels, label_smoothing, return_logits)

    def _lm_output(self, dec, enc, labels, label_smoothing, return_logits):
        cap = self.config.final_logit_softcapping
        if labels is not None and not return_logits and wants_lm_head_loss(dec, labels.numel(), self.config.vocab_size):
            # LM head + capped CE without materialised logits (ops/lm_head.py: vocabulary chunks with a cap)
            loss = lm_head_loss(dec, self.output_embedding(), labels, label_smoothing=label_smoothing, softcap=cap)
            return Seq2SeqLMOutput(loss=loss, logits=None, encoder_last_hidden_state=enc)
        logits = linear(dec, self.output_embedding())  # uncapped: the CE kernels cap in their pass
        want = return_logits or labels is None
        out = self._cap(logits) if want else None
        loss = None
        if labels is not None:
            V = logits.shape[-1]
            loss = cross_entropy(logits.view(-1, V), labels.reshape(-1), label_smoothing=label_smoothing,
                                 inplace_grad=not return_logits, softcap=cap)
        return Seq2SeqLMOutput(loss=loss, logits=out, encoder_last_hidden_state=enc)
