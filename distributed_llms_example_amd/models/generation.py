"""Autoregressive generation for the seq2seq models: greedy and beam search with a KV cache.

The reference evaluates with ``unwrap_model(model).generate(input_ids, attention_mask=...,
max_length=128, num_beams=2)`` (ref/train-accelerator.py:239-249, ref/train-task.py:310-313), i.e.
transformers' GenerationMixin beam search (generation/utils.py:3208): encode once, expand to
``batch × num_beams``, per step fp32 ``log_softmax`` + logits processors, top-``2·num_beams``
candidates over ``num_beams × V``, finished hypotheses scored ``sum_logprobs / len**length_penalty``,
``early_stopping`` rules, cache reordering.  Processors implemented: ``min_length``,
``no_repeat_ngram_size``, ``forced_bos_token_id``, ``forced_eos_token_id`` (bart-large-cnn's
generation_config uses all of them).

MI355X specifics: the decoder self-attention cache is preallocated ``[B, max_len, H, D]`` (no
per-step concatenation; the attention kernel reads the strided prefix view), cross-attention K/V are
projected once per generate call, and every decode step runs the same fused kernels as training
(attention with the bias LUT offset by the cache length).
"""
from __future__ import annotations


import torch

from ..ops import routing
from ..ops.attention import relative_bias_lut  # noqa: F401  (documented dependency)


class KVStore:
    """Self-attention K/V of EVERY decoder layer in one preallocated buffer [layers * 2, rows, max_len, H * D].

    A beam reorder is ONE in-place kernel over all layers on the GPU (csrc/beam.hip ``kv_reorder``): a batch entry
    whose hypotheses all kept their own row moves no bytes, and otherwise only the rows that change are written (the
    group's source rows are read first).  That replaces an index_select + copy-back per layer and tensor (48 launches
    and two full passes over the live prefix for a 12-layer decoder)."""

    def __init__(self, layers: int, batch: int, max_len: int, heads: int, dim: int, dtype, device, nb: int = 1):
        self.buf = torch.empty(layers * 2, batch, max_len, heads * dim, dtype=dtype, device=device)
        self.heads, self.dim, self.nb = heads, dim, nb
        self.len = 0
        self.layers = [KVCache(self, i) for i in range(layers)]

    def reorder(self, idx):
        n = self.len
        if not n:
            return
        from .. import _ext
        hd = self.heads * self.dim
        if (self.buf.dtype == torch.bfloat16 and _ext.use_native(self.buf) and self.nb * hd // 8 <= 512
                and hd % 8 == 0):
            _ext.native().kv_reorder(self.buf, idx.contiguous(), self.nb, n)
            return
        live = self.buf[:, :, :n]
        live.copy_(live.index_select(1, idx))


class KVCache:
    """Layer ``i``'s view of a KVStore (the interface the attention modules use: append, then read the prefix)."""

    def __init__(self, store: KVStore, i: int):
        self.store = store
        self.i = i

    @property
    def len(self):
        return self.store.len

    def append(self, k, v):
        st = self.store
        s = k.shape[1]
        last = self.i == len(st.layers) - 1
        kb = st.buf[2 * self.i].view(-1, st.buf.shape[2], st.heads, st.dim)
        vb = st.buf[2 * self.i + 1].view(-1, st.buf.shape[2], st.heads, st.dim)
        kb[:, st.len:st.len + s] = k
        vb[:, st.len:st.len + s] = v
        n = st.len + s
        if last:  # the last layer of the step advances the shared length
            st.len = n
        return kb[:, :n], vb[:, :n]


def _head_geom(model):
    cfg = model.config
    if cfg.model_type == "t5":
        return cfg.num_heads, cfg.d_kv
    if cfg.model_type == "t5gemma":  # the cache holds the K/V heads; the model repeats them for the query heads
        return cfg.num_kv_heads, cfg.d_kv
    return cfg.num_heads, cfg.d_model // cfg.num_heads


def _ban_ngrams(logp, seqs, cur_len: int, n: int):
    """no_repeat_ngram_size on the device: every earlier n-gram whose first n-1 tokens equal the last n-1 generated
    tokens bans its n-th token (transformers NoRepeatNGramLogitsProcessor), without a host round trip."""
    if n <= 0 or cur_len < n:  # no complete earlier n-gram yet
        return logp
    prev = seqs[:, :cur_len]
    if n == 1:
        return logp.scatter_(1, prev, float("-inf"))
    wins = prev.unfold(1, n, 1)  # [N, cur_len - n + 1, n]
    match = (wins[:, :, :n - 1] == prev[:, cur_len - n + 1:cur_len].unsqueeze(1)).all(-1)
    tok = wins[:, :, n - 1]
    vals = torch.where(match, torch.full_like(tok, 0, dtype=logp.dtype) - float("inf"),
                       torch.full_like(tok, 0, dtype=logp.dtype) + float("inf"))
    return logp.scatter_reduce_(1, tok, vals, reduce="amin", include_self=True)


def _apply_processors_device(logp, seqs, cur_len, min_length, no_repeat_ngram_size, forced_bos, forced_eos,
                             max_length, eos):
    """transformers' processor order: NoRepeatNGram and MinLength, then ForcedBOS / ForcedEOS (a forced token wins
    over a ban)."""
    if min_length is not None and cur_len < min_length and eos is not None:
        logp[:, eos] = -float("inf")
    logp = _ban_ngrams(logp, seqs, cur_len, no_repeat_ngram_size or 0)
    if forced_bos is not None and cur_len == 1:
        logp.fill_(-float("inf"))
        logp[:, forced_bos] = 0.0
    if forced_eos is not None and cur_len == max_length - 1:
        logp.fill_(-float("inf"))
        logp[:, forced_eos] = 0.0
    return logp


def _penalize(scores, seqs, cur_len: int, penalty: float):
    """transformers' RepetitionPenaltyLogitsProcessor: every token id in the row's decoder prefix ``seqs[row, :cur]``
    (start token included) has its score multiplied by ``penalty`` when negative and divided by it otherwise."""
    if penalty == 1.0:
        return scores
    prev = seqs[:, :cur_len]
    s = scores.gather(1, prev)
    r = torch.full((), penalty, dtype=scores.dtype, device=scores.device)  # a tensor: a true division on every device
    return scores.scatter(1, prev, torch.where(s < 0, s * r, s / r))


def _warp(scores, temperature: float, top_k: int, top_p: float):
    """Temperature, top-k, top-p on fp32 scores [N, V] (transformers' warpers, in their order); removed tokens become
    -inf.  Top-k keeps every tie with the k-th largest value.  Top-p is stated by value: on the softmax of the top-k
    survivors a token is kept iff the probability mass of the tokens with a STRICTLY larger score is < ``top_p``, so
    tied scores are kept or dropped together and the maximum always stays (TopPLogitsWarper wherever the scores at
    the boundary are distinct)."""
    V = scores.shape[-1]
    ninf = float("-inf")
    if temperature != 1.0:  # divided by a tensor: torch turns a division by a Python scalar into a multiplication
        scores = scores / torch.full((), temperature, dtype=scores.dtype, device=scores.device)
    if 0 < top_k < V:
        kth = scores.topk(top_k, dim=-1).values[:, -1:]
        scores = scores.masked_fill(scores < kth, ninf)
    if top_p < 1.0:
        srt = scores.sort(dim=-1, descending=True).values
        cum = srt.softmax(dim=-1).cumsum(dim=-1)
        excl = torch.cat([torch.zeros_like(cum[:, :1]), cum[:, :-1]], 1)  # mass at earlier sort positions
        first = torch.ones_like(srt, dtype=torch.bool)  # first position of each run of equal scores
        first[:, 1:] = srt[:, 1:] != srt[:, :-1]
        above = torch.where(first, excl, torch.zeros_like(excl)).cummax(dim=-1).values  # mass of strictly larger scores
        keep = above < top_p
        keep[:, 0] = True
        thr = srt.gather(1, keep.sum(-1, keepdim=True) - 1)
        scores = scores.masked_fill(scores < thr, ninf)
    return scores


def _sample_scores(logits, seqs, cur, proc, penalty, temperature, top_k, top_p):
    """The scores one sampling step draws from (torch composite): fp32 logits -> repetition penalty -> n-gram /
    min-length bans and forced tokens -> temperature, top-k, top-p.  -inf marks a removed token."""
    min_length, ngram, forced_bos, forced_eos, max_length, eos = proc
    x = _penalize(logits.float(), seqs, cur, penalty)
    if x.data_ptr() == logits.data_ptr():
        x = x.clone()  # the processors write in place
    x = _apply_processors_device(x, seqs, cur, min_length, ngram, forced_bos, forced_eos, max_length, eos)
    return _warp(x, temperature, top_k, top_p)


def _gumbel_argmax(scores, seed: int, step: int):
    """Gumbel-max draw over the kept tokens: argmax of ``x - log(-log u)`` with the counter-based uniforms of
    ops/rng.py ``sample_uniform`` (fp64; ties resolve to the lower index)."""
    from ..ops import rng
    N, V = scores.shape
    dev = scores.device
    u = rng.sample_uniform(seed, step, N, torch.arange(N, device=dev).view(N, 1),
                           torch.arange(V, device=dev).view(1, V))
    return (scores.double() - torch.log(-torch.log(u))).argmax(-1)


def _fused_sample_ok(logits) -> bool:
    from .. import _ext
    return (bool(routing.get("gen_fused_sample")) and logits.dim() == 2
            and logits.dtype in (torch.bfloat16, torch.float32) and _ext.use_native(logits))


def _sample_step(logits, seqs, cur, proc, penalty, temperature, top_k, top_p, seed, step):
    """One sampling step: the token per row, int64 [N].  On the GPU one csrc/sample.hip launch (penalty, bans, forced
    token, temperature, top-k and top-p thresholds by radix select, Gumbel-max draw); otherwise, and for arguments the
    kernel does not take, the torch composite of the same ops."""
    if _fused_sample_ok(logits):
        from .. import _ext
        min_length, ngram, forced_bos, forced_eos, max_length, eos = proc
        ban = eos if (min_length is not None and cur < min_length and eos is not None) else -1
        force = -1
        if forced_bos is not None and cur == 1:
            force = forced_bos
        if forced_eos is not None and cur == max_length - 1:
            force = forced_eos
        rc, tok, _thr = _ext.native().sample_step(logits, seqs, cur, ngram or 0, ban, force, float(penalty),
                                                  float(temperature), int(top_k), float(top_p), int(seed), int(step))
        if rc == 0:
            return tok
        if rc != -4:
            raise RuntimeError(f"sample_step failed: rc={rc}")
    return _gumbel_argmax(_sample_scores(logits, seqs, cur, proc, penalty, temperature, top_k, top_p), seed, step)


def _fused_beam_ok(logits, nb: int, penalty: float = 1.0) -> bool:
    from .. import _ext
    return (bool(routing.get("gen_fused_beam")) and penalty == 1.0 and nb <= 8 and 2 * nb <= 16 and logits.dim() == 2
            and logits.dtype in (torch.bfloat16, torch.float32) and _ext.use_native(logits))


def _beam_candidates(logits, beam_scores, seqs, cur, B, nb, proc, penalty: float = 1.0):
    """Top-2·nb candidates over nb·V per batch entry: (scores [B, 2nb], flat indices beam·V + token).  On the GPU one
    csrc/beam.hip launch (log_softmax normaliser + processors + beam score + top-k in one pass over the logits);
    otherwise, and for arguments the kernel does not take, the torch composite of the same ops.  A repetition penalty
    acts on the log-probabilities, before the bans (transformers' beam search), on the torch path only."""
    min_length, ngram, forced_bos, forced_eos, max_length, eos = proc
    if _fused_beam_ok(logits, nb, penalty):
        from .. import _ext
        ban = eos if (min_length is not None and cur < min_length and eos is not None) else -1
        force = -1
        if forced_bos is not None and cur == 1:
            force = forced_bos
        if forced_eos is not None and cur == max_length - 1:
            force = forced_eos
        rc, top_s, top_i = _ext.native().beam_topk(logits.contiguous(), beam_scores.reshape(-1).float().contiguous(),
                                                   seqs, cur, ngram or 0, ban, force, nb, 2 * nb)
        if rc == 0:
            return top_s, top_i
        if rc != -4:  # -4: arguments the kernel does not take (a vocabulary past its LDS bitmap): the composite below
            raise RuntimeError(f"beam_topk failed: rc={rc}")
    logp = _penalize(torch.log_softmax(logits.float(), dim=-1), seqs, cur, penalty)
    logp = _apply_processors_device(logp, seqs, cur, min_length, ngram, forced_bos, forced_eos, max_length, eos)
    V = logp.shape[-1]
    return (beam_scores.view(-1, 1) + logp).view(B, nb * V).topk(2 * nb, dim=1)


def _apply_processors(logp, seqs, cur_len, cfg, min_length, no_repeat_ngram_size, forced_bos, forced_eos,
                      max_length, eos):
    V = logp.shape[-1]
    if min_length is not None and cur_len < min_length and eos is not None:
        logp[:, eos] = -float("inf")
    n = no_repeat_ngram_size or 0
    if n > 0 and cur_len + 1 >= n:  # bans before the forced tokens (transformers' order: a forced token wins)
        rows = seqs.tolist()
        for b, row in enumerate(rows):
            prefix = tuple(row[cur_len - n + 1:cur_len]) if n > 1 else ()
            banned = set()
            for i in range(cur_len - n + 1):
                if tuple(row[i:i + n - 1]) == prefix:
                    banned.add(row[i + n - 1])
            if banned:
                logp[b, [t for t in banned if t < V]] = -float("inf")
    if forced_bos is not None and cur_len == 1:
        logp[:] = -float("inf")
        logp[:, forced_bos] = 0.0
    if forced_eos is not None and cur_len == max_length - 1:
        logp[:] = -float("inf")
        logp[:, forced_eos] = 0.0
    return logp


def _beam_search_device(model, seqs, enc, attention_mask, caches, cross, B, nb, max_length, proc, eos, pad,
                        length_penalty, early_stopping, check_every, penalty: float = 1.0):
    """Beam search with all bookkeeping on the device (transformers BeamSearchScorer semantics): top-2·nb candidates
    over nb·V, eos candidates ranked < nb scored ``sum_logprobs / len**length_penalty`` into a per-batch top-nb of
    finished hypotheses, the first nb non-eos candidates become the next beams, ``is_done`` per batch; the host only
    looks at ``done.all()`` every ``check_every`` steps and at the final length."""
    dev = seqs.device
    L = max_length
    inf = float("inf")
    beam_scores = torch.zeros(B, nb, device=dev)
    beam_scores[:, 1:] = -1e9
    fin_scores = torch.full((B, nb), -inf, device=dev)
    fin_seqs = torch.full((B, nb, L), pad, dtype=torch.long, device=dev)
    fin_len = torch.zeros(B, nb, dtype=torch.long, device=dev)
    fin_cnt = torch.zeros(B, dtype=torch.long, device=dev)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    base = torch.arange(B, device=dev).unsqueeze(1) * nb
    rank = torch.arange(2 * nb, device=dev).unsqueeze(0)

    def add_finished(scores, cand_seqs, cand_len):
        nonlocal fin_scores, fin_seqs, fin_len
        all_s = torch.cat([fin_scores, scores], 1)
        keep_s, keep_i = all_s.topk(nb, dim=1)
        all_seq = torch.cat([fin_seqs, cand_seqs], 1)
        fin_seqs = all_seq.gather(1, keep_i.unsqueeze(-1).expand(-1, -1, L))
        fin_len = torch.cat([fin_len, cand_len], 1).gather(1, keep_i)
        fin_scores = keep_s

    cur = 1
    while cur < max_length:
        h = model.decode(seqs[:, cur - 1:cur], enc, attention_mask, caches=caches, q_offset=cur - 1, cross_kv=cross)
        logits = model.lm_logits(h[:, -1])
        V = logits.shape[-1]
        top_s, top_i = _beam_candidates(logits, beam_scores, seqs, cur, B, nb, proc, penalty)
        src = base + top_i // V
        tok = top_i % V
        is_eos = tok == eos if eos is not None else torch.zeros_like(tok, dtype=torch.bool)
        # finished hypotheses: eos candidates among the top nb of a live batch
        add = is_eos & (rank < nb) & ~done.unsqueeze(1)
        if eos is not None:
            sc = torch.where(add, top_s / (max(cur, 1) ** length_penalty), torch.full_like(top_s, -inf))
            cand = seqs.index_select(0, src.reshape(-1)).view(B, 2 * nb, L)
            cand[:, :, cur] = tok
            add_finished(sc, cand, torch.full_like(tok, cur + 1))
            fin_cnt = torch.clamp(fin_cnt + add.sum(1), max=nb)
        # next beams: the first nb non-eos candidates in rank order; finished batches stay frozen on pad
        order = (is_eos.long() * (2 * nb) + rank).argsort(dim=1)[:, :nb]
        new_scores = top_s.gather(1, order)
        new_src = src.gather(1, order)
        new_tok = tok.gather(1, order)
        dn = done.unsqueeze(1)
        new_scores = torch.where(dn, torch.full_like(new_scores, -1e9), new_scores)
        new_src = torch.where(dn, base.expand(-1, nb), new_src)
        new_tok = torch.where(dn, torch.full_like(new_tok, pad), new_tok)
        # BeamHypotheses.is_done
        full = fin_cnt >= nb
        if early_stopping is True:
            now = full
        else:
            gl = cur if early_stopping is False else max_length - 1
            now = full & (fin_scores.min(1).values >= new_scores.max(1).values / (max(gl, 1) ** length_penalty))
        done = done | now
        idx = new_src.reshape(-1)
        seqs = seqs.index_select(0, idx)
        seqs[:, cur] = new_tok.reshape(-1)
        caches[0].store.reorder(idx)
        beam_scores = new_scores
        cur += 1
        if cur % check_every == 0 and bool(done.all()):
            break
    # finalize: the running beams of unfinished batches join the finished hypotheses, best one per batch
    live = ~done.unsqueeze(1)
    sc = torch.where(live, beam_scores / (max(cur - 1, 1) ** length_penalty), torch.full_like(beam_scores, -inf))
    add_finished(sc, seqs.view(B, nb, L), torch.full((B, nb), cur, dtype=torch.long, device=dev))
    best, best_len = fin_seqs[:, 0], fin_len[:, 0]
    return best[:, :int(best_len.max())]


# transformers' generation keys that generate() does not implement, with the value at which each one does nothing
# (GenerationConfig._get_default_generation_params() of transformers 5.15; None where it sets none).  A key that
# arrives with another value is named in a one-time warning: the output then differs from transformers'.
_IGNORED_KEYS = {
    "encoder_no_repeat_ngram_size": 0, "bad_words_ids": None, "num_return_sequences": 1, "typical_p": 1.0,
    "min_p": None, "epsilon_cutoff": 0.0, "eta_cutoff": 0.0, "encoder_repetition_penalty": 1.0, "num_beam_groups": 1,
    "diversity_penalty": 0.0, "penalty_alpha": None, "suppress_tokens": None, "begin_suppress_tokens": None,
    "sequence_bias": None, "exponential_decay_length_penalty": None, "renormalize_logits": False,
    "remove_invalid_values": False, "min_new_tokens": None, "guidance_scale": None, "use_cache": True,
    "output_scores": False, "return_dict_in_generate": False,
}
_warned_keys: set = set()


def _warn_ignored(given: dict) -> None:
    names = sorted(k for k, v in given.items() if v is not None and not (k in _IGNORED_KEYS and v == _IGNORED_KEYS[k]))
    new = [k for k in names if k not in _warned_keys]
    if not new:
        return
    _warned_keys.update(new)
    from ..utils.logging import get_logger
    get_logger().warning("generate(): ignoring %s (not implemented: the tokens may differ from transformers')",
                         ", ".join(f"{k}={given[k]!r}" for k in new))


@torch.no_grad()
def generate(model, input_ids, attention_mask=None, max_length: int | None = None, num_beams: int | None = None,
             min_length: int | None = None, length_penalty: float | None = None, no_repeat_ngram_size=None,
             early_stopping=None, forced_bos_token_id=None, forced_eos_token_id=None, max_new_tokens=None,
             global_attention_mask=None, global_index=None, do_sample: bool | None = None,
             temperature: float | None = None, top_k: int | None = None, top_p: float | None = None,
             repetition_penalty: float | None = None, seed: int | None = None, **_unused):
    """Greedy search, beam search or multinomial sampling with a KV cache.

    Every option resolves as: the explicit argument, then ``model.config.generation``, then the default of the
    installed transformers (5.15: ``GenerationConfig()`` leaves every attribute None and ``generate()`` fills them from
    ``GenerationConfig._get_default_generation_params()``): ``max_length=20, num_beams=1, min_length=0,
    length_penalty=1.0, no_repeat_ngram_size=0, early_stopping=False, do_sample=False, temperature=1.0, top_k=50,
    top_p=1.0, repetition_penalty=1.0``.

    ``repetition_penalty`` r != 1: every token id in the row's decoder prefix (start token included) gets
    ``x * r if x < 0 else x / r`` — on the raw logits in greedy search and sampling, on the log-probabilities in beam
    search (as transformers), before the n-gram / min-length bans and the forced tokens.  ``do_sample``: after those,
    temperature (``x / T``), top-k (ties with the k-th value kept; 0 or >= V: off) and top-p by value (kept iff the
    softmax mass of the strictly larger scores is < ``top_p``; >= 1: off), then a Gumbel-max draw from the
    counter-based uniforms of ops/rng.py ``sample_uniform(seed, step, rows, row, token)``: the same ``seed`` gives the
    same tokens (None: the next seed of the default seed stream).  Beam sampling is not implemented.  Keys of
    transformers' generation config that are not implemented are ignored with a one-time warning that names them."""
    cfg = model.config
    gen = dict(cfg.generation)
    _warn_ignored({**{k: v for k, v in gen.items() if k in _IGNORED_KEYS}, **_unused})
    max_length = max_length if max_length is not None else gen.get("max_length", 20)
    if max_new_tokens is not None:
        max_length = max_new_tokens + 1
    num_beams = num_beams if num_beams is not None else gen.get("num_beams", 1)
    min_length = min_length if min_length is not None else gen.get("min_length", 0)
    length_penalty = length_penalty if length_penalty is not None else gen.get("length_penalty", 1.0)
    no_repeat_ngram_size = no_repeat_ngram_size if no_repeat_ngram_size is not None else \
        gen.get("no_repeat_ngram_size", 0)
    early_stopping = early_stopping if early_stopping is not None else gen.get("early_stopping", False)
    forced_bos = forced_bos_token_id if forced_bos_token_id is not None else cfg.forced_bos_token_id
    forced_eos = forced_eos_token_id if forced_eos_token_id is not None else cfg.forced_eos_token_id
    do_sample = bool(do_sample if do_sample is not None else gen.get("do_sample", False))
    temperature = float(temperature if temperature is not None else gen.get("temperature", 1.0))
    top_k = int(top_k if top_k is not None else gen.get("top_k", 50))
    top_p = float(top_p if top_p is not None else gen.get("top_p", 1.0))
    repetition_penalty = float(repetition_penalty if repetition_penalty is not None
                               else gen.get("repetition_penalty", 1.0))
    if repetition_penalty <= 0:
        raise ValueError(f"repetition_penalty must be > 0, got {repetition_penalty}")
    if do_sample:
        if max(1, num_beams) > 1:
            raise ValueError("do_sample with num_beams > 1 (beam sampling) is not implemented")
        if temperature <= 0 or top_k < 0 or not 0 < top_p <= 1:
            raise ValueError(f"sampling needs temperature > 0, top_k >= 0 and 0 < top_p <= 1; got {temperature}, "
                             f"{top_k}, {top_p}")
        if seed is None:
            from ..ops import rng
            seed = rng.default_rng().next_seed()
        seed = int(seed) & 0xFFFFFFFF
    eos, pad, start = cfg.eos_token_id, cfg.pad_token_id, cfg.decoder_start_token_id
    was_training = model.training
    model.eval()
    try:
        B = input_ids.shape[0]
        dev = input_ids.device
        if global_attention_mask is not None or global_index is not None:  # LED's global tokens (models/bart.py)
            enc = model.encode(input_ids, attention_mask, global_attention_mask=global_attention_mask,
                               global_index=global_index)
        else:
            enc = model.encode(input_ids, attention_mask)
        nb = max(1, num_beams)
        # cross-attention K/V projected once per batch entry and shared by its nb hypotheses: the decoder's
        # cross-attention runs the beams as nb query rows of one (entry, head) — K/V read once per step, not nb times
        cross = model.project_cross_kv(enc)
        if nb > 1 and not routing.get("gen_shared_cross"):  # A/B: per-hypothesis copies
            enc = enc.repeat_interleave(nb, 0)
            attention_mask = attention_mask.repeat_interleave(nb, 0) if attention_mask is not None else None
            cross = model.project_cross_kv(enc)
        N = B * nb
        H, D = _head_geom(model)
        dtype = next(model.parameters()).dtype
        store = KVStore(cfg.num_decoder_layers, N, max_length, H, D, dtype, dev, nb)
        caches = store.layers
        seqs = torch.full((N, max_length), pad, dtype=torch.long, device=dev)
        seqs[:, 0] = start
        cur = 1
        check_every = max(1, int(routing.get("gen_check_every")))

        def process(logp, sq, c):
            return _apply_processors_device(logp, sq, c, min_length, no_repeat_ngram_size, forced_bos, forced_eos,
                                            max_length, eos)

        proc = (min_length, no_repeat_ngram_size, forced_bos, forced_eos, max_length, eos)
        if nb == 1:  # greedy / sampling: device-side done flags, one host check every check_every steps
            done = torch.zeros(B, dtype=torch.bool, device=dev)
            all_done_at = []
            while cur < max_length:
                h = model.decode(seqs[:, cur - 1:cur], enc, attention_mask, caches=caches, q_offset=cur - 1,
                                 cross_kv=cross)
                logits = model.lm_logits(h[:, -1])
                if do_sample:
                    nxt = _sample_step(logits, seqs, cur, proc, repetition_penalty, temperature, top_k, top_p, seed,
                                       cur - 1)
                else:
                    logp = process(torch.log_softmax(_penalize(logits.float(), seqs, cur, repetition_penalty),
                                                     dim=-1), seqs, cur)
                    nxt = logp.argmax(-1)
                nxt = torch.where(done, torch.full_like(nxt, pad), nxt)
                seqs[:, cur] = nxt
                if eos is not None:
                    done |= nxt == eos
                all_done_at.append(done.all())
                cur += 1
                if cur % check_every == 0 and bool(all_done_at[-1]):
                    break
            # trim the steps run after every sequence had finished (at most check_every - 1)
            flags = torch.stack(all_done_at).tolist() if all_done_at else []
            end = next((i + 2 for i, f in enumerate(flags) if f), cur)
            return seqs[:, :end]
        if not routing.get("gen_host"):
            return _beam_search_device(model, seqs, enc, attention_mask, caches, cross, B, nb, max_length, proc,
                                       eos, pad, length_penalty, early_stopping, check_every, repetition_penalty)
        # ---------------------------------------------------------------- beam search, host bookkeeping
        # (routing gen_host=1: the original per-step host loop, kept as the A/B oracle of the device version)
        beam_scores = torch.zeros(B, nb, device=dev)
        beam_scores[:, 1:] = -1e9
        beam_scores = beam_scores.view(-1)
        finished = [[] for _ in range(B)]  # (score, tokens)
        batch_done = [False] * B
        V = cfg.vocab_size
        while cur < max_length:
            h = model.decode(seqs[:, cur - 1:cur], enc, attention_mask, caches=caches, q_offset=cur - 1,
                             cross_kv=cross)
            logp = _penalize(torch.log_softmax(model.lm_logits(h[:, -1]).float(), dim=-1), seqs, cur,
                             repetition_penalty)
            logp = _apply_processors(logp, seqs[:, :cur], cur, cfg, min_length, no_repeat_ngram_size, forced_bos,
                                     forced_eos, max_length, eos)
            V = logp.shape[-1]
            cand = (beam_scores[:, None] + logp).view(B, nb * V)
            top_s, top_i = cand.topk(2 * nb, dim=1)
            top_s, top_i = top_s.tolist(), top_i.tolist()
            new_scores = torch.empty(B, nb, device=dev)
            new_beam = torch.empty(B, nb, dtype=torch.long)
            new_tok = torch.empty(B, nb, dtype=torch.long)
            for b in range(B):
                if batch_done[b]:
                    new_scores[b] = -1e9
                    new_beam[b] = b * nb
                    new_tok[b] = pad
                    continue
                k = 0
                for rank, (s, idx) in enumerate(zip(top_s[b], top_i[b])):
                    beam, tok = divmod(idx, V)
                    src = b * nb + beam
                    if eos is not None and tok == eos:
                        if rank >= nb:
                            continue
                        hyp = seqs[src, :cur].tolist() + [tok]
                        gen_len = len(hyp) - 1
                        finished[b].append((s / (max(gen_len, 1) ** length_penalty), hyp))
                        finished[b].sort(key=lambda x: -x[0])
                        del finished[b][nb:]
                    else:
                        new_scores[b, k] = s
                        new_beam[b, k] = src
                        new_tok[b, k] = tok
                        k += 1
                    if k == nb:
                        break
                # stopping rule (BeamHypotheses.is_done)
                if len(finished[b]) == nb:
                    if early_stopping is True:
                        batch_done[b] = True
                    else:
                        best_running = float(new_scores[b].max())
                        gl = cur if early_stopping is False else max_length - 1
                        if finished[b][-1][0] >= best_running / (max(gl, 1) ** length_penalty):
                            batch_done[b] = True
            beam_idx = new_beam.view(-1).to(dev)
            seqs = seqs.index_select(0, beam_idx)
            seqs[:, cur] = new_tok.view(-1).to(dev)
            caches[0].store.reorder(beam_idx)
            beam_scores = new_scores.view(-1)
            cur += 1
            if all(batch_done):
                break
        # finalize: add running beams
        scores = beam_scores.view(B, nb).tolist()
        for b in range(B):
            if batch_done[b]:
                continue
            for j in range(nb):
                hyp = seqs[b * nb + j, :cur].tolist()
                gen_len = len(hyp) - 1
                finished[b].append((scores[b][j] / (max(gen_len, 1) ** length_penalty), hyp))
            finished[b].sort(key=lambda x: -x[0])
        best = [finished[b][0][1] for b in range(B)]
        L = max(len(x) for x in best)
        out = torch.full((B, L), pad, dtype=torch.long, device=dev)
        for b, x in enumerate(best):
            out[b, : len(x)] = torch.tensor(x, device=dev)
        return out
    finally:
        model.train(was_training)
