"""Kernel routing of a training step — the ONE table of which kernel runs which op.

Every shape-dependent kernel choice of the framework reads its setting here (``get``), so what a given (model, batch)
step launches is decided in one place and can be read off the table below; ``plan`` evaluates it for a step's shapes
(tests/test_routing_gpu.py compares that plan with the kernels a BASELINE.json config's step really launches).

=============================  ===========================================================  =============================
op (key)                       default route                                                 evidence (profiles/)
=============================  ===========================================================  =============================
weight gradient dW = dYᵀX      csrc/gemm_w4.hip weight-gradient mode (K split over           r5_wgrad_w4_ab.txt
                               workgroups, fp32 slabs + csrc/gemm.hip split-K pass) from
                               ``wgrad_min_rows`` (4096) token rows; hipBLASLt below (a       r6_wgrad_small_rows.txt
                               256x256-tile kernel has ~23 us of fixed cost); deferred over
                               a GA window (ops/gemm.py WgradDefer)                          r5_defer_wgrad_ab.txt
projection forward             hipBLASLt + TunableOp table (``proj_fwd`` = lib); arms:       r6_proj_fwd_arms_ab.txt,
Y = X Wᵀ (+ b)                 ``narrow`` (w4 for K <= 1024, N <= 4096 at >=                 r6_w4_vs_lib_nt_pmc.txt
                               ``proj_fwd_min_rows`` tokens: step-neutral), ``w4`` (every
                               forward: -0.46 % t5-base, -0.67 % bart-large)
projection input gradient      w4 from ``proj_dgrad_min_rows`` (16K) token rows at any       r6_dgrad_min_rows_ab.txt,
dX (+)= dY W                   width / depth (early-release schedule: faster than the         r6_dgrad_rows_ab.txt
                               library on every such shape); hipBLASLt below (``proj_dgrad``
                               = rows)
FFN, ReLU (T5)                 forward: w4 ReLU + row-Weyl dropout + bit-mask epilogue at     r6_ffn_rowweyl_dropout_ab.txt,
                               every fused size (``ffn_w4_min_rows`` = 0; the ping-pong       r6_ffn_w4_rows_ab.txt
                               forward below it is the A/B arm); backward: w4 through the
                               bit mask; < ``ffn_min_rows`` (1025) rows: hipBLASLt +
                               csrc/act.hip (unfused)                                        r5_ffn_small_rows_ab.txt
FFN, GELU (BART)               ping-pong GEMM with GELU epilogues (``ffn_gelu`` = pp; w4      r5_w4_gelu_ab.txt
                               GELU epilogues measured 0.25-0.43 % slower)
FFN, gated GELU (FLAN-T5)      one GEMM pairing gate / up columns when tokens x d_ff >=       r4_gemm_pp_stage_ab.txt
                               ``gated_min_mf`` and d_model <= ``gated_max_d`` (1024)
LM head + cross-entropy        full logits while they fit ``lmhead_full_mb`` (16 GiB),       r3_lmhead_b512_ab.txt,
                               else vocabulary chunks of ``lmhead_chunk_mb``; the fused       r4_lmhead_fused_ab.txt,
                               GEMM+CE (w4 CEF / CEB epilogues) when ``lmhead`` = fused or    r5_bart_lmhead_fused_ab.txt
                               (auto) when the logits would exceed the budget
distillation loss              csrc/kd.hip (``kd`` = fused): CE + KL to a teacher's logits    kd_step.txt
(CE + KL to a teacher)         in one pass over both [N, V] tensors, gradient in place;
                               both logits tensors count against ``lmhead_full_mb``, above
                               it vocabulary chunks (``kd_chunk_*``); ``composite``: the
                               torch ops.  The GEMM-epilogue CE does not serve this loss
preference loss                csrc/pref.hip (``pref`` = fused): per-row log-probabilities    pref_step.txt
(DPO / IPO / hinge against a   of the policy's and the reference's logits in one pass over
frozen reference)              both [N, V] tensors, one small launch for the pair losses,
                               gradient in place; both logits tensors count against
                               ``lmhead_full_mb``, above it vocabulary chunks
                               (``pref_chunk_*``); ``composite``: the torch ops
attention                      csrc/attn.hip bf16 flash kernels; fp32 inputs on the fp32      r4_t5base_fp32_b16_summary.txt
                               MFMA kernels of csrc/attn_f32.hip (``attn_f32`` = 1)
cross-attention backward       one pass: dQ folded into the short-query dK/dV kernel (one    attn_sq_onepass_ab.txt
(Sq <= 128, no bias, not       workgroup per (batch, head) over every key block, K / V read
causal, >= 2 key blocks)       once, no dQ kernel) when B x H >= 6 per CU (``attn_sq_onepass``
                               = 1; 0: the split arm); below that the dQ kernel + the        r4_dkdv_sq_ab.txt
                               short-query dK/dV kernel at 4 / 2 key blocks per workgroup,
                               or dkdv2 (one per key block) on the smallest launches
attention, head dim != 64      bf16 at head dims 32 .. 128 (% 8 == 0): csrc/attn_hd.hip      attn_hd_vs_composite.txt
                               (``attn_hd`` = 1; 0: the O(Sq·Sk) composite); anything
                               else: the composite, with a one-time warning
sliding-window attention       bf16 at head dims 32 .. 128 (% 8 == 0), 64 included:          attn_window_vs_full.txt
(LongT5-local encoder)         csrc/attn_hd.hip; fp32 at head dim 64: csrc/attn_f32.hip.
                               Their block walks skip the blocks outside the band
                               (O(S·w)); csrc/attn.hip has no window; anything else: the
                               O(S²) composite, with a one-time warning
window + global keys           as the window (same route; bf16 head dim 32: composite): the   attn_global_keys.txt
(LED encoder)                  walks cover the band plus the 64-key blocks that hold a
                               global key, skipping the rest,
                               O(S·(w + 64·such blocks)); the rows at the global positions
                               are an ordinary short-query call (csrc/attn.hip at head dim
                               64)
block-list attention           as the window (same route; bf16 head dim 32 and block sizes   attn_block_lists.txt
(BigBird-Pegasus encoder)      that are no multiple of 64: composite): forward and dQ
                               follow each query block's list of 64-key blocks, dK / dV
                               its transpose; a block listed n times counts n times; the
                               rest is never loaded (``attn_lists`` = 1; 0: the composite)
soft-capped attention          as the window (same route; bf16 head dim 32, and a cap with    attn_softcap.txt
(T5Gemma)                      a bias LUT, segments, global keys or lists: composite):
                               c·tanh(s / c) per score in instantiations of their own in
                               csrc/attn_hd.hip and csrc/attn_f32.hip; csrc/attn.hip has
                               no cap
segment-masked attention       as the window: bf16 (head dim 64 included) on                 attn_segments_vs_masked.txt
(sequence packing)             csrc/attn_hd.hip, fp32 at head dim 64 on csrc/attn_f32.hip;
                               blocks of other segments are skipped by per-block (min,
                               max) id tables; csrc/attn.hip has no segments
long-context attention         query chunks of ``attn_chunk`` rows from ``attn_chunk_min``   (parallel/context.py)
weight gradients, small        side stream for micro-batches <= ``wgrad_stream_max_tokens``  r4_wgrad_stream_ab.txt
micro-batches                  (``wgrad_stream`` = auto | 1 | 0)
beam search                    fused device-side beam step (``gen_fused_beam``), encoder K/V  r3_eval_beam_fused.jsonl
                               shared by a batch entry's beams (``gen_shared_cross``)
sampling                       one launch per decode step (``gen_fused_sample``): penalty,    sample_step.txt
                               bans, temperature, top-k / top-p thresholds by radix select
                               and the Gumbel-max draw in csrc/sample.hip (0: the torch
                               composite, a sort of [rows, V] per step)
low-rank adapters (LoRA)       csrc/lora.hip (``lora`` = fused): mask regenerated from the     lora_step.txt
                               row hash, one pass over x, the output slice read and written
                               once, split reductions summed in order into the flat
                               gradient; ``lib``: the composite on torch matmuls (2-9x
                               slower per adapted projection, 3.3-3.6x per step)
Adafactor                      csrc/adafactor.hip (``adafactor`` = fused): five launches per   adafactor_step.txt
                               step over a device unit table, three gradient reads, fixed-
                               order partial sums; ``composite``: the per-unit torch ops
gradient reducer               native C++ engine (``reducer`` = native | python), buckets     r5_gloo2_gpu.txt
                               re-laid in gradient-ready order (``rebuild_buckets``)
HIP-graph DP schedule          overlap: backward segments cut at bucket readiness            r5_gloo2_gpu_final.txt
                               (``graph_comm`` = overlap | split | capture)
=============================  ===========================================================  =============================

Fixed choices that used to be switches (their losing arms were deleted in round 6): the ReLU backward reads the
forward's bit mask; GELU / attention / post-LN bias gradients come from the producing kernel's column partials; the
post-LN residual gradient accumulates in the input-gradient GEMM (beta = 1); the ping-pong kernel persists on every
shape it serves; the T5 attention forward adds saturated bias tiles as scalars.

Overrides (A/B runs, tests): ``DLLM_ROUTE="key=value,key=value"`` (read at every ``get``: a test may change it between
calls); unknown keys fail loudly.
"""
from __future__ import annotations

import os

DEFAULTS: dict = {
    # projection GEMMs (ops/gemm.py)
    "proj_fwd": "lib",            # lib | w4 | narrow (w4 for K <= 1024, N <= 4096 at >= proj_fwd_min_rows tokens)
    "proj_fwd_min_rows": 131072,
    "proj_dgrad": "rows",         # rows | w4 | lib
    "proj_dgrad_min_rows": 16384,
    # weight gradients (ops/gemm.py): w4 weight-gradient mode from this many token rows, hipBLASLt (fp32 addmm) below
    "wgrad_min_rows": 4096,
    # feed-forward blocks (ops/ffn.py)
    "ffn": "fused",               # fused | unfused
    "ffn_min_rows": 1025,
    "ffn_w4_min_rows": 0,
    "ffn_gelu": "pp",             # pp | w4
    "gated_min_mf": 2 * 256 * 256 * 256,
    "gated_max_d": 1024,
    # LM head + cross-entropy (ops/lm_head.py)
    "lmhead": "auto",             # auto | fused | logits
    "lmhead_full_mb": 16384.0,
    "lmhead_chunk_mb": 128.0,
    # distillation loss (ops/distill.py): csrc/kd.hip, or the torch composite
    "kd": "fused",                # fused | composite
    # preference loss (ops/preference.py): csrc/pref.hip, or the torch composite
    "pref": "fused",              # fused | composite
    # low-rank adapters (ops/lora.py): csrc/lora.hip, or the composite on torch matmuls
    "lora": "fused",              # fused | lib
    # Adafactor (ops/optim.py FusedAdafactor): csrc/adafactor.hip, or the per-unit torch composite
    "adafactor": "fused",         # fused | composite
    # attention (ops/attention.py, parallel/context.py)
    "attn_f32": 1,
    "attn_hd": 1,                 # bf16 head dims 32 .. 128 other than 64 on csrc/attn_hd.hip (0: composite)
    "attn_lists": 1,              # block-list calls on csrc/attn_hd.hip / csrc/attn_f32.hip (0: composite)
    "attn_chunk": 0,              # 0: 8192 rows for < 32 rows per head, else 4096
    "attn_chunk_min": 8192,
    # weight-gradient side stream (ops/streams.py)
    "wgrad_stream": "auto",       # auto | 1 | 0
    "wgrad_stream_max_tokens": 32768,
    "wgrad_stream_lag": 2,
    "wgrad_stream_sites": "",     # comma list of layer roles ("" = the default pairing policy)
    # generation (models/generation.py)
    "gen_fused_beam": 1,
    "gen_fused_sample": 1,        # sampling step on csrc/sample.hip (0: the torch composite)
    "gen_shared_cross": 1,
    "gen_check_every": 8,
    "gen_host": 0,
    # data-parallel runtime (parallel/reducer.py, train/graph.py)
    "reducer": "native",          # native | python
    "rebuild_buckets": 1,
    "graph_comm": "",             # "" = overlap when the reducer overlaps, else split
    # evaluation batch on the GPU (cli.py)
    "eval_batch": 256,
    # read by the C++ launchers (csrc/route.h): ping-pong GEMM tile-group size; test hook forcing the short-query
    # dK/dV kernel on any launch size; its one-pass arm (dQ folded in; 0: dQ kernel + split arm, the tests' comparison)
    "gemm_grp": 4,
    "attn_dkdv_sq_force": 0,
    "attn_sq_onepass": 1,
    # csrc/gemm_w4.hip k-loop schedule (template RS): 769 = early fragment reads + DMAs riding on MFMAs + the LDS buffer
    # released half-way through sub-step 0 so the next DMA spreads over 88 MFMAs (default); 257 = without the early
    # release, 1 = the round-5 schedule; bits 16-128 = timing ablations (tools/gemm_w4_bench.py --ablate; garbage)
    "w4_sched": 769,
}

_cache: tuple[str, dict] | None = None


def overrides() -> dict:
    """The parsed ``DLLM_ROUTE`` overrides (typed like their defaults)."""
    global _cache
    raw = os.environ.get("DLLM_ROUTE", "")
    if _cache is not None and _cache[0] == raw:
        return _cache[1]
    out = {}
    for item in filter(None, (x.strip() for x in raw.split(","))):
        k, _, v = item.partition("=")
        k = k.strip()
        if k not in DEFAULTS:
            raise KeyError(f"DLLM_ROUTE: unknown key {k!r} (known: {', '.join(sorted(DEFAULTS))})")
        d = DEFAULTS[k]
        out[k] = type(d)(float(v)) if isinstance(d, (int, float)) and not isinstance(d, bool) else v.strip()
    _cache = (raw, out)
    return out


def merged(**kw) -> str:
    """A ``DLLM_ROUTE`` string: the current overrides with ``kw`` added (tests: ``monkeypatch.setenv("DLLM_ROUTE",
    routing.merged(lmhead="fused"))``)."""
    cur = dict(overrides())
    for k, v in kw.items():
        if k not in DEFAULTS:
            raise KeyError(f"unknown route key {k!r}")
        cur[k] = v
    return ",".join(f"{k}={v}" for k, v in cur.items())


def get(key: str):
    """The route / threshold ``key`` of the table (``DLLM_ROUTE`` override, else its default)."""
    ov = overrides()
    return ov[key] if key in ov else DEFAULTS[key]


def attention_route(head_dim: int, bf16: bool = True, window: int | None = None, *,
                    segments: bool = False, lists: bool = False, softcap: bool = False) -> str:
    """Kernel family of an attention call on the GPU by head dim and dtype (bf16, else fp32): ``"attn.hip"``,
    ``"attn_hd.hip"``, ``"attn_f32.hip"`` or ``"composite"`` — the rule ops/attention.py ``_route`` applies.
    ``window``: the call's sliding window (None: full attention).  csrc/attn.hip has no window, so a windowed bf16
    call at head dim 64 runs csrc/attn_hd.hip's 64-wide instantiation.  ``segments``: the call carries segment ids
    (sequence packing); csrc/attn.hip has none either, so the same holds.  The fp32 route is unchanged by both.
    A windowed call with global keys (LED) routes as the windowed call, except bf16 at head dim 32, where
    csrc/attn_hd.hip serves no global keys and ops/attention.py ``_route`` takes the composite.  ``lists``: the call
    carries block lists (BigBird); it routes as a call with segments, with the same exception at head dim 32 and
    ``attn_lists`` = 0 sending it to the composite.  ``softcap``: the call caps its scores (Gemma 2 / T5Gemma);
    csrc/attn.hip has no cap, so it routes as a windowed call does — bf16 at head dim 32 excepted, where
    csrc/attn_hd.hip has none either (composite); a cap with a bias LUT, segments, global keys or lists is the
    composite's (ops/attention.py ``_route``)."""
    if lists and not get("attn_lists"):
        return "composite"
    if softcap and (segments or lists or bf16 and head_dim == 32):
        return "composite"
    if head_dim == 64 and (window is None and not segments and not lists and not softcap or not bf16):
        return "attn.hip" if bf16 else ("attn_f32.hip" if get("attn_f32") else "composite")
    if bf16 and 32 <= head_dim <= 128 and head_dim % 8 == 0 and get("attn_hd"):
        return "attn_hd.hip"
    return "composite"


def plan(model: str, tokens_enc: int, tokens_dec: int, d_model: int, d_ff: int, act: str, vocab: int, *,
         head_dim: int = 64, window: int | None = None, teacher: bool = False) -> dict:
    """What the table routes for one training step of an encoder-decoder model with these shapes (per micro-batch
    token rows): a dict op -> kernel family, as the tests and docs/ARCHITECTURE.md read it.  ``head_dim``: the
    model's attention head dim (bf16 step); ``window``: the encoder self-attention's sliding window (LongT5-local),
    reported as ``attention.window`` with its kernel family under ``enc.self_attention``."""
    rows = {"enc": tokens_enc, "dec": tokens_dec}
    out = {}
    dmode = get("proj_dgrad")
    for side, r in rows.items():
        out[f"{side}.wgrad"] = "w4-wgrad" if r >= get("wgrad_min_rows") else "hipblaslt"
        fm = get("proj_fwd")
        out[f"{side}.proj_fwd"] = ("w4" if fm == "w4" else "w4-narrow" if fm == "narrow" and r >= get("proj_fwd_min_rows")
                                   else "hipblaslt")
        if dmode == "w4":
            dg = "w4"
        elif dmode == "lib":
            dg = "hipblaslt"
        else:
            dg = "w4" if r >= get("proj_dgrad_min_rows") else "hipblaslt"
        out[f"{side}.proj_dgrad"] = dg
        if get("ffn") != "fused" or r < get("ffn_min_rows"):
            out[f"{side}.ffn"] = "hipblaslt+act"
        elif act == "relu":
            out[f"{side}.ffn"] = "w4-relu" if r >= get("ffn_w4_min_rows") else "pingpong-relu+w4-drelu"
        elif act in ("gelu", "gelu_new", "gelu_fast") and not act.startswith("gated"):
            out[f"{side}.ffn"] = "w4-gelu" if get("ffn_gelu") == "w4" else "pingpong-gelu"
        else:
            out[f"{side}.ffn"] = ("pingpong-geglu" if r * d_ff >= get("gated_min_mf") and d_model <= get("gated_max_d")
                                  else "hipblaslt+act")
    logits_mb = tokens_dec * vocab * 2 / 2**20
    lm = get("lmhead")
    out["lm_head"] = ("w4-fused-ce" if lm == "fused" or (lm == "auto" and logits_mb > get("lmhead_full_mb"))
                      else "hipblaslt+ce")
    if teacher:  # the distillation loss replaces the LM head's CE (ops/distill.py); no GEMM-epilogue form
        if get("kd") != "fused":
            out["lm_head"] = "hipblaslt+composite-kd"
        elif get("lmhead_full_mb") >= 0 and 2 * logits_mb > get("lmhead_full_mb"):
            out["lm_head"] = "hipblaslt+kd-chunk"
        else:
            out["lm_head"] = "hipblaslt+kd"
    out["attention"] = attention_route(head_dim)
    if window is not None:
        out["attention.window"] = int(window)
        out["enc.self_attention"] = attention_route(head_dim, True, window)
    return out
