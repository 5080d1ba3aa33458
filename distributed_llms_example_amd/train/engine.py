"""The training step every loop shares: model → flat params → gradient reducer → fused AdamW.

Both the Trainer-style loop (train/trainer.py, ref/train-torchrun.py) and the Accelerate-style
facade (train/accelerator.py, ref/train-accelerator.py / train-task.py) — and bench.py — dispatch to
this one engine and therefore to the same kernel library and the same RCCL reducer (BASELINE.json
north star: "both loops dispatch to the same kernel library").
"""
from __future__ import annotations

import contextlib
import os

import torch

from ..data.packing import PACKED_KEYS
from ..models.distill import Distill
from ..models.preference import Preference, check_batch as check_preference_batch
from ..ops import gemm
from ..ops import rng as rng_mod
from ..ops import streams
from ..ops.distill import check_weights
from ..ops.preference import check_config as check_preference
from ..ops.optim import FusedAdafactor, FusedAdamW
from ..utils import profiling
from ..parallel.env import DistEnv
from ..parallel.flat import FlatParams
from ..parallel.reducer import DEFAULT_BUCKET_MB, GradReducer, wire_dtype_of

# transformers Trainer.get_decay_parameter_names: no decay for biases and norm weights (trainer.py:1305-1315)
def default_no_decay(name: str) -> bool:
    n = name.lower()
    return n.endswith(".bias") or "layer_norm" in n or "layernorm" in n or "norm.weight" in n


def default_grad_dtype(param_dtype: torch.dtype) -> torch.dtype:
    """Gradient buffer dtype: fp32 (the reference's HF Trainer / Accelerate keep fp32 gradients, and GA sums
    16 micro-batches, ref/train-torchrun.py:126) unless ``DLLM_GRAD_DTYPE=bf16`` opts into param-dtype
    gradients (half the all-reduce bytes, every accumulation rounded to 8 mantissa bits)."""
    choice = os.environ.get("DLLM_GRAD_DTYPE", "fp32").lower()
    if choice in ("bf16", "param", "same"):
        return param_dtype
    return torch.float32


def token_count(labels: torch.Tensor, ignore_index: int = -100) -> torch.Tensor:
    """Non-ignored target tokens of a micro-batch, as a device scalar (no host sync)."""
    return (labels != ignore_index).sum()


def pair_count(labels: torch.Tensor) -> torch.Tensor:
    """Preference pairs of a micro-batch (``labels [2P, T]``: interleaved chosen / rejected rows), as a device scalar."""
    return torch.full((), labels.shape[0] // 2, dtype=torch.int64, device=labels.device)


class TrainEngine:
    def __init__(self, model: torch.nn.Module, env: DistEnv, *, lr: float = 5e-5, weight_decay: float = 0.0,
                 betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm: float | None = 1.0,
                 dtype: torch.dtype = torch.bfloat16, bucket_mb: float | str = DEFAULT_BUCKET_MB, overlap: bool = True,
                 no_decay=default_no_decay, label_smoothing: float = 0.0, grad_dtype: torch.dtype | None = None,
                 force_reducer: bool = False, grad_reduce_dtype: str | None = None, optim: str = "adamw",
                 teacher: torch.nn.Module | None = None, kd_alpha: float = 0.5, kd_temperature: float = 2.0,
                 reference: torch.nn.Module | None = None, dpo_beta: float = 0.1, dpo_loss: str = "sigmoid",
                 dpo_label_smoothing: float = 0.0, dpo_sft_alpha: float = 0.0):
        """``bucket_mb``: MiB per all-reduce bucket, or "auto" (parallel/reducer.py choose_bucket_mb: probed on the
        job's process group, recorded in ``reducer.bucket_choice``).  ``grad_reduce_dtype``: "bf16" compresses each bucket
        for the wire only (fp32 accumulation kept), None / "fp32" reduces the gradient buffer as it is.  ``optim``:
        "adamw", or "adafactor" as the HF Trainer builds it (scale_parameter=False, relative_step=False, the learning
        rate from ``lr``; ``betas`` / ``eps`` are AdamW's and unused).  ``teacher``: a frozen model to distil from
        (``set_teacher``): training steps then minimise (1 - kd_alpha) CE + kd_alpha T^2 KL(teacher || student) at
        temperature ``kd_temperature`` (ops/distill.py).  ``reference``: a frozen reference policy (``set_reference``):
        training steps then minimise the preference loss (ops/preference.py) of batches of (prompt, chosen, rejected)
        triples, normalised by pairs."""
        self.env = env
        self.model = model.to(device=env.device, dtype=dtype)
        self.dtype = dtype
        self.flat = FlatParams(self.model, grad_dtype=grad_dtype or default_grad_dtype(dtype))
        streams.tag_roles(self.model)  # layer roles for the paired side-stream policy (ops/streams.py)
        # force_reducer: a reducer (and its collectives) on a 1-rank process group — GPU tests of the RCCL paths
        self.reducer = (GradReducer(self.flat, bucket_mb=bucket_mb, overlap=overlap, force=force_reducer,
                                    wire_dtype=wire_dtype_of(grad_reduce_dtype))
                        if env.world_size > 1 or force_reducer else None)
        if self.reducer is not None:
            self.reducer.broadcast_params(self.model)
        if optim == "adamw":
            self.optimizer = FusedAdamW(self.flat, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                        no_decay=no_decay)
        elif optim == "adafactor":
            from ..models.hf_io import hf_param_parts
            cfg = getattr(self.model, "config", None)
            self.optimizer = FusedAdafactor(self.flat, lr=lr, weight_decay=weight_decay, scale_parameter=False,
                                            relative_step=False, no_decay=no_decay,
                                            parts=(lambda n: hf_param_parts(cfg, n)) if cfg is not None else None)
        else:
            raise ValueError(f"optim must be 'adamw' or 'adafactor', got {optim!r}")
        self.max_grad_norm = max_grad_norm
        self.label_smoothing = label_smoothing
        self.step_seed: rng_mod.StepSeed | None = None
        self._init_defer()
        self.set_teacher(teacher, kd_alpha, kd_temperature)
        self.set_reference(reference, dpo_beta, dpo_loss, dpo_label_smoothing, dpo_sft_alpha)

    def set_reference(self, model: torch.nn.Module | None, beta: float = 0.1, kind: str = "sigmoid",
                      label_smoothing: float = 0.0, sft_alpha: float = 0.0) -> None:
        """Preference optimisation against the frozen reference policy ``model`` (None: plain CE).  Like a teacher
        (``set_teacher``) the reference is cast to the compute dtype, put in ``eval()`` and frozen; it lives outside the
        flat parameters, the reducer, the optimizer and the checkpoints, and runs under ``no_grad`` in a seed scope of
        its own, on the step's stream.  Batches then carry ``labels [2P, T]`` (interleaved chosen / rejected rows) over
        ``input_ids [P, S]``, and ``forward_backward`` normalises by pairs."""
        self.reference = None
        self.dpo = (float(beta), str(kind), float(label_smoothing), float(sft_alpha))
        self.last_pref_stats = None
        if model is None:
            return
        check_preference(beta, kind, label_smoothing)
        if self.teacher is not None:
            raise ValueError("a reference policy (--dpo-beta) and a teacher (--teacher-ckpt) exclude each other")
        rv, pv = model.config.vocab_size, self.model.config.vocab_size
        if rv != pv:
            raise ValueError(f"reference (--ref-ckpt) vocab_size {rv} and policy vocab_size {pv} differ (a reference "
                             "with another vocabulary is not supported)")
        if model is self.model:
            raise ValueError("the reference must be a model of its own (a frozen copy), not the policy")
        self._check_reference_cp()
        self.reference = model.to(device=self.env.device, dtype=self.dtype).eval().requires_grad_(False)

    def _check_reference_cp(self) -> None:
        enc = getattr(self.model, "encoder", None)
        if getattr(enc, "_cp_group", False) is not False:
            raise NotImplementedError("--context-parallel with --dpo-beta is not implemented: the reference's encoder "
                                      "is not sharded")

    def item_count(self, labels: torch.Tensor) -> torch.Tensor:
        """What an optimizer step's loss is normalised by, counted on one micro-batch (a device scalar): preference
        pairs with a reference policy, else non-ignored target tokens."""
        return pair_count(labels) if self.reference is not None else token_count(labels)

    def set_teacher(self, teacher: torch.nn.Module | None, alpha: float = 0.5, temperature: float = 2.0) -> None:
        """Distil from ``teacher`` (None: plain CE).  The teacher is cast to the compute dtype, put in ``eval()`` and
        frozen; it lives outside the flat parameters, the reducer, the optimizer and the checkpoints.  It runs in
        ``eval()`` under a seed scope of its own (``forward``), so it draws nothing from the dropout seed stream and the
        student's masks are those of a run without it."""
        self.teacher, self.kd_alpha, self.kd_temperature = None, float(alpha), float(temperature)
        self.last_ce_loss = self.last_kd_loss = None
        if teacher is None:
            return
        if getattr(self, "reference", None) is not None:
            raise ValueError("a teacher (--teacher-ckpt) and a reference policy (--dpo-beta) exclude each other")
        check_weights(alpha, temperature)
        tv, sv = teacher.config.vocab_size, self.model.config.vocab_size
        if tv != sv:
            raise ValueError(f"teacher vocab_size {tv} and student vocab_size {sv} differ (teachers with another "
                             "vocabulary are not supported)")
        if teacher is self.model:
            raise ValueError("the teacher must be a model of its own, not the student")
        self._check_teacher_cp()
        self.teacher = teacher.to(device=self.env.device, dtype=self.dtype).eval().requires_grad_(False)

    def _check_teacher_cp(self) -> None:
        enc = getattr(self.model, "encoder", None)
        if getattr(enc, "_cp_group", False) is not False:
            raise NotImplementedError("--context-parallel with a teacher (--teacher-ckpt) is not implemented: the "
                                      "teacher's encoder is not sharded")

    # micro-batches of at most this many input tokens defer their weight gradients to the window's last one
    DEFER_MAX_TOKENS = 16384

    def _init_defer(self):
        """Deferred weight gradients for gradient accumulation (ops/gemm.py WgradDefer): ``DLLM_DEFER_WGRAD`` = auto
        (micro-batches of <= DEFER_MAX_TOKENS input tokens on the GPU), 1 (always), 0 (never).  Kept operands end the
        window's deferral early past 60 % of the device memory."""
        cap = None
        if self.env.device.type == "cuda":
            cap = int(0.6 * torch.cuda.get_device_properties(self.env.device).total_memory)
        self.wgrad_defer = gemm.WgradDefer(mem_cap=cap)
        self._defer_mode = os.environ.get("DLLM_DEFER_WGRAD", "auto").lower()
        self._ga_k = 0
        # callers that measure one micro-batch's activation memory (train/trainer.py coalescing) switch deferral off for
        # that step: the kept operands of the whole window would count as one micro-batch's activations
        self.defer_enabled = True

    def _defer_for(self, batch: dict, grad_accum: int) -> gemm.WgradDefer | None:
        if grad_accum <= 1 or not self.defer_enabled or self._defer_mode in ("0", "off", "false"):
            return None
        if self._defer_mode == "auto":
            ids = batch.get("input_ids")
            if self.env.device.type != "cuda" or ids is None or ids.numel() > self.DEFER_MAX_TOKENS:
                return None
        return self.wgrad_defer

    @classmethod
    def from_parts(cls, model: torch.nn.Module, env: DistEnv, flat: FlatParams, reducer: GradReducer | None,
                   optimizer: FusedAdamW, max_grad_norm: float | None = None, label_smoothing: float = 0.0,
                   teacher: torch.nn.Module | None = None, kd_alpha: float = 0.5, kd_temperature: float = 2.0,
                   reference: torch.nn.Module | None = None, dpo_beta: float = 0.1, dpo_loss: str = "sigmoid",
                   dpo_label_smoothing: float = 0.0, dpo_sft_alpha: float = 0.0):
        """An engine over state another front end already built (train/accelerator.py: the prepared model's flat
        buffers and reducer, the prepared optimizer), so its loop can run the same step — and the same HIP-graph
        step runner (train/graph.py) — as the Trainer."""
        eng = cls.__new__(cls)
        eng.env, eng.model, eng.dtype = env, model, flat.dtype
        eng.flat, eng.reducer, eng.optimizer = flat, reducer, optimizer
        eng.max_grad_norm, eng.label_smoothing = max_grad_norm, label_smoothing
        eng.step_seed = None
        eng._init_defer()
        eng.set_teacher(teacher, kd_alpha, kd_temperature)
        eng.set_reference(reference, dpo_beta, dpo_loss, dpo_label_smoothing, dpo_sft_alpha)
        return eng

    def enable_step_seeds(self, start: int | None = None) -> rng_mod.StepSeed:
        """Dropout seeds that a captured HIP graph can replay (ops/rng.py StepSeed): from now on every micro-step
        advances a device counter the kernels mix into each site seed, and the host seed stream restarts per micro-step.
        Masks differ from the default mode's (another, equally uniform, stream), so enable it before training."""
        if self.step_seed is None:
            self.step_seed = rng_mod.StepSeed(self.env.device)
            self.step_seed.enable()
        if start is not None:  # resumed run (train/checkpoint.py "step_seed")
            self.step_seed.t.fill_(int(start))
            self.step_seed.host = int(start)
        return self.step_seed

    def disable_step_seeds(self) -> None:
        """Back to the default dropout seed stream: the kernels' device step pointer, the active-step registry and the
        host stream's site mode are all restored (StepSeed.disable), and forward_backward stops advancing it."""
        if self.step_seed is not None:
            self.step_seed.disable()
            self.step_seed = None

    def no_sync(self):
        return self.reducer.no_sync() if self.reducer is not None else contextlib.nullcontext()

    def forward(self, batch: dict, distill: bool = True):
        """The model's forward on ``batch``.  With a teacher (``set_teacher``) the teacher runs first, under ``no_grad``,
        and the loss is the distillation loss; ``distill=False`` (evaluation) keeps plain CE on the student alone.
        With a reference policy (``set_reference``) the reference runs first, the same way, and the loss is the
        preference loss of the batch's pairs, in training and in evaluation alike."""
        self.flat.reset_pending()
        # packed rows (data/packing.py) carry their segment and position ids; other batches none of these keys
        packed = {k: batch[k] for k in PACKED_KEYS if k in batch}
        # LED batches (data/collator.py) carry their global tokens, as a mask and as an index of fixed shape
        packed.update({k: batch[k] for k in ("global_attention_mask", "global_index") if k in batch})
        if self.teacher is not None and distill:
            self._check_teacher_cp()
            # a stream of its own: every block draws a scope seed even at p = 0 (models/blocks.py), and the student's
            # stream must be the one of a run without a teacher
            with torch.no_grad(), rng_mod.rng_scope(0):
                th, tw, tb = self.teacher.lm_head_operands(
                    input_ids=batch["input_ids"], attention_mask=batch.get("attention_mask"),
                    decoder_input_ids=batch.get("decoder_input_ids"), labels=batch["labels"], **packed)
            packed["distill"] = Distill(th, tw, tb, self.kd_alpha, self.kd_temperature)
        if self.reference is not None:
            self._check_reference_cp()
            if any(k in batch for k in PACKED_KEYS):
                raise NotImplementedError("--pack-sequences with --dpo-beta is not implemented: a packed row has no "
                                          "(chosen, rejected) pair structure")
            check_preference_batch(batch["input_ids"], batch["labels"])
            with torch.no_grad(), rng_mod.rng_scope(0):  # a seed stream of its own, as the teacher's
                rh, rw, rb = self.reference.lm_head_operands(
                    input_ids=batch["input_ids"], attention_mask=batch.get("attention_mask"),
                    decoder_input_ids=batch.get("decoder_input_ids"), labels=batch["labels"], **packed)
            packed["preference"] = Preference(rh, rw, rb, *self.dpo)
        return self.model(input_ids=batch["input_ids"], attention_mask=batch.get("attention_mask"),
                          decoder_input_ids=batch.get("decoder_input_ids"), labels=batch["labels"],
                          label_smoothing=self.label_smoothing, **packed)

    def backward(self, loss: torch.Tensor, scale: float = 1.0, sync: bool = True):
        ctx = contextlib.nullcontext() if sync else self.no_sync()
        with ctx:
            (loss * scale if scale != 1.0 else loss).backward()
        if sync and self.reducer is not None:
            self.reducer.post_backward()

    def forward_backward(self, batch: dict, grad_accum: int = 1, sync: bool = True,
                         num_items: torch.Tensor | None = None, dp_ranks: int | None = None) -> torch.Tensor:
        """Forward + backward of one micro-batch; returns its mean loss (detached).

        ``num_items``: the GLOBAL number of non-ignored target tokens (with a reference policy: of preference pairs,
        ``item_count``) of the whole optimizer step (all GA
        micro-batches on all data-parallel ranks, a device scalar).  Given, the gradient is that of
        Σ token losses / num_items — every token weighs the same however the tokens are spread over
        micro-batches and ranks (HF Trainer ``num_items_in_batch``); the reducer's average
        over ranks is undone by the number of data-parallel ranks ``dp_ranks`` whose tokens ``num_items``
        counts (default: the reducer's world; context-parallel ranks share one batch and count once).  Without it each micro-batch mean is divided by
        ``grad_accum`` (identical when every micro-batch has the same token count)."""
        ctx = contextlib.nullcontext() if sync else self.no_sync()
        if self.step_seed is not None:
            self.step_seed.advance()
            rng_mod.default_rng().begin_micro_step()
        # weight gradients on a side stream (ops/streams.py) unless the reducer launches all-reduces from the hooks
        # of this backward (those order themselves after the compute stream only)
        hooks_reduce = self.reducer is not None and sync and self.reducer.overlap and self.reducer.dp
        ids = batch.get("input_ids")
        side = streams.scope(streams.default_enabled(ids.numel() if ids is not None else None) and not hooks_reduce
                             and self.env.device.type == "cuda")
        # the accumulation window ends at the synchronising micro-batch, or after grad_accum of them (a graph's split
        # schedule runs every micro-batch unsynchronised and reduces after the last)
        self._ga_k += 1
        last = sync or self._ga_k >= grad_accum
        if last:
            self._ga_k = 0
        dfr = self._defer_for(batch, grad_accum)
        if dfr is None and last and self.wgrad_defer.active and self.wgrad_defer.pending():
            # a last micro-batch that does not defer itself (too many tokens) still closes the window the earlier ones
            # opened: its weight-gradient GEMMs merge the kept segments in the backward, before the hooks that launch
            # the overlapped bucket all-reduces fire (a flush after backward() would add them after the reduction)
            dfr = self.wgrad_defer
        with ctx, side, gemm.defer_wgrads(dfr, final=last):
            with profiling.range("forward"):
                out = self.forward(batch)
                loss = out.loss
                # the distillation loss's components of this micro-batch (None without a teacher), for logging
                self.last_ce_loss, self.last_kd_loss = getattr(out, "ce_loss", None), getattr(out, "kd_loss", None)
                self.last_pref_stats = getattr(out, "pref_stats", None)  # the preference statistics, likewise
            with profiling.range("backward" if sync else "backward(no_sync)"):
                if num_items is not None:
                    w = dp_ranks if dp_ranks is not None else (self.reducer.world if self.reducer is not None else 1)
                    scale = self.item_count(batch["labels"]).to(torch.float32) * w / num_items.to(torch.float32)
                    (loss * scale).backward()
                else:
                    (loss / grad_accum if grad_accum > 1 else loss).backward()
        if last:
            # weights the last micro-batch did not touch, before the reducer's post-backward launches their buckets
            if self.wgrad_defer.pending():
                self.wgrad_defer.flush()
            self.wgrad_defer.active = True
        elif dfr is not None and dfr.mem_cap is not None and torch.cuda.memory_allocated(self.env.device) > dfr.mem_cap:
            dfr.flush()
            dfr.active = False  # the rest of this window runs undeferred
        if sync and self.reducer is not None:
            with profiling.range("allreduce(post_backward)"):
                self.reducer.post_backward()
        return loss.detach()

    def step(self, lr: float | None = None, hyper: torch.Tensor | None = None):
        """Clip + AdamW + zero_grad.  Returns the pre-clip grad norm as a device tensor (or None).  ``hyper``: device
        [lr, lr / bc1, 1 / sqrt(bc2)] (graph mode, ops/optim.py device_hyper)."""
        if lr is not None:
            self.optimizer.param_groups[0]["lr"] = lr
        if self.wgrad_defer.pending():  # a window left open (fewer micro-batches than its grad_accum)
            self.wgrad_defer.flush()
        self.wgrad_defer.active = True
        self._ga_k = 0
        with profiling.range("optimizer(clip+adamw)" if isinstance(self.optimizer, FusedAdamW) else
                             "optimizer(clip+adafactor)"):
            norm = self.optimizer.step(self.max_grad_norm, hyper=hyper)
            self.optimizer.zero_grad()
        return norm

    def train(self, mode: bool = True):
        self.model.train(mode)
        return self
