"""Shared command-line surface of the three entry points.

The six flags of the reference are kept verbatim (ref/train-torchrun.py:183-188,
ref/train-accelerator.py:320-325, ref/train-task.py:411-416); everything else is optional and
defaults to reference semantics.  Data comes from the Valohai ``dataset``
input (``train.json``/``val.json``), or ``--data-dir``, or ``--synthetic N`` (offline runs).
"""
from __future__ import annotations

import argparse
import os

from .data.dataset import (convert_examples_to_features, convert_pairs_to_features, load_samsum,
                           synthetic_preference_records, synthetic_samsum_records)
from .data.packing import pack_features
from .data.tokenization import load_tokenizer
from .models.config import resolve_config
from .ops import routing
from .platform import valohai


def bucket_mb_arg(v: str):
    """``--bucket-mb``: a size in MiB or ``auto``."""
    return "auto" if str(v).lower() == "auto" else float(v)


def base_parser(description: str, defaults: dict | None = None) -> argparse.ArgumentParser:
    d = {"batch_size": 1, "num_epochs": 1, "warmup_steps": 500, "evaluation_steps": 500}
    d.update(defaults or {})
    ap = argparse.ArgumentParser(description=description)
    ap.add_argument("--model-ckpt", type=str, default="facebook/bart-large-cnn", action=_StoreGiven,
                    help="Pretrained model checkpoint")
    ap.add_argument("--output-dir", type=str, default="bart-large-cnn", help="Output directory for the trained model")
    ap.add_argument("--batch-size", type=int, default=d["batch_size"], help="Batch size")
    ap.add_argument("--num-epochs", type=int, default=d["num_epochs"], help="Number of training epochs")
    ap.add_argument("--warmup-steps", type=int, default=d["warmup_steps"], help="Warmup steps")
    ap.add_argument("--evaluation-steps", type=int, default=d["evaluation_steps"], help="Evaluation steps")
    g = ap.add_argument_group("MI355X framework options (defaults reproduce the reference)")
    g.add_argument("--data-dir", type=str, default=None, help="directory with train.json/val.json")
    g.add_argument("--synthetic", type=int, default=0, help="use N synthetic SAMSum-schema records")
    g.add_argument("--max-source-length", type=int, default=1024)
    g.add_argument("--max-target-length", type=int, default=128)
    g.add_argument("--ignore-pad-labels", action="store_true", help="mask pad tokens out of the loss")
    g.add_argument("--pack-sequences", action="store_true",
                   help="pack several training examples into each max-source-length x max-target-length row, with "
                        "attention confined to each example (segment-masked kernels); steps and schedules then count "
                        "rows.  Implies that pad labels are not trained on (as --ignore-pad-labels); evaluation stays "
                        "unpacked; not for LongT5 or --context-parallel")
    g.add_argument("--precision", choices=["bf16", "fp32"], default=None, help="default: bf16 on GPU, fp32 on CPU")
    g.add_argument("--grad-accum", type=int, default=None)
    g.add_argument("--coalesce-grad-accum", type=str, default="auto",
                   help="run gradient-accumulation micro-batches as fewer larger passes: 'auto' (as many as the "
                        "first step's measured activation memory allows in 60%% of HBM), N (max samples per pass), 0 off")
    g.add_argument("--learning-rate", type=float, default=5e-5)
    g.add_argument("--optim", choices=["adamw", "adafactor"], default="adamw",
                   help="optimizer: fused AdamW, or Adafactor as the HF Trainer builds it (scale_parameter=False, "
                        "relative_step=False, the learning rate from --learning-rate and the usual schedule)")
    g.add_argument("--max-steps", type=int, default=-1)
    g.add_argument("--bucket-mb", type=bucket_mb_arg, default="auto",
                   help="gradient all-reduce bucket size in MiB, or 'auto' (default: probe RCCL's bus bandwidth over "
                        "32-256 MiB on the job's process group and take the smallest size within 5%% of the best)")
    g.add_argument("--no-overlap", action="store_true",
                   help="all-reduce after backward instead of overlapping (HIP-graph steps: the post-backward "
                        "'split' schedule)")
    g.add_argument("--grad-reduce-dtype", choices=["fp32", "bf16"], default="fp32",
                   help="dtype of the gradient all-reduce on the wire: bf16 halves the xGMI bytes; gradients are still "
                        "accumulated in fp32 and widened back after each bucket's all-reduce")
    g.add_argument("--eval-batch-size", type=int, default=None)
    g.add_argument("--max-eval-samples", type=int, default=None)
    g.add_argument("--gen-max-length", type=int, default=128)
    g.add_argument("--num-beams", type=int, default=2)
    g.add_argument("--resume-from", type=str, default=None, help="checkpoint dir, or 'latest'")
    g.add_argument("--save-steps", type=int, default=None,
                   help="full training checkpoint every N optimizer steps (reference: final only)")
    g.add_argument("--seed", type=int, default=42)
    g.add_argument("--gradient-checkpointing", action="store_true",
                   help="recompute each transformer block in backward (long sequences / large models)")
    g.add_argument("--context-parallel", type=int, default=1,
                   help="shard the encoder sequence over groups of N ranks (ring attention; T5 family)")
    g.add_argument("--model-overrides", type=str, default=None,
                   help="comma list key=value applied to the --model-ckpt model's config (e.g. num_layers=2); a "
                        "--teacher-ckpt model keeps its own")
    g.add_argument("--lora-r", type=int, default=0,
                   help="LoRA rank (1 .. 64): freeze the model and train low-rank adapters only; 0 (default) = full "
                        "fine-tuning")
    g.add_argument("--lora-alpha", type=float, default=16.0, help="LoRA scale numerator (scale = alpha / r)")
    g.add_argument("--lora-dropout", type=float, default=0.0, help="dropout on the adapter branch's input")
    g.add_argument("--lora-targets", type=str, default="q,v",
                   help="comma list of adapted projections out of q,k,v,o,wi,wo")
    g.add_argument("--teacher-ckpt", type=str, default=None,
                   help="distil from this frozen teacher (anything --model-ckpt takes): the training loss becomes "
                        "(1 - kd-alpha) CE + kd-alpha T^2 KL(teacher || student); evaluation and the saved model are "
                        "the student's alone")
    g.add_argument("--kd-alpha", type=float, default=0.5, help="weight of the KL term, in [0, 1]")
    g.add_argument("--kd-temperature", type=float, default=2.0, help="softmax temperature T > 0 of the KL term")
    g.add_argument("--student-layers", type=str, default=None, metavar="E,D",
                   help="build the student from the teacher with E encoder and D decoder layers (evenly spaced teacher "
                        "layers, layer 0 kept) instead of loading --model-ckpt; not with --model-overrides")
    g.add_argument("--dpo-beta", type=float, default=None,
                   help="preference optimisation (DPO) at this beta > 0 against a frozen reference policy: records are "
                        "{id, dialogue, chosen, rejected}, the training loss becomes the pairwise preference loss "
                        "(ops/preference.py); not with --teacher-ckpt, --pack-sequences or --context-parallel")
    g.add_argument("--ref-ckpt", type=str, default=None,
                   help="the frozen reference policy of --dpo-beta (anything --model-ckpt takes; default: a copy of "
                        "the --model-ckpt model as loaded)")
    g.add_argument("--dpo-loss", choices=["sigmoid", "ipo", "hinge"], default="sigmoid", help="pair loss of --dpo-beta")
    g.add_argument("--dpo-label-smoothing", type=float, default=0.0,
                   help="probability in [0, 0.5) that a pair's preference is flipped (sigmoid loss)")
    g.add_argument("--dpo-sft-alpha", type=float, default=0.0,
                   help="weight of an added length-averaged NLL term on the chosen target")
    return ap


class _StoreGiven(argparse.Action):
    """``store`` that also records, as ``<dest>_given``, that the flag was on the command line (any spelling argparse
    accepts, whatever list was parsed): a default cannot tell."""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        setattr(namespace, self.dest + "_given", True)


def resolve_distill(args):
    """Validate the distillation flags (loud ``ValueError``s) and, with ``--student-layers``, make the teacher's
    checkpoint the source of the student's config and tokenizer.  Returns ``args``; a no-op without the flags, and on
    ``args`` it has already resolved."""
    from .ops.distill import check_weights
    layers = getattr(args, "student_layers", None)
    teacher = getattr(args, "teacher_ckpt", None)
    if layers and not teacher:
        raise ValueError("--student-layers needs --teacher-ckpt (the student is built from the teacher)")
    if not teacher:
        return args
    check_weights(args.kd_alpha, args.kd_temperature)
    if getattr(args, "context_parallel", 1) > 1:
        raise NotImplementedError("--context-parallel with --teacher-ckpt is not implemented (the teacher's encoder is "
                                  "not sharded)")
    if layers:
        if getattr(args, "model_ckpt_given", False):
            raise ValueError("--student-layers builds the student from --teacher-ckpt: give it or --model-ckpt, not "
                             "both")
        if getattr(args, "model_overrides", None):
            raise ValueError("--student-layers takes the teacher's config with the two layer counts replaced: "
                             "--model-overrides does not apply to it (it is for a --model-ckpt student)")
        if isinstance(layers, str):
            try:
                e, d = (int(x) for x in layers.split(","))
            except ValueError:
                raise ValueError(f"--student-layers takes E,D (two integers), got {layers!r}") from None
            args.student_layers = (e, d)
        args.model_ckpt = teacher
    return args


def preference_on(args) -> bool:
    return getattr(args, "dpo_beta", None) is not None


def resolve_preference(args):
    """Validate the preference-optimisation flags (loud errors that name the flag).  Returns ``args``; a no-op without
    ``--dpo-beta``."""
    if not preference_on(args):
        if getattr(args, "ref_ckpt", None):
            raise ValueError("--ref-ckpt needs --dpo-beta (it names the reference policy of the preference loss)")
        return args
    from .ops.preference import check_config
    check_config(args.dpo_beta, getattr(args, "dpo_loss", "sigmoid"), getattr(args, "dpo_label_smoothing", 0.0))
    if getattr(args, "teacher_ckpt", None):
        raise ValueError("--teacher-ckpt and --dpo-beta exclude each other: a step trains on one loss")
    if getattr(args, "pack_sequences", False):
        raise NotImplementedError("--pack-sequences with --dpo-beta is not implemented: a packed row has no (chosen, "
                                  "rejected) pair structure")
    if getattr(args, "context_parallel", 1) > 1:
        raise NotImplementedError("--context-parallel with --dpo-beta is not implemented (the reference's encoder is "
                                  "not sharded)")
    return args


def preference_kwargs(args) -> dict:
    """The ``dpo_*`` settings of TrainEngine / TrainingArguments / ``make_train_step`` (``{}`` without ``--dpo-beta``)."""
    if not preference_on(args):
        return {}
    return {"dpo_beta": args.dpo_beta, "dpo_loss": args.dpo_loss, "dpo_label_smoothing": args.dpo_label_smoothing,
            "dpo_sft_alpha": args.dpo_sft_alpha}


def build_reference(args, model):
    """The frozen reference policy of ``--dpo-beta`` (None without it): ``--ref-ckpt``, else a copy of ``model`` as it
    stands — call it before adapters are attached or a step is taken.  The saved model is the policy alone."""
    if not preference_on(resolve_preference(args)):
        return None
    import copy
    ref = _load(args.ref_ckpt) if getattr(args, "ref_ckpt", None) else copy.deepcopy(model)
    if ref.config.vocab_size != model.config.vocab_size:
        raise ValueError(f"--ref-ckpt vocab_size {ref.config.vocab_size} and policy vocab_size "
                         f"{model.config.vocab_size} differ (a reference with another vocabulary is not supported)")
    return ref.eval().requires_grad_(False)


def pref_logs(engine) -> dict:
    """The six preference statistics of the engine's last micro-batch when it trains on pairs, else ``{}``."""
    stats = getattr(engine, "last_pref_stats", None)
    if getattr(engine, "reference", None) is None or stats is None:
        return {}
    return {k: round(float(v), 4) for k, v in stats.items()}


def eval_targets(batch):
    """The label rows generation is scored against: the chosen targets of a preference batch (``labels [2P, T]`` over
    ``input_ids [P, S]``), else the labels."""
    labels = batch["labels"]
    return labels[0::2] if labels.shape[0] == 2 * batch["input_ids"].shape[0] else labels


class PreferenceEval:
    """Preference loss and ``rewards/accuracies`` over the validation pairs, next to generation and ROUGE."""

    def __init__(self, engine):
        self.engine, self.loss, self.acc, self.n = engine, 0.0, 0.0, 0

    def add(self, batch):
        if getattr(self.engine, "reference", None) is None:
            return
        import torch
        with torch.no_grad():
            out = self.engine.forward(batch)
        self.loss += float(out.loss)
        self.acc += float(out.pref_stats["rewards/accuracies"])
        self.n += 1

    def result(self) -> dict:
        if not self.n:
            return {}
        return {"eval_loss": self.loss / self.n, "eval_rewards/accuracies": self.acc / self.n}


def _load(ckpt: str, cfg=None):
    from .models import build_model, from_pretrained
    return from_pretrained(ckpt) if os.path.isdir(ckpt or "") else build_model(cfg or resolve_config(ckpt))


def build_models(args, cfg):
    """``(model, teacher)``: the model the entry points train — ``--model-ckpt``, or with ``--student-layers`` a
    shallower copy of the teacher (models/distill.py make_student) — and the ``--teacher-ckpt`` model or None.  On
    ``--resume-from`` the teacher is rebuilt from ``--teacher-ckpt`` the same way: checkpoints hold the student only."""
    teacher_ckpt = getattr(args, "teacher_ckpt", None)
    if not teacher_ckpt:
        return _load(args.model_ckpt, cfg), None
    from .models.distill import make_student
    layers = getattr(resolve_distill(args), "student_layers", None)
    teacher = _load(teacher_ckpt)
    if layers:
        model = make_student(teacher, *layers)
    else:
        model = _load(args.model_ckpt, cfg)
    if model.config.vocab_size != teacher.config.vocab_size:
        raise ValueError(f"teacher vocab_size {teacher.config.vocab_size} and student vocab_size "
                         f"{model.config.vocab_size} differ (teachers with another vocabulary are not supported)")
    return model, teacher


def kd_logs(engine) -> dict:
    """``{"ce_loss", "kd_loss"}`` of the engine's last micro-batch when it distils, else ``{}``."""
    if getattr(engine, "teacher", None) is None or engine.last_ce_loss is None:
        return {}
    return {"ce_loss": round(float(engine.last_ce_loss), 4), "kd_loss": round(float(engine.last_kd_loss), 4)}


def maybe_apply_lora(model, args, log_fn=None):
    """``--lora-r N``: freeze ``model`` and attach adapters (models/lora.py) — before the engine is built — and log the
    trainable / total parameter counts once.  Without the flag the model is returned untouched."""
    if not getattr(args, "lora_r", 0):
        return model
    import json

    from .models.lora import LoraConfig, apply_lora, param_counts
    targets = tuple(t.strip() for t in args.lora_targets.split(",") if t.strip())
    apply_lora(model, LoraConfig(r=args.lora_r, alpha=args.lora_alpha, dropout=args.lora_dropout, targets=targets))
    train, total = param_counts(model)
    if log_fn is not None:
        log_fn(json.dumps({"trainable_params": train, "total_params": total, "lora_r": args.lora_r,
                           "lora_targets": list(targets)}))
    return model


# Evaluation / generation batch when --eval-batch-size is not given.  Beam-search generation is launch-bound at small
# batches (t5-base, 818 samples, num_beams=2, one MI355X: 107 samples/s at batch 64, 195 at 128, 299 at 256, 480 with
# all 818 at once; tools/eval_bench.py, profiles/r2_eval_batch.txt), and a 288 GB GPU holds the caches of hundreds of
# sequences, so GPU runs evaluate in batches of at least this many samples (the reference evaluates with its training
# batch size, or 1 in train-accelerator).  Results are the same per sample.
def gpu_eval_batch() -> int:
    return int(routing.get("eval_batch"))


def eval_batch_size(args, device) -> int:
    if getattr(args, "eval_batch_size", None):
        return args.eval_batch_size
    bs = args.batch_size or 1
    return max(bs, gpu_eval_batch()) if getattr(device, "type", str(device)) == "cuda" else bs


def apply_overrides(cfg, spec: str | None):
    if not spec:
        return cfg
    kv = {}
    for item in spec.split(","):
        k, v = item.split("=")
        cur = getattr(cfg, k)
        kv[k] = type(cur)(v) if not isinstance(cur, bool) else v.lower() in ("1", "true", "yes")
    if "num_layers" in kv and "num_decoder_layers" not in kv:
        kv["num_decoder_layers"] = kv["num_layers"]
    return cfg.replace(**kv)


def load_records(args):
    if args.synthetic and preference_on(args):
        n = args.synthetic
        return {"train": synthetic_preference_records(n, args.seed),
                "validation": synthetic_preference_records(max(4, n // 4), args.seed + 1)}
    if args.synthetic:
        n = args.synthetic
        return {"train": synthetic_samsum_records(n, args.seed), "validation": synthetic_samsum_records(max(4, n // 4),
                                                                                                    args.seed + 1)}
    data_dir = args.data_dir or os.path.dirname(valohai.inputs("dataset").path())
    return load_samsum(data_dir)


def build_data(args, cfg):
    """(tokenizer, train_features, eval_features, eval_records) following convert_examples_to_features."""
    recs = load_records(args)
    if preference_on(resolve_preference(args)):  # (dialogue, chosen, rejected) triples: data/collator.py interleaves
        tok = load_tokenizer(args.model_ckpt, cfg, texts=[r[k] for k in ("dialogue", "chosen", "rejected")
                                                          for r in recs["train"]])
        ev_recs = recs["validation"][: args.max_eval_samples] if args.max_eval_samples else recs["validation"]
        return tok, *(convert_pairs_to_features(r, tok, args.max_source_length, args.max_target_length)
                      for r in (recs["train"], ev_recs))
    tok = load_tokenizer(args.model_ckpt, cfg, texts=[r["dialogue"] for r in recs["train"]] +
                         [r["summary"] for r in recs["train"]])
    tr = convert_examples_to_features(recs["train"], tok, args.max_source_length, args.max_target_length,
                                      ignore_pad_labels=args.ignore_pad_labels)
    if getattr(args, "pack_sequences", False):
        if cfg.model_type == "t5gemma":
            raise NotImplementedError("--pack-sequences is not implemented for T5Gemma (the attention kernels have no "
                                      "soft cap with segments)")
        if cfg.local_encoder:
            raise NotImplementedError("--pack-sequences is not implemented for LongT5 (windowed attention takes no "
                                      "segments)")
        if getattr(args, "context_parallel", 1) > 1:
            raise NotImplementedError("--pack-sequences is not implemented under --context-parallel")
        tr = pack_features(tr, cfg, args.max_source_length, args.max_target_length, seed=args.seed)
    ev_recs = recs["validation"][: args.max_eval_samples] if args.max_eval_samples else recs["validation"]
    ev = convert_examples_to_features(ev_recs, tok, args.max_source_length, args.max_target_length,
                                      ignore_pad_labels=args.ignore_pad_labels)
    return tok, tr, ev


def model_config(args):
    resolve_preference(args)
    resolve_distill(args)
    cfg = apply_overrides(resolve_config(args.model_ckpt), args.model_overrides)
    if isinstance(getattr(args, "student_layers", None), tuple):
        from .models.distill import student_config
        cfg = student_config(cfg, *args.student_layers)
    if getattr(args, "gradient_checkpointing", False):
        cfg = cfg.replace(gradient_checkpointing=True)
    return cfg
