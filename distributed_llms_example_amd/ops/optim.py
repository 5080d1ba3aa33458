"""Fused AdamW + global-norm gradient clipping over the flat parameter space.

Semantics = ``torch.optim.AdamW`` (decoupled weight decay, bias-corrected moments; the Trainer
builds it with ``fused=True``, transformers trainer_optimizer.py:202-207, the custom loops with the
foreach default, ref/train-accelerator.py:187) preceded by ``clip_grad_norm_(max_norm)``
(transformers trainer.py:2535-2539): ``coef = min(1, max_norm / (||g|| + 1e-6))``.

MI355X design: parameters live in bf16 (what the GEMMs read), the optimizer keeps fp32 master
weights + fp32 moments, all as flat buffers (parallel/flat.py).  One reduction kernel computes
||g||² into a device scalar, and ONE elementwise kernel (csrc/adamw.hip) reads that scalar, so the
step never synchronises with the host (no ``.item()``).  The grad-norm is returned as a device
tensor for logging.
"""
from __future__ import annotations

import math

import torch

from .. import _ext
from ..parallel.flat import FlatParams


class FusedAdamW:
    def __init__(self, flat: FlatParams, lr: float = 5e-5, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, no_decay=None, master_weights: bool | None = None):
        self.flat = flat
        self.lr = lr
        self.betas = betas
        self.eps = eps
        self.weight_decay = weight_decay
        self.step_count = 0
        if master_weights is None:
            master_weights = flat.dtype != torch.float32
        self.master = flat.param_buf.float().clone() if master_weights else None
        self.exp_avg = torch.zeros(flat.numel, dtype=torch.float32, device=flat.device)
        self.exp_avg_sq = torch.zeros(flat.numel, dtype=torch.float32, device=flat.device)
        self.wd_mask = flat.decay_mask(no_decay) if (no_decay is not None and weight_decay != 0.0) else None
        if no_decay is not None and weight_decay != 0.0 and self.wd_mask is None:
            # uniform: either all decay or none
            if all(no_decay(s.name) for s in flat.segments):
                self.weight_decay = 0.0
        for attr in ("master", "exp_avg", "exp_avg_sq", "wd_mask"):
            flat.register_companion(self, attr)  # kept in step with a reducer-driven relayout (parallel/flat.py)
        self._one = torch.ones((), dtype=torch.float32, device=flat.device)
        # param_groups-like view for schedulers / logging parity with torch optimizers
        self.param_groups = [{"lr": lr, "initial_lr": lr, "weight_decay": weight_decay, "betas": betas, "eps": eps}]

    # ------------------------------------------------------------------------------------------
    def grad_norm(self) -> torch.Tensor:
        g = self.flat.grad_buf
        if _ext.use_native(g):
            return _ext.native().sq_norm(g).sqrt()
        return torch.linalg.vector_norm(g.float())

    def state_bytes(self) -> int:
        """Bytes of optimizer state: two fp32 moments, the fp32 master and the decay mask."""
        return sum(t.numel() * t.element_size() for t in (self.exp_avg, self.exp_avg_sq, self.master, self.wd_mask)
                   if t is not None)

    def device_hyper(self, t: torch.Tensor, lr) -> torch.Tensor:
        """[lr, lr / bc1, 1 / sqrt(bc2)] as a device tensor from a device step count ``t`` (float, already incremented)
        and ``lr`` (float or device scalar): the AdamW kernel reads it instead of host floats, so a captured graph
        replays with the right bias corrections and learning rate every step."""
        b1, b2 = self.betas
        lr_t = lr if torch.is_tensor(lr) else torch.full_like(t, float(lr))
        bc1 = 1.0 - torch.pow(torch.full_like(t, b1), t)
        bc2 = 1.0 - torch.pow(torch.full_like(t, b2), t)
        return torch.stack([lr_t, lr_t / bc1, torch.rsqrt(bc2)]).reshape(3).float().contiguous()

    @torch.no_grad()
    def step(self, max_grad_norm: float | None = None, hyper: torch.Tensor | None = None) -> torch.Tensor | None:
        """One clip + AdamW update.  ``hyper`` (device_hyper) replaces the host lr / bias corrections (graph mode)."""
        lr = self.param_groups[0]["lr"]
        self.step_count += 1
        norm = None
        coef = self._one
        if max_grad_norm is not None and max_grad_norm > 0:
            norm = self.grad_norm()
            coef = torch.clamp(max_grad_norm / (norm + 1e-6), max=1.0)
        b1, b2 = self.betas
        bc1 = 1.0 - b1 ** self.step_count
        bc2 = 1.0 - b2 ** self.step_count
        p = self.flat.param_buf
        g = self.flat.grad_buf
        if _ext.use_native(p):
            _ext.native().adamw_step(p, self.master, g, self.exp_avg, self.exp_avg_sq, self.wd_mask, coef, float(lr),
                                     float(b1), float(b2), float(self.eps), float(self.weight_decay), float(bc1),
                                     float(bc2), hyper)
        else:
            if hyper is not None:
                lr, bc1, bc2 = float(hyper[0]), float(hyper[0] / hyper[1]), float(1.0 / hyper[2] ** 2)
            self._reference_step(p, g, coef, lr, b1, b2, bc1, bc2)
        return norm

    def _reference_step(self, p, g, coef, lr, b1, b2, bc1, bc2):
        master = self.master if self.master is not None else p
        gf = g.float() * coef
        if self.weight_decay != 0.0:
            if self.wd_mask is None:
                master.mul_(1.0 - lr * self.weight_decay)
            else:
                master.sub_(master * self.wd_mask.float() * (lr * self.weight_decay))
        self.exp_avg.lerp_(gf, 1.0 - b1)
        self.exp_avg_sq.mul_(b2).addcmul_(gf, gf, value=1.0 - b2)
        denom = (self.exp_avg_sq.sqrt() / math.sqrt(bc2)).add_(self.eps)
        master.addcdiv_(self.exp_avg, denom, value=-lr / bc1)
        if self.master is not None:
            p.copy_(master)

    def zero_grad(self, set_to_none: bool = False) -> None:
        self.flat.zero_grad()

    # ------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """Flat state in the model's canonical (construction) segment order, whatever the current layout."""
        f = self.flat
        can = f.to_canonical
        return {"step": self.step_count, "exp_avg": can(self.exp_avg), "exp_avg_sq": can(self.exp_avg_sq),
                "master": can(self.master) if self.master is not None else None, "lr": self.param_groups[0]["lr"],
                "betas": list(self.betas), "eps": self.eps, "weight_decay": self.weight_decay,
                "layout": [{"name": n, "numel": s.numel} for n, s in
                           zip(f.canonical, sorted(f.segments, key=lambda s: f.canonical.index(s.name)))]}

    def load_state_dict(self, d: dict) -> None:
        if d.get("kind", "adamw") != "adamw":
            raise ValueError(f"optimizer state of kind {d.get('kind')!r} cannot be loaded into FusedAdamW")
        f = self.flat
        by_name = {s.name: s.numel for s in f.segments}
        if [s["numel"] for s in d["layout"]] != [by_name.get(n) for n in f.canonical]:
            raise ValueError("optimizer state layout does not match the model")
        self.step_count = int(d["step"])
        self.exp_avg.copy_(f.from_canonical(d["exp_avg"].to(self.exp_avg.device)))
        self.exp_avg_sq.copy_(f.from_canonical(d["exp_avg_sq"].to(self.exp_avg_sq.device)))
        if self.master is not None and d.get("master") is not None:
            self.master.copy_(f.from_canonical(d["master"].to(self.master.device)))
            self.flat.param_buf.copy_(self.master)
        self.param_groups[0]["lr"] = d.get("lr", self.param_groups[0]["lr"])


# ------------------------------------------------------------------------------------------------ Adafactor
_warned_composite = [False]


class FusedAdafactor:
    """Adafactor with factored second moments and no first moment over the flat parameter space.

    Semantics = ``transformers.optimization.Adafactor`` with ``beta1=None``, preceded by the same global-norm clip as
    :class:`FusedAdamW`.  Every formula applies per UNIT: one transformers parameter.  Our parameters are
    concatenations of transformers' along dim 0 (``qkv``, ``kv``, gated ``wi``, BART's fused projections and their 1-D
    biases), so ``parts(name)`` says into how many equal dim-0 slices a flat segment splits — or, where the slices
    differ (T5Gemma's qkv with grouped K/V heads: q, then the shorter k and v), their dim-0 sizes in order; each slice
    has its own
    ``C``, its own ``mean(R)``, its own ``rms(u)`` clip and its own ``rms(w)``.  State per unit: ``R[rows]`` and
    ``C[cols]`` for matrices, ``V[numel]`` for 1-D tensors, kept in canonical unit order in ``self.rv`` / ``self.c`` —
    not flat-indexed, so a relayout of the flat buffers moves nothing in them; only the device unit table
    (csrc/adafactor_params.h) is rebuilt from the new segment offsets.  The fp32 master is a flat companion as in AdamW.

    On the GPU one call of csrc/adafactor.hip runs the step in five launches whatever the number of parameters (route
    ``adafactor`` = fused); ``_reference_step`` is the torch composite over units: the CPU path, the test oracle, and
    what ``adafactor=composite`` / ``DLLM_REFERENCE_OPS=1`` select.
    """

    def __init__(self, flat: FlatParams, lr: float | None = None, eps=(1e-30, 1e-3), clip_threshold: float = 1.0,
                 decay_rate: float = -0.8, beta1=None, weight_decay: float = 0.0, scale_parameter: bool = True,
                 relative_step: bool = True, warmup_init: bool = False, no_decay=None,
                 master_weights: bool | None = None, parts=None):
        if beta1 is not None:
            raise ValueError("FusedAdafactor: beta1 (a first moment) is not supported; pass beta1=None")
        if lr is not None and relative_step:
            raise ValueError("Cannot combine manual `lr` and `relative_step=True` options")
        if lr is None and not relative_step:
            raise ValueError("FusedAdafactor: relative_step=False needs a learning rate")
        if warmup_init and not relative_step:
            raise ValueError("`warmup_init=True` requires `relative_step=True`")
        self.flat = flat
        self.eps = (float(eps[0]), float(eps[1]))
        self.clip_threshold = float(clip_threshold)
        self.decay_rate = float(decay_rate)
        self.weight_decay = float(weight_decay)
        self.scale_parameter = bool(scale_parameter)
        self.relative_step = bool(relative_step)
        self.warmup_init = bool(warmup_init)
        self.step_count = 0
        if master_weights is None:
            master_weights = flat.dtype != torch.float32
        self.master = flat.param_buf.float().clone() if master_weights else None
        flat.register_companion(self, "master")
        parts = parts or (lambda name: 1)
        shape_of = {s.name: s.shape for s in flat.segments}
        self.units: list[dict] = []  # canonical order: segments as constructed, their slices in order
        rv_off = c_off = 0
        for name in flat.canonical:
            shape, k = shape_of[name], parts(name)
            if len(shape) > 2 or len(shape) == 0:
                raise NotImplementedError(f"FusedAdafactor: parameter {name} has {len(shape)} dims (1 or 2 are served)")
            if isinstance(k, (list, tuple)):  # the slices' dim-0 sizes
                sizes = [int(x) for x in k]
                if not sizes or min(sizes) < 1 or sum(sizes) != shape[0]:
                    raise ValueError(f"FusedAdafactor: {name} {tuple(shape)} does not split into dim-0 slices of "
                                     f"{sizes}")
            else:
                k = int(k)
                if k < 1 or shape[0] % k:
                    raise ValueError(f"FusedAdafactor: {name} {tuple(shape)} does not split into {k} equal dim-0 "
                                     "slices")
                sizes = [shape[0] // k] * k
            decay = self.weight_decay != 0.0 and not (no_decay is not None and no_decay(name))
            first = 0  # the slice's first dim-0 index
            for j, size in enumerate(sizes):
                rows, cols = (size, shape[1]) if len(shape) == 2 else (1, size)
                u = {"name": name, "part": j, "rows": rows, "cols": cols, "factored": len(shape) == 2, "rv": rv_off,
                     "c": c_off if len(shape) == 2 else -1, "decay": decay,
                     "start": first * (shape[1] if len(shape) == 2 else 1)}  # element offset inside the segment
                first += size
                self.units.append(u)
                # 4-element aligned so the kernels may use 16-byte access on the state
                rv_off += ((rows if u["factored"] else cols) + 3) // 4 * 4
                if u["factored"]:
                    c_off += (cols + 3) // 4 * 4
        dev = flat.device
        self.rv = torch.zeros(max(rv_off, 4), dtype=torch.float32, device=dev)
        self.c = torch.zeros(max(c_off, 4), dtype=torch.float32, device=dev)
        self._one = torch.ones((), dtype=torch.float32, device=dev)
        self._table_version = None  # flat.layout_version the device table was built for
        self._table = self._table_host = self._scratch = None
        lr0 = 0.0 if lr is None else lr  # relative_step: the step size comes from the step count, "lr" is unused
        self.param_groups = [{"lr": lr0, "initial_lr": lr0, "weight_decay": weight_decay, "eps": self.eps,
                              "clip_threshold": clip_threshold, "decay_rate": decay_rate, "beta1": None,
                              "scale_parameter": scale_parameter, "relative_step": relative_step,
                              "warmup_init": warmup_init}]

    # ------------------------------------------------------------------------------------------
    def grad_norm(self) -> torch.Tensor:
        from . import routing
        g = self.flat.grad_buf
        if _ext.use_native(g) and routing.get("adafactor") == "fused":  # the composite route runs no native call
            return _ext.native().sq_norm(g).sqrt()
        return torch.linalg.vector_norm(g.float())

    def state_bytes(self) -> int:
        """Bytes of optimizer state: R + C per matrix unit, V per 1-D unit, and the fp32 master."""
        n = sum(u["rows"] + u["cols"] if u["factored"] else u["cols"] for u in self.units) * 4
        return n + (self.master.numel() * 4 if self.master is not None else 0)

    def _offsets(self) -> list[int]:
        """Flat element offset of every unit under the current layout."""
        seg = {s.name: s.offset for s in self.flat.segments}
        return [seg[u["name"]] + u["start"] for u in self.units]

    def _rel(self, t: int, lr: float) -> float:
        if not self.relative_step:
            return float(lr)
        return min(1e-6 * t if self.warmup_init else 1e-2, 1.0 / math.sqrt(t))

    def device_hyper(self, t: torch.Tensor, lr) -> torch.Tensor:
        """[rel, beta2t] as a device tensor from a device step count ``t`` (float, already incremented) and ``lr``
        (float or device scalar; unused under relative_step): the kernels read it instead of host floats, so a
        captured graph replays with the right decay and step size every step."""
        beta2t = 1.0 - torch.pow(t, self.decay_rate)
        if self.relative_step:
            floor = 1e-6 * t if self.warmup_init else torch.full_like(t, 1e-2)
            rel = torch.minimum(floor, torch.rsqrt(t))
        else:
            rel = lr if torch.is_tensor(lr) else torch.full_like(t, float(lr))
        return torch.stack([rel.reshape(()), beta2t.reshape(())]).float().contiguous()

    def _fused(self, p: torch.Tensor, g: torch.Tensor) -> bool:
        from . import routing
        if not _ext.use_native(p) or routing.get("adafactor") != "fused":
            return False
        served = g.dtype == torch.float32 and ((p.dtype == torch.bfloat16 and self.master is not None) or
                                               (p.dtype == torch.float32 and self.master is None))
        if not served and not _warned_composite[0]:
            _warned_composite[0] = True
            import warnings
            warnings.warn("FusedAdafactor: the fused kernels serve fp32 gradients with bf16 parameters + fp32 master or "
                          f"fp32 parameters; {g.dtype} gradients / {p.dtype} parameters take the torch composite")
        return served

    def _ensure_table(self) -> None:
        """(Re)build the device unit table when the flat layout changed.  Tile order and scratch offsets depend on the
        unit shapes only, so a relayout rewrites the table's offsets in place: pointers captured in a graph stay."""
        f = self.flat
        if self._table_version == f.layout_version:
            return
        C = _ext.native()
        rows = [[off, u["rows"], u["cols"], u["rv"], u["c"], int(u["decay"])]
                for off, u in zip(self._offsets(), self.units)]
        host, n_tiles, colpart, rowpart = C.adafactor_plan(torch.tensor(rows, dtype=torch.int64))
        if self._table is None:
            dev = f.device
            self._table = torch.empty_like(host, device=dev)
            new = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
            # per-unit scalars, column partials, row partials, per-tile partials (sum u^2 | sum w^2): allocated once
            self._scratch = (new(4 * len(self.units)), new(colpart), new(rowpart), new(2 * n_tiles))
        self._table.copy_(host)
        self._table_host = host
        self._table_version = f.layout_version

    @torch.no_grad()
    def step(self, max_grad_norm: float | None = None, hyper: torch.Tensor | None = None) -> torch.Tensor | None:
        """One clip + Adafactor update.  ``hyper`` (device_hyper) replaces the host step size / decay (graph mode)."""
        lr = self.param_groups[0]["lr"]
        self.step_count += 1
        t = self.step_count
        norm = None
        coef = self._one
        if max_grad_norm is not None and max_grad_norm > 0:
            norm = self.grad_norm()
            coef = torch.clamp(max_grad_norm / (norm + 1e-6), max=1.0)
        beta2t = 1.0 - math.pow(t, self.decay_rate)
        rel = self._rel(t, lr)
        p, g = self.flat.param_buf, self.flat.grad_buf
        if self._fused(p, g):
            self._ensure_table()
            scal, colpart, rowpart, tpart = self._scratch
            _ext.native().adafactor_step(p, self.master, g, self.rv, self.c, self._table, self._table_host, scal,
                                         colpart, rowpart, tpart, coef, float(rel), float(beta2t), self.eps[0],
                                         self.eps[1], self.clip_threshold, self.weight_decay, self.scale_parameter,
                                         hyper)
        else:
            if hyper is not None:
                rel, beta2t = (hyper[0], hyper[1]) if hyper.is_cuda else (float(hyper[0]), float(hyper[1]))
            self._reference_step(p, g, coef, rel, beta2t)
        return norm

    @staticmethod
    def _rms(x: torch.Tensor) -> torch.Tensor:
        return x.norm(2) / (x.numel() ** 0.5)

    @staticmethod
    def _blend(state: torch.Tensor, new: torch.Tensor, beta2t) -> None:
        if torch.is_tensor(beta2t):
            state.mul_(beta2t).add_(new * (1.0 - beta2t))
        else:
            state.mul_(beta2t).add_(new, alpha=1.0 - beta2t)

    def _reference_step(self, p, g, coef, rel, beta2t):
        """The torch composite, unit by unit, in the operation order of transformers' Adafactor.step."""
        master = self.master if self.master is not None else p
        gf = g.float() * coef
        eps1, eps2 = self.eps
        for off, u in zip(self._offsets(), self.units):
            rows, cols = u["rows"], u["cols"]
            n = rows * cols
            shape = (rows, cols) if u["factored"] else (cols,)
            grad = gf[off:off + n].view(shape)
            w = master[off:off + n].view(shape)
            wf = w.float()
            lr_t = rel * torch.clamp(self._rms(wf), min=eps2) if self.scale_parameter else rel
            upd = grad ** 2 + eps1
            if u["factored"]:
                R = self.rv[u["rv"]:u["rv"] + rows]
                Cc = self.c[u["c"]:u["c"] + cols]
                self._blend(R, upd.mean(dim=-1), beta2t)
                self._blend(Cc, upd.mean(dim=-2), beta2t)
                r_factor = (R / R.mean(dim=-1, keepdim=True)).rsqrt_().unsqueeze(-1)
                upd = (r_factor * Cc.unsqueeze(-2).rsqrt()).mul_(grad)
            else:
                V = self.rv[u["rv"]:u["rv"] + cols]
                self._blend(V, upd, beta2t)
                upd = V.rsqrt().mul_(grad)
            upd.div_((self._rms(upd) / self.clip_threshold).clamp_(min=1.0))
            upd.mul_(lr_t)
            if u["decay"]:
                wf = wf - wf * (self.weight_decay * lr_t)
            w.copy_(wf - upd)
        if self.master is not None:
            p.copy_(master)

    def zero_grad(self, set_to_none: bool = False) -> None:
        self.flat.zero_grad()

    # ------------------------------------------------------------------------------------------
    def _layout(self) -> list[dict]:
        return [{"name": u["name"], "part": u["part"], "rows": u["rows"], "cols": u["cols"],
                 "factored": u["factored"]} for u in self.units]

    def _gather(self, kind: str) -> torch.Tensor:
        """R, C or V of every unit that has one, concatenated in canonical unit order (no padding)."""
        out = []
        for u in self.units:
            if kind == "R" and u["factored"]:
                out.append(self.rv[u["rv"]:u["rv"] + u["rows"]])
            elif kind == "C" and u["factored"]:
                out.append(self.c[u["c"]:u["c"] + u["cols"]])
            elif kind == "V" and not u["factored"]:
                out.append(self.rv[u["rv"]:u["rv"] + u["cols"]])
        return torch.cat(out).clone() if out else torch.zeros(0, dtype=torch.float32, device=self.rv.device)

    def _scatter(self, kind: str, t: torch.Tensor) -> None:
        at = 0
        for u in self.units:
            if kind == "R" and u["factored"]:
                buf, o, n = self.rv, u["rv"], u["rows"]
            elif kind == "C" and u["factored"]:
                buf, o, n = self.c, u["c"], u["cols"]
            elif kind == "V" and not u["factored"]:
                buf, o, n = self.rv, u["rv"], u["cols"]
            else:
                continue
            buf[o:o + n].copy_(t[at:at + n])
            at += n
        if at != t.numel():
            raise ValueError(f"optimizer state {kind} has {t.numel()} elements, the model needs {at}")

    def state_dict(self) -> dict:
        """State in canonical unit order, whatever the current flat layout."""
        f = self.flat
        return {"kind": "adafactor", "step": self.step_count, "R": self._gather("R"), "C": self._gather("C"),
                "V": self._gather("V"), "master": f.to_canonical(self.master) if self.master is not None else None,
                "lr": self.param_groups[0]["lr"], "weight_decay": self.weight_decay, "layout": self._layout()}

    def load_state_dict(self, d: dict) -> None:
        if d.get("kind") != "adafactor":
            raise ValueError(f"optimizer state of kind {d.get('kind', 'adamw')!r} cannot be loaded into FusedAdafactor")
        if list(d["layout"]) != self._layout():
            raise ValueError("optimizer state layout does not match the model")
        self.step_count = int(d["step"])
        for kind in ("R", "C", "V"):
            self._scatter(kind, d[kind].to(self.rv.device))
        if self.master is not None and d.get("master") is not None:
            self.master.copy_(self.flat.from_canonical(d["master"].to(self.master.device)))
            self.flat.param_buf.copy_(self.master)
        self.param_groups[0]["lr"] = d.get("lr", self.param_groups[0]["lr"])
