"""fp64 reference of the Adafactor recurrence (transformers ``optimization.Adafactor``, ``beta1=None``) over units of a
flat buffer, with the scalars as the kernels of csrc/adafactor.hip receive them (fp32 values widened to fp64), and the
flat test layout the GPU kernel tests share."""
import numpy as np
import torch

ALIGN = 64


def f32(x) -> float:
    """``x`` as the fp32 value a kernel argument carries, widened back to a Python float."""
    return float(np.float32(x))


class Unit:
    def __init__(self, off, rows, cols, factored, decay=False, tag=""):
        self.off, self.rows, self.cols, self.factored, self.decay, self.tag = off, rows, cols, factored, decay, tag
        self.numel = rows * cols

    @property
    def shape(self):
        return (self.rows, self.cols) if self.factored else (self.cols,)


def layout(specs):
    """``specs``: (shape, parts, tag) per flat segment.  Segments start 64-element aligned; a segment with ``parts``
    > 1 splits into equal dim-0 slices, each its own unit.  Returns (units, flat numel)."""
    units, off = [], 0
    for shape, parts, tag in specs:
        numel = int(np.prod(shape))
        assert shape[0] % parts == 0
        rows, cols = (shape[0] // parts, shape[1]) if len(shape) == 2 else (1, shape[0] // parts)
        for j in range(parts):
            units.append(Unit(off + j * rows * cols, rows, cols, len(shape) == 2, tag=f"{tag}{list(shape)}/{j}"))
        off += (numel + ALIGN - 1) // ALIGN * ALIGN
    return units, off


class RefState:
    """The recurrence's state in fp64: the weights and R / C / V per unit."""

    def __init__(self, units, w: torch.Tensor):
        self.units = units
        self.w = w.detach().double().cpu().clone()
        self.R = [torch.zeros(u.rows, dtype=torch.float64) if u.factored else None for u in units]
        self.C = [torch.zeros(u.cols, dtype=torch.float64) if u.factored else None for u in units]
        self.V = [None if u.factored else torch.zeros(u.cols, dtype=torch.float64) for u in units]

    def step(self, grad: torch.Tensor, coef, rel, beta2t, eps1=1e-30, eps2=1e-3, clip_threshold=1.0, wd=0.0,
             scale_parameter=False):
        """One step on fp32 gradients ``grad`` (flat).  Returns the per-unit update ``w_new - w_old`` (fp64)."""
        coef, rel, beta2t, eps1, eps2, clip, wd = (f32(x) for x in (coef, rel, beta2t, eps1, eps2, clip_threshold, wd))
        g_all = grad.detach().double().cpu()
        deltas = []
        for i, u in enumerate(self.units):
            g = g_all[u.off:u.off + u.numel].view(u.shape) * coef
            w = self.w[u.off:u.off + u.numel].view(u.shape)
            lr_t = rel * max(eps2, float(w.pow(2).mean().sqrt())) if scale_parameter else rel
            s = g * g + eps1
            if u.factored:
                self.R[i] = beta2t * self.R[i] + (1.0 - beta2t) * s.mean(dim=1)
                self.C[i] = beta2t * self.C[i] + (1.0 - beta2t) * s.mean(dim=0)
                upd = g * (self.R[i] / self.R[i].mean()).rsqrt().unsqueeze(1) * self.C[i].rsqrt().unsqueeze(0)
            else:
                self.V[i] = beta2t * self.V[i] + (1.0 - beta2t) * s
                upd = g * self.V[i].rsqrt()
            upd = upd / max(1.0, float(upd.pow(2).mean().sqrt()) / clip)
            old = w.clone()
            if u.decay:
                w.sub_(w * (wd * lr_t))
            w.sub_(upd * lr_t)
            deltas.append(w - old)
        return deltas


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """Largest elementwise relative error of a positive statistic."""
    got = got.detach().double().cpu()
    return float(((got - ref).abs() / ref.abs()).max())
