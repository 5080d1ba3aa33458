"""fp64 references and error metrics for the row-wise (memory-bound) kernels: norm, activation, dropout, AdamW.

Plain torch in float64, written from the operations' definitions (not from the kernels): the oracle of
tests/test_rowwise_kernels_gpu.py, itself validated on the CPU by tests/test_rowwise_refs_cpu.py against the package's
fp32 composites and ``torch.optim.AdamW``.  Not a conftest: imported by name.
"""
import math

import torch

RMS, LAYER = 0, 1
TINY = 1e-300

# Bounds (one place).  bf16 rows: the suite's 2e-2, ~5x one bf16 rounding (2^-8) of an fp32 result.  fp32 rows: the
# fp32-vs-fp64 bound of tests/test_grads_gpu.py.  fp32 column sums: error against the column's L1 mass (the form of
# test_colsum_partials_acc); one dropped / doubled row of N <= 6150 moves a column by ~1/N >= 1.6e-4 of that mass.
ROW_BOUND = {torch.bfloat16: 2e-2, torch.float32: 1e-5}
COL_BOUND = 1e-5
BF16_ACC_BOUND = 1e-2


# ----------------------------------------------------------------------------------------------------------- metrics
def row_err(got, ref):
    """max over rows of ||got_r - ref_r|| / (||ref_r|| + tiny); rows = all leading dims."""
    g = got.detach().double().reshape(-1, got.shape[-1])
    r = ref.detach().double().reshape(-1, ref.shape[-1])
    assert g.shape == r.shape, (g.shape, r.shape)
    return ((g - r).norm(dim=1) / (r.norm(dim=1) + TINY)).max().item()


def col_err(got, ref, mass):
    """max over columns of |got - ref| / sum_r |term_r| (``mass``: the L1 mass of the column's terms)."""
    return ((got.detach().double() - ref).abs() / mass.clamp_min(TINY)).max().item()


def acc_err(got, ref):
    """|got - ref| / max(|ref|, 1): a sum stored in bf16 (the store's rounding)."""
    return ((got.detach().double() - ref).abs() / ref.abs().clamp_min(1.0)).max().item()


def rel_l2(got, ref):
    return ((got.detach().double() - ref.double()).norm() / (ref.double().norm() + TINY)).item()


def elem_err(got, ref, slack=0.0):
    """max (|got - ref| - slack |ref|)+ / (|ref| + rms(ref)): no single element (one 4- or 8-wide group) can hide in a
    global norm, and an element that cancels to ~0 is measured against the tensor's scale.  ``slack``: the relative
    rounding of a low-precision store (2^-8 for bf16), allowed on top."""
    r = ref.double()
    err = ((got.detach().double() - r).abs() - slack * r.abs()).clamp_min(0.0)
    return (err / (r.abs() + r.pow(2).mean().sqrt() + TINY)).max().item()


def nonzero_randn(*shape, device, dtype, lo=0.01, hi=4.0, generator=None):
    """randn with lo <= |x| <= hi, so a zero in a dropout output can only be a dropped element."""
    x = torch.randn(*shape, device=device, generator=generator)
    x = torch.where(x < 0, -1.0, 1.0) * x.abs().clamp(lo, hi)
    return x.to(dtype)


# -------------------------------------------------------------------------------------------------------------- norm
def _stats(sd, kind, eps):
    if kind == LAYER:
        xc = sd - sd.mean(-1, keepdim=True)
    else:
        xc = sd
    rstd = torch.rsqrt(xc.pow(2).mean(-1, keepdim=True) + eps)
    return xc * rstd, rstd


def norm_fwd_ref(x, resid, w, b, eps, p, keep, kind):
    """(out, s) in fp64.  s = (resid +) dropout(x) exact; out = norm of s as STORED (rounded to x.dtype whenever the op
    stores it, i.e. with a residual or dropout) times w (+ b)."""
    xd = x.double()
    if p > 0.0:
        xd = torch.where(keep, xd / (1.0 - p), torch.zeros_like(xd))
    s = xd + resid.double() if resid is not None else xd
    stored = s.to(x.dtype).double() if (resid is not None or p > 0.0) else s
    xh, _ = _stats(stored, kind, eps)
    out = xh * w.double()
    if kind == LAYER and b is not None:
        out = out + b.double()
    return out, s


def norm_bwd_ref(s, w, dout, ds_extra, eps, p, keep, kind):
    """Backward of out = norm(s) * w (+ b), s = (resid +) dropout(x), from the stored s, in fp64.

    dstream = d loss / d s (= d resid) = norm_bwd(dout) + ds_extra;  dx = dropout_bwd(dstream);  dw = sum_r dout * xhat,
    db = sum_r dout, dxs = sum_r dx, each with the L1 mass of its terms."""
    sd, wd = s.double(), w.double()
    xh, rstd = _stats(sd, kind, eps)
    dy = dout.double() if dout is not None else torch.zeros_like(sd)
    g = dy * wd
    s2 = (g * xh).mean(-1, keepdim=True)
    s1 = g.mean(-1, keepdim=True) if kind == LAYER else 0.0
    ds = (g - s1 - xh * s2) * rstd
    if ds_extra is not None:
        ds = ds + ds_extra.double()
    dx = torch.where(keep, ds / (1.0 - p), torch.zeros_like(ds)) if p > 0.0 else ds
    t = dy * xh
    return {"dstream": ds, "dx": dx, "dw": t.sum(0), "dw_mass": t.abs().sum(0), "db": dy.sum(0),
            "db_mass": dy.abs().sum(0), "dxs": dx.sum(0), "dxs_mass": dx.abs().sum(0)}


# -------------------------------------------------------------------------------------------------------- activation
def act64(x, act):
    if act == "relu":
        return torch.relu(x)
    if act == "gelu":
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if act == "gelu_new":
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)))
    if act == "silu":
        return x * torch.sigmoid(x)
    raise ValueError(act)


def act_ref(x, act, gated, p, keep, dy=None):
    """(y, dx, y_nodrop, dx_nodrop) in fp64: y = dropout(act(x[:, :F]) * x[:, F:]) (gated) or dropout(act(x)); dx its
    gradient for the output gradient dy (autograd in fp64).  The *_nodrop pair is the same without dropout (its zeros
    are the zeros the activation itself produces, e.g. relu of a negative input)."""
    xd = x.detach().double().requires_grad_(True)
    if gated:
        f = xd.shape[-1] // 2
        y0 = act64(xd[..., :f], act) * xd[..., f:]
    else:
        y0 = act64(xd, act)
    y = y0 * keep.double() / (1.0 - p) if p > 0.0 else y0
    if dy is None:
        return y.detach(), None, y0.detach(), None
    (dx,) = torch.autograd.grad(y, xd, dy.double(), retain_graph=p > 0.0)
    dx0 = torch.autograd.grad(y0, xd, dy.double())[0] if p > 0.0 else dx
    return y.detach(), dx, y0.detach(), dx0


# ------------------------------------------------------------------------------------------------------------- AdamW
def f32(v):
    """The value a float argument has once the kernel receives it (fp32)."""
    return float(torch.tensor(float(v), dtype=torch.float32).item())


def adamw_ref(w, g, m, v, mask, coef, lr, b1, b2, eps, wd, step, f32_scalars=True):
    """One decoupled-weight-decay Adam step (Loshchilov & Hutter; torch.optim.AdamW) in fp64, not in place:
    w *= 1 - lr*wd*mask;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  w -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps),
    g pre-multiplied by the clip coefficient, bc = 1 - beta^step from the exact betas.  ``f32_scalars``: the scalars as
    the kernel receives them (lr, betas, eps, wd, coef rounded to fp32); False: exact doubles."""
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    if f32_scalars:
        coef, lr, b1, b2, eps, wd, bc1, bc2 = (f32(t) for t in (coef, lr, b1, b2, eps, wd, bc1, bc2))
    w, g, m, v = w.double(), g.double() * coef, m.double(), v.double()
    dec = lr * wd * (mask.double() if mask is not None else 1.0)
    w = w * (1.0 - dec)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    w = w - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return w, m, v
