"""fp64 reference, bf16 error model, case builder and error metrics for the attention kernels (csrc/attn.hip,
attn_hd.hip, attn_f32.hip).

``attn_ref`` is plain torch in float64 written from the contract in csrc/attn_params.h (visibility per key, causal
bottom-right aligned, a row without a visible key gives a zero output row, LSE = +inf and no gradient), with the
backward as explicit formulas (no autograd) — not from ``ops.attention._reference``, which tests/test_attn_refs_cpu.py
compares it with. It is the oracle of tests/test_attn_rows_gpu.py. ``attn_bf16_model`` is the same math with values
rounded to bf16 where the kernels round them: the error the design permits, from which the GPU tests take their bounds
(4 x). Not a conftest: imported by name.
"""
import math
import types

import torch

from distributed_llms_example_amd.ops import attention as A
from distributed_llms_example_amd.ops.rng import rowwise_keep_mask

TINY = 1e-300
LN2 = math.log(2.0)
BF16 = torch.bfloat16
# the loosest attention-gradient bound the suite has used at more than one query row: 4 x the model's row error of every
# GPU case must fit under it (tests/test_attn_refs_cpu.py), so no kernel bound derived from the model exceeds it
ROW_CAP = 5e-2
MODEL_FACTOR = 4.0  # accumulation order, online-softmax rescaling, exp2 vs exp, fp32 partial sums: not in the model
LSE_BOUND = 1e-3    # log2 units: fp32 arithmetic on bf16 products


# ----------------------------------------------------------------------------------------------------------- metrics
def row_err(got, ref):
    """max over rows (all leading dims of [B, S, H, D]) of ||got - ref|| / (||ref|| + 1e-3 * rms row norm): no row can
    hide in a whole-tensor norm, and a row that cancels to ~0 is measured against the tensor's typical row."""
    g = got.detach().double().reshape(-1, got.shape[-1])
    r = ref.detach().double().reshape(-1, ref.shape[-1])
    assert g.shape == r.shape, (g.shape, r.shape)
    rn = r.norm(dim=1)
    return ((g - r).norm(dim=1) / (rn + 1e-3 * rn.pow(2).mean().sqrt() + TINY)).max().item()


def mass_err(got, ref, mass):
    """max over entries of |got - ref| / sum |term| (``mass``: the L1 mass of the entry's terms, as
    rowwise_refs.col_err); an entry without terms must be exactly 0."""
    return ((got.detach().double() - ref).abs() / mass.clamp_min(TINY)).max().item()


def rel_l2(got, ref):
    return ((got.detach().double() - ref.double()).norm() / (ref.double().norm() + TINY)).item()


def _bf(x):
    return x.to(BF16).double()


# --------------------------------------------------------------------------------------------------------- reference
def visible(B, Sq, Sk, causal, kpm, device):
    """bool [B, 1, Sq, Sk]: key j is visible to query i iff kpm[b][j] != 0 (if given) and, causal, j <= i + Sk - Sq."""
    vis = torch.ones(B, 1, Sq, Sk, dtype=torch.bool, device=device)
    if kpm is not None:
        vis = vis & (kpm != 0).view(B, 1, 1, Sk)
    if causal:
        i = torch.arange(Sq, device=device).view(Sq, 1)
        j = torch.arange(Sk, device=device).view(1, Sk)
        vis = vis & (j <= i + (Sk - Sq))
    return vis


def _rel_index(Sq, Sk, device):
    return (torch.arange(Sk, device=device).view(1, Sk) - torch.arange(Sq, device=device).view(Sq, 1) + (Sq - 1))


def _attn64(q, k, v, do, scale, causal, kpm, lut, p, keep, model, fwd_only=False, phase=1.0, pre_scale=False):
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    dev = q.device
    qd, kd, vd, dod = (t.double().permute(0, 2, 1, 3) for t in (q, k, v, do))  # [B, H, S, D]
    s = torch.matmul(qd, kd.transpose(-1, -2)) * scale
    rel = _rel_index(Sq, Sk, dev)
    if lut is not None:
        s = s + lut.double()[:, rel].unsqueeze(0)
    vis = visible(B, Sq, Sk, causal, kpm, dev)
    s = s.masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    empty = torch.isneginf(m)
    m = torch.where(empty, torch.zeros_like(m), m)
    e = torch.exp(s - m)  # masked keys: exactly 0
    del s
    l = e.sum(-1, keepdim=True)
    linv = torch.where(empty, torch.zeros_like(l), 1.0 / l.clamp_min(TINY))
    lse2 = torch.where(empty, torch.full_like(l, float("inf")), (m + torch.log(l.clamp_min(TINY))) / LN2).squeeze(-1)
    kscale = keep.double() / (1.0 - p) if p > 0.0 else None
    pr = e * linv
    if model:  # forward: exp(s - max) rounded to bf16 for the PV product, the row sum taken from the unrounded values
        if pre_scale and p > 0.0:  # csrc/attn_hd.hip: keep / (1 - p) applied before the rounding
            o = torch.matmul(_bf(e * kscale * phase) / phase, vd) * linv
        else:
            eh = _bf(e * phase) / phase
            o = torch.matmul(eh * kscale if p > 0.0 else eh, vd) * linv
        o = _bf(o)
    else:
        o = torch.matmul(pr * kscale if p > 0.0 else pr, vd)
    del e
    if fwd_only:
        return types.SimpleNamespace(o=o.permute(0, 2, 1, 3).contiguous(), lse2=lse2, row_empty=empty.squeeze(-1))
    ph = pr * kscale if p > 0.0 else pr
    dv = torch.matmul((_bf(ph) if model else ph).transpose(-1, -2), dod)
    del ph
    dp = torch.matmul(dod, vd.transpose(-1, -2))
    delta = (dod * o).sum(-1, keepdim=True)  # model: from the stored (bf16) o
    ds = pr * ((dp * kscale if p > 0.0 else dp) - delta)
    del dp, pr
    dsh = _bf(ds) if model else ds
    dq = scale * torch.matmul(dsh, kd)
    dk = scale * torch.matmul(dsh.transpose(-1, -2), qd)
    del dsh
    out = types.SimpleNamespace(lse2=lse2, row_empty=empty.squeeze(-1))  # [B, H, Sq]
    if lut is not None:  # sums of the unrounded dS (the kernels sum fp32 dS before packing it)
        L = Sq + Sk - 1
        idx = rel.reshape(-1)
        out.dlut = torch.zeros(H, L, dtype=torch.float64, device=dev).index_add_(1, idx, ds.sum(0).reshape(H, -1))
        out.dlut_mass = torch.zeros(H, L, dtype=torch.float64, device=dev).index_add_(
            1, idx, ds.abs().sum(0).reshape(H, -1))
    del ds
    back = lambda t: t.permute(0, 2, 1, 3).contiguous()  # [B, S, H, D]
    out.o, out.dq, out.dk, out.dv = back(o), back(dq), back(dk), back(dv)
    if model:
        out.dq, out.dk, out.dv = _bf(out.dq), _bf(out.dk), _bf(out.dv)
    for n in ("dq", "dk", "dv"):  # column sums over tokens of the (model: stored) gradients, [H * D]
        t = getattr(out, n)
        setattr(out, "cs_" + n, t.sum((0, 1)).reshape(-1))
        setattr(out, "cs_" + n + "_mass", t.abs().sum((0, 1)).reshape(-1))
    out.key_dead = ~vis.any(-2).squeeze(1)  # [B, Sk]: visible to no query -> dk = dv = 0 exactly
    return out


_SUM = ("dlut", "dlut_mass", "cs_dq", "cs_dq_mass", "cs_dk", "cs_dk_mass", "cs_dv", "cs_dv_mass")
_CAT = ("o", "lse2", "dq", "dk", "dv", "row_empty", "key_dead")
CHUNK_SCORES = 1 << 23


def _run(q, k, v, do, scale, causal, kpm, lut, p, seed, keep, model, fwd_only=False, **kw):
    """Batch rows in chunks of <= CHUNK_SCORES scores (bounded memory for the large short-query cases)."""
    B, Sq, H, _ = q.shape
    Sk = k.shape[1]
    nb = max(1, min(B, CHUNK_SCORES // max(1, H * Sq * Sk)))
    parts = []
    for b0 in range(0, B, nb):
        b1 = min(B, b0 + nb)
        kp = None
        if p > 0.0:
            kp = keep[b0:b1] if keep is not None else rowwise_keep_mask(
                seed, p, (b1 - b0) * H * Sq, Sk, q.device, row0=b0 * H * Sq).view(b1 - b0, H, Sq, Sk)
        parts.append(_attn64(q[b0:b1], k[b0:b1], v[b0:b1], do[b0:b1], scale, causal,
                             kpm[b0:b1] if kpm is not None else None, lut, p, kp, model, fwd_only, **kw))
    if len(parts) == 1:
        return parts[0]
    out = types.SimpleNamespace()
    for n in _CAT:
        if hasattr(parts[0], n):
            setattr(out, n, torch.cat([getattr(t, n) for t in parts], 0))
    for n in _SUM:
        if hasattr(parts[0], n):
            setattr(out, n, torch.stack([getattr(t, n) for t in parts], 0).sum(0))
    return out


def attn_ref(q, k, v, do, scale, causal, kpm, lut, p, keep=None, seed=0, fwd_only=False):
    """Attention forward and backward in float64 from the contract of csrc/attn_params.h.

    q, do [B, Sq, H, D], k, v [B, Sk, H, D]; kpm [B, Sk] (nonzero = visible) or None; lut [H, Sq + Sk - 1] or None;
    ``keep`` the bool [B, H, Sq, Sk] dropout mask of ``ops.rng.attention_keep_mask`` (None with p > 0: generated from
    ``seed`` by the same hash, chunk by chunk). With P the softmax over the visible keys (a row without one: P = 0) and
    P^ = P keep / (1 - p): o = P^ V; dV = P^T dO; dP = dO V^T; delta = rowsum(dO o); dS = P (keep dP / (1 - p) - delta);
    dQ = scale dS K; dK = scale dS^T Q; dlut[h, j - i + Sq - 1] = sum dS.

    Returns a namespace: o, dq, dk, dv [B, S, H, D]; lse2 [B, H, Sq] in log2 units (+inf on an empty row); dlut,
    dlut_mass [H, L]; cs_dq / cs_dk / cs_dv (+ _mass) [H * D] column sums over batch and sequence; row_empty [B, H, Sq],
    key_dead [B, Sk]. ``fwd_only``: o, lse2 and row_empty only."""
    return _run(q, k, v, do, scale, causal, kpm, lut, p, seed, keep, False, fwd_only)


def attn_bf16_model(q, k, v, do, scale, causal, kpm, lut, p, keep=None, seed=0, fwd_only=False, phase=1.0,
                    pre_scale=False):
    """``attn_ref`` with values rounded to bf16 where the bf16 kernels round them (read from csrc/attn.hip;
    csrc/attn_hd.hip packs at the same points but for ``pre_scale``), everything else exact:

    * forward, ``pack8(s0 / s1)`` before O^T += V^T P^T: the unnormalised probabilities exp2(s - m) (the row sum l is
      taken from the unrounded fp32 values; keep bits zero whole bf16 values, 1 / ((1 - p) l) scales the fp32
      accumulator). The online softmax rounds exp2(s - m_run) with m_run the RUNNING maximum (csrc/attn.hip lets it lag
      the tile maximum by up to 8), not the row's final one, so which values round up or down depends on the tile walk:
      ``phase`` rounds exp(s - max) * phase instead, and the figures the bounds come from (``ref_and_figures``) are the
      maximum over PHASES, four roundings the design permits equally. ``pre_scale``: csrc/attn_hd.hip multiplies by keep
      / (1 - p) BEFORE this rounding (``pr * dscale`` then ``pack8``), csrc/attn.hip after it;
    * the stored ``o`` (``store_rows_staged``), which the backward's delta = rowsum(dO o) reads;
    * dK/dV kernels, ``pack8(pd)``: P keep / (1 - p), recomputed in fp32 from the fp32 LSE, before dV^T += dO^T Pd;
    * dQ and dK/dV kernels, ``pack8(sv)`` / ``pack8(ds)``: dS before dQ^T += K^T dS^T and dK^T += Q^T dS (dP, delta and
      the diagonal sums for the bias gradient stay fp32, the scale is applied to the fp32 accumulator);
    * the stored dq, dk, dv; the column sums add those stored values.

    It is built from the reference alone and describes the precision the design permits: never tuned to a kernel's
    measured error. Not modelled (the factor 4 on top): accumulation order, the online softmax's deferred rescaling,
    exp2 against exp, fp32 partial sums."""
    return _run(q, k, v, do, scale, causal, kpm, lut, p, seed, keep, True, fwd_only, phase=phase, pre_scale=pre_scale)


# -------------------------------------------------------------------------------------------------------------- cases
# Seeds of the cases whose default draw (1234) misses the row condition of tests/test_attn_refs_cpu.py in the MODEL
# (the first higher seed that meets it at 1.1e-2; found with the reference and the model alone, no kernel involved).
# They are mostly the causal Sq >= Sk cases: the second live query row sees two keys, its dS has ONE degree of freedom
# (dP_1 - dP_0), and in ~10 % of the draws that scalar is so small that the row is rounding noise of delta against a
# vanishing reference.
SEEDS = {
    "B2H3D64-200x200---c-": 1237, "B2H3D64-200x200---cd": 1236, "B2H3D64-200x200--kc-": 1237,
    "B2H3D64-200x200--kcd": 1236, "B2H3D64-200x200-b-c-": 1235, "B2H3D64-200x200-b-cd": 1236,
    "B2H3D64-77x300-b-cd": 1235, "B2H3D64-200x200-bkc-": 1235, "B2H3D64-200x200-bkcd": 1236,
    "B2H2D64-200x200---cd": 1237, "B2H2D64-200x200--kcd": 1237, "B2H2D64-320x200--k-d": 1235,
    "B2H2D64-200x130---c-": 1235, "B2H2D64-200x130-bkcd": 1236, "B2H3D40-200x200---c-": 1236,
    "B2H3D40-200x200---cd": 1236, "B2H3D40-200x200--kc-": 1236, "B2H3D40-200x200--kcd": 1236,
    "B2H3D40-200x200-b-c-": 1243, "B2H3D40-200x200-b-cd": 1243, "B2H3D40-200x200-bkc-": 1243,
    "B2H3D40-200x200-bkcd": 1243, "B2H3D128-200x200---c-": 1244, "B2H3D128-200x200---cd": 1236,
    "B2H3D128-200x200--kc-": 1244, "B2H3D128-200x200--kcd": 1236, "B2H3D128-200x200-b-c-": 1236,
    "B2H3D128-200x200-b-cd": 1258, "B2H3D128-200x200-bkc-": 1236, "B2H3D128-200x200-bkcd": 1258,
}


def case(Sq, Sk, B=2, H=2, D=64, bias=False, kpm=None, causal=False, p=0.0, seed=None, dtype=BF16, cus=None):
    """One test case. ``kpm``: None, "suffix" (each batch row a padded suffix, ragged against the 64 / 128 tiles),
    "heavy" (batch row 0 keeps 40 keys: one live key block), "holes" (a whole 64-key tile, a whole 128-key block,
    scattered keys and key 0 padded), "empty" (batch row 1 has no valid key), "allpad" (no valid key at all)."""
    c = types.SimpleNamespace(Sq=Sq, Sk=Sk, B=B, H=H, D=D, bias=bias, kpm=kpm, causal=causal, p=p, seed=seed,
                              dtype=dtype, cus=cus)
    if seed is None:
        c.seed = SEEDS.get(case_id(c).replace("-f32", ""), 1234)  # the fp32 cases draw from the same seeds
    return c


def case_id(c):
    return (f"B{c.B}H{c.H}D{c.D}-{c.Sq}x{c.Sk}-" + ("b" if c.bias else "-") + ("k" if c.kpm else "-")
            + ("c" if c.causal else "-") + ("d" if c.p > 0 else "-")
            + (f"-{c.kpm}" if c.kpm not in (None, "suffix") else "")
            + ("-f32" if c.dtype == torch.float32 else ""))


def _kpm(kind, B, Sk, gen):
    m = torch.ones(B, Sk, dtype=torch.uint8)
    if kind == "suffix":
        for b in range(B):
            m[b, Sk - (37 + 45 * b) % Sk:] = 0
    elif kind == "heavy":
        m[0, 40:] = 0
        for b in range(1, B):
            if (11 * b) % 97:
                m[b, Sk - (11 * b) % 97:] = 0
    elif kind == "holes":
        m[:, 0] = 0
        if Sk >= 192:
            m[0, 64:128] = 0   # one whole 64-key tile
        if Sk >= 400:
            m[:, 256:384] = 0  # one whole 128-key block
        m[:, torch.randperm(Sk, generator=gen)[:max(3, Sk // 16)]] = 0
        m[:, Sk // 2 + 1] = 1
    elif kind == "empty":
        m[1 % B] = 0
        m[0, Sk - 21:] = 0
    elif kind == "allpad":
        m[:] = 0
    else:
        raise ValueError(kind)
    return m


QK_T5 = 0.7
QK_CAUSAL = 0.5


def make_case(c):
    """Every input of case ``c`` on the CPU from a seeded CPU generator (the CPU and GPU tests see identical values): q,
    k, v, do rounded to ``c.dtype`` (bf16), ``do`` without zeros, the T5 bucket table scaled by 0.5.

    Input choices made so that 4 x the model's row error fits ROW_CAP (tests/test_attn_refs_cpu.py), i.e. so that every
    row HAS a relative error to measure:
    * bias cases are T5's: scale 1.0 (no 1/sqrt(d)); q and k are drawn at std d^-1/4 * QK_T5, the others (scale d^-1/2)
      at std 1 or, causal, QK_CAUSAL. A peaked row's dS = P (dP - delta) cancels to ~0 while the rounding of the stored
      o (through delta) does not, so the gradient rows of a peaked softmax are rounding noise against a vanishing
      reference; causal rows that see a handful of keys are the most exposed;
    * a query row that sees exactly ONE key (causal) has dq = 0 identically, but with dropout its stored o = v / (1 - p)
      is rounded and dq becomes pure noise: the value row of such a key is zero, which makes o, delta and dP exact."""
    gen = torch.Generator().manual_seed(c.seed + 7919 * c.Sq + 104729 * c.Sk + (1 if c.bias else 0))
    std = c.D ** -0.25 * QK_T5 if c.bias else (QK_CAUSAL if c.causal else 1.0)
    r = types.SimpleNamespace(case=c, scale=1.0 if c.bias else c.D ** -0.5, causal=c.causal, p=c.p, seed=c.seed)
    r.q = (torch.randn(c.B, c.Sq, c.H, c.D, generator=gen) * std).to(c.dtype)
    r.k = (torch.randn(c.B, c.Sk, c.H, c.D, generator=gen) * std).to(c.dtype)
    r.v = torch.randn(c.B, c.Sk, c.H, c.D, generator=gen).to(c.dtype)
    do = torch.randn(c.B, c.Sq, c.H, c.D, generator=gen)
    r.do = (torch.where(do < 0, -1.0, 1.0) * do.abs().clamp(0.01, 4.0)).to(c.dtype)
    r.kpm = _kpm(c.kpm, c.B, c.Sk, gen) if c.kpm else None
    if c.causal:
        vis = visible(c.B, c.Sq, c.Sk, True, r.kpm, "cpu")[:, 0]
        single = vis & (vis.sum(-1, keepdim=True) == 1)  # [B, Sq, Sk]
        r.v[single.any(1)] = 0
    r.lut = r.idx = r.sat = None
    if c.bias:
        table = torch.randn(32, c.H, generator=gen) * 0.5
        off = c.Sk - c.Sq if c.causal else 0  # decoder with a key cache: query i sits at position i + Sk - Sq
        rel = torch.arange(-(c.Sq - 1), c.Sk, dtype=torch.long) - off
        r.idx = A.relative_position_bucket(rel, not c.causal, 32, 128)  # [L] bucket of each LUT entry
        r.lut = table.index_select(0, r.idx).t().contiguous()
        r.sat = A.saturated_ranges(r.idx)
    return r


def to_device(r, device):
    out = types.SimpleNamespace(**vars(r))
    for n in ("q", "k", "v", "do", "kpm", "lut", "idx"):
        t = getattr(r, n)
        if t is not None:
            setattr(out, n, t.to(device))
    return out


PHASES = (1.0, 2.0 ** 0.25, 2.0 ** 0.5, 2.0 ** 0.75)


def ref_and_figures(r, fwd_only=False):
    """(attn_ref, the model's figures) of built case ``r`` on its device: per output the largest error of
    ``attn_bf16_model`` against the reference over PHASES, in the metrics of the GPU tests."""
    args = (r.q, r.k, r.v, r.do, r.scale, r.causal, r.kpm, r.lut, r.p)
    ref = attn_ref(*args, seed=r.seed, fwd_only=fwd_only)
    fig = {}
    for ph in PHASES:
        mdl = attn_bf16_model(*args, seed=r.seed, fwd_only=fwd_only, phase=ph, pre_scale=r.case.D != 64)
        for n, v in model_figures(ref, mdl, r, fwd_only).items():
            fig[n] = max(fig.get(n, 0.0), v)
        del mdl
    return ref, fig


def per_bucket(dlut, idx, nb=32):
    """[H, L] LUT gradient (or mass) contracted to [H, buckets]: what reaches the T5 table."""
    return torch.zeros(dlut.shape[0], nb, dtype=dlut.dtype, device=dlut.device).index_add_(1, idx, dlut)


def model_figures(ref, mdl, r, fwd_only=False):
    """One model evaluation's error per output against the reference, in the metrics of the GPU tests."""
    if fwd_only:
        return {"o": row_err(mdl.o, ref.o)}
    f = {n: row_err(getattr(mdl, n), getattr(ref, n)) for n in ("o", "dq", "dk", "dv")}
    for n in ("cs_dq", "cs_dk", "cs_dv"):
        f[n] = mass_err(getattr(mdl, n), getattr(ref, n), getattr(ref, n + "_mass"))
    if r.lut is not None:
        f["dlut"] = mass_err(mdl.dlut, ref.dlut, ref.dlut_mass)
        f["dlut_bucket"] = mass_err(per_bucket(mdl.dlut, r.idx), per_bucket(ref.dlut, r.idx),
                                    per_bucket(ref.dlut_mass, r.idx))
    return f


# ------------------------------------------------------------------------------------- the cases of the GPU test file
def flag_matrix(D=64, dtype=BF16):
    """a: all 16 (bias, kpm, causal, p) combinations at self-attention 200 x 200 and cross 77 x 300, the causal ones
    also with a key cache (130 x 200). 200 / 300 / 77 / 130: no multiple of the 64 / 128 tiles, more than one block."""
    out = []
    for bias in (False, True):
        for kp in (None, "suffix"):
            for causal in (False, True):
                for p in (0.0, 0.1):
                    kw = dict(B=2, H=3, D=D, bias=bias, kpm=kp, causal=causal, p=p, dtype=dtype)
                    out.append(case(200, 200, **kw))
                    if D == 64 and dtype == BF16:
                        out.append(case(77, 300, **kw))
                        if causal:
                            out.append(case(130, 200, **kw))
    return out


def fwd_ring3_cases():
    """b: the forward's 3-deep K/V ring, with bias (Sk >= 2368) and without (Sk > 4864)."""
    return [case(130, sk, B=1, H=2, bias=b, kpm="suffix", causal=ca, p=0.1)
            for sk, b in ((2500, True), (5000, False)) for ca in (False, True)]


def dkdv2_cases():
    """c: dkdv2 ring depth 3 without bias, depth 2, and the > 64 KB dynamic-LDS opt-in with bias."""
    return [case(320, 200, p=0.1), case(320, 200, p=0.0), case(1100, 130, B=1, H=2, bias=True, p=0.1)]


def sq_forced_cases():
    """d: the short-query kernel forced to MB = 4: 5 and 8 key blocks (a ragged last group of 1, two full groups)."""
    return [case(sq, sk, kpm=kp, p=p) for sq in (40, 100, 128) for sk in (520, 1000) for kp in (None, "suffix")
            for p in (0.0, 0.1)]


def sq_mb2_cases(cus=256):
    """d: the short-query kernel unforced at MB = 2: B * H = 2 x CUs at 5 key blocks, 3 x CUs at 4 (H = 16)."""
    return [case(100, 600, B=-(-2 * cus // 16), H=16, kpm="heavy", p=0.1, cus=cus),
            case(100, 500, B=-(-3 * cus // 16), H=16, kpm="heavy", p=0.1, cus=cus)]


def colsum_cases():
    """e: column-sum arms: dQ + dkdv2 at ring depth 2 (200 x 200) and 3 (320 x 200, p = 0.1), dkdv_sq (forced MB 4)."""
    out = [case(200, 200, kpm=kp, causal=ca, p=p) for kp in (None, "suffix") for ca in (False, True)
           for p in (0.0, 0.1)]
    out += [case(320, 200, kpm=kp, p=0.1) for kp in (None, "suffix")]
    out += [case(100, 520, kpm=kp, p=p) for kp in (None, "suffix") for p in (0.0, 0.1)]
    return out


def mask_cases():
    """f: a batch row with no valid key (forward, dQ, dkdv2; dkdv_sq at 100 x 520), masks with holes, causal Sq > Sk."""
    return [case(200, 200, kpm="empty", p=0.1), case(200, 200, bias=True, kpm="empty", causal=True, p=0.1),
            case(100, 520, kpm="empty", p=0.1), case(200, 520, kpm="holes", p=0.1),
            case(100, 520, kpm="holes", p=0.1), case(200, 520, bias=True, kpm="holes", causal=True),
            case(200, 130, causal=True), case(200, 130, bias=True, kpm="suffix", causal=True, p=0.1)]


def all_gpu_cases(cus=256):
    seen, out = set(), []
    for c in (flag_matrix() + fwd_ring3_cases() + dkdv2_cases() + sq_forced_cases() + sq_mb2_cases(cus) + colsum_cases()
              + mask_cases() + flag_matrix(D=40) + flag_matrix(D=128)):
        if case_id(c) not in seen:
            seen.add(case_id(c))
            out.append(c)
    return out
