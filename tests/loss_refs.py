"""fp64 references, input generators and error metrics for the loss-path kernels: cross-entropy (csrc/ce.hip), the
LM-head CE epilogues of csrc/gemm_w4.hip (W4_EPI_CEF / W4_EPI_CEB) and the embedding backward (csrc/embed.hip).

Plain torch in float64, written from the operations' definitions (not from the kernels): the oracle of
tests/test_loss_kernels_gpu.py and tests/test_embed_kernels_gpu.py, itself validated on the CPU by
tests/test_loss_refs_cpu.py against ``F.cross_entropy`` and autograd in float64.  Not a conftest: imported by name, like
tests/rowwise_refs.py and tests/gemm_refs.py.

The contract all four CE routes state: a row whose label is ``ignore``, negative or ``>= V`` has loss 0 and gradient 0;
``lse`` is defined for every row.  loss = lse - (1 - eps) x_y - eps mean_v(x_v);  dx_v = g (exp(x_v - lse) - eps / V -
(1 - eps) [v == y]).  Without smoothing (eps == 0) the mean term is absent, so a ``-inf`` logit (a banned token) on a
column other than the label leaves the loss finite, as in ``F.cross_entropy``.
"""
import torch

import gemm_refs as G
import rowwise_refs as R

BF16, F32 = torch.bfloat16, torch.float32
U32 = 2.0 ** -24  # unit roundoff of fp32 (round to nearest)
EXP_ULPS = 8.0    # allowance for the exp intrinsic itself, in units of U32 (see ce_abs_term)
COMP_MARGIN = 4.0  # a bound is 4x what a faithful fp32 evaluation may lose (the comp rule; see ce_abs_term)
LOSS_BOUND = R.ROW_BOUND[F32]  # per-row bound of loss and lse: |got - ref| / max(1, |ref|)


class Figures:
    """Collects a test's figures: each is printed ([fig] lines; run with -s or -rP to collect them) before the test
    asserts, and ``done`` fails with every figure over its bound (the style of tests/test_distill_gpu.py)."""

    def __init__(self, tag):
        self.tag, self.bad, self.worst = tag, [], {}

    def add(self, name, val, bound, quiet=False):
        line = f"[fig] {self.tag} {name}: err {val:.3e} bound {bound:.1e}"
        if not quiet:
            print(line)
        if not val <= bound:
            self.bad.append(line)
        return val

    def fold(self, name, val, bound, case):
        """One figure for a family of cases: keeps the worst val / bound (printed by ``done``), fails like ``add``."""
        if not val <= bound:
            self.bad.append(f"[fig] {self.tag} {name} [{case}]: err {val:.3e} bound {bound:.1e}")
        r = val / bound if val == val else float("inf")
        if name not in self.worst or not r <= self.worst[name][0]:
            self.worst[name] = (r, val, bound, case)

    def check(self, name, ok, quiet=True):
        if not (ok and quiet):
            print(f"[fig] {self.tag} {name}: {'ok' if ok else 'FAILED'}")
        if not ok:
            self.bad.append(f"{self.tag} {name}")

    def done(self):
        for name, (r, val, bound, case) in self.worst.items():
            print(f"[fig] {self.tag} {name}: worst err {val:.3e} bound {bound:.1e} (x{r:.3g} of the bound) at [{case}]")
        assert not self.bad, "\n".join(self.bad)


# ---------------------------------------------------------------------------------------------------------- references
def valid_rows(labels, ignore, V):
    return (labels != ignore) & (labels >= 0) & (labels < V)


def ce_ref(logits, labels, bias, eps, ignore, V, g=1.0):
    """(loss_rows [N], lse [N], dlogits [N, V]) in fp64 of the logits as given (+ bias [V]); ``g``: the scalar every
    valid row's gradient is multiplied by."""
    x = logits.double()
    assert x.dim() == 2 and x.shape[1] == V, (x.shape, V)
    if bias is not None:
        x = x + bias.double().view(1, V)
    lse = torch.logsumexp(x, dim=1)
    valid = valid_rows(labels, ignore, V)
    y = labels.clamp(0, V - 1)
    xy = x.gather(1, y.view(-1, 1)).view(-1)
    loss = lse - (1.0 - eps) * xy
    if eps != 0.0:
        loss = loss - eps * x.mean(dim=1)
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    d = torch.exp(x - lse.view(-1, 1)) - eps / V
    d.scatter_add_(1, y.view(-1, 1), torch.full_like(xy, -(1.0 - eps)).view(-1, 1))
    d = float(g) * d * valid.view(-1, 1).double()
    return loss, lse, d


def lm_head_ref(h, w, labels, bias, eps, ignore, g=1.0):
    """(loss_rows, lse, dlogits, dh [N, d], dW [V, d]) in fp64 on the logits h @ w^T (+ bias)."""
    h64, w64 = h.double(), w.double()
    loss, lse, d = ce_ref(h64 @ w64.t(), labels, bias, eps, ignore, w.shape[0], g)
    return loss, lse, d, d @ w64, d.t() @ h64


def embed_bwd_ref(ids, dy, V, pad, out0):
    """out0 + index_add of dy's rows at ``ids`` in fp64; pad (``pad`` = -1: none) and out-of-range ids are dropped."""
    keep = (ids >= 0) & (ids < V) & (ids != pad)
    out = out0.double().clone()
    out.index_add_(0, ids[keep], dy.double()[keep])
    return out


# ------------------------------------------------------------------------------------------------------------- metrics
def row_metric(got, ref):
    """max over rows of |got - ref| / max(1, |ref|) (loss and lse); a non-finite ``got`` counts as infinite."""
    g, r = got.detach().double().view(-1), ref.double().view(-1)
    assert g.shape == r.shape, (g.shape, r.shape)
    err = (g - r).abs() / r.abs().clamp_min(1.0)
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    return err.max().item()


def ce_abs_term(logits, labels, bias, eps, ignore, V, g=1.0):
    """Per-element fp32 evaluation error of  g (exp(x - lse) - eps / V - (1 - eps) [v == y])  given exact x (the stored
    logit or the exact fp32 accumulator), an fp32 bias and lse rounded to fp32.  With u = 2^-24, t = x + b - lse and
    p = exp(t) <= 1:

      argument of exp:  fl(x + b) adds (|x| + |b|) u;  lse, held in fp32, adds |lse| u;  the subtraction adds |t| u;
                        the fast exp is exp2(t log2 e), whose product rounds once more: another |t| u in t
      -> exp turns an argument error dt into p dt:  p (|x| + |b| + |lse| + 2 |t|) u
      the intrinsic:    v_exp_f32 is good to 1 ulp (2 u relative); EXP_ULPS = 8 u leaves a factor 4 for the range
                        reduction around it:  p EXP_ULPS u
      final roundings:  fl(p - eps / V), fl(. - (1 - eps)), fl(g .) and an fp32 store, each <= u on a magnitude <= 1
                        (eps / V and 1 - eps themselves carry u relative, on magnitudes <= 1):  4 u

      model    = |g| u (p (|x| + |b| + |lse| + 2 |t| + EXP_ULPS) + 4)
      abs_term = COMP_MARGIN model,  COMP_MARGIN = 4

    The model is what ANY fp32 evaluation of the expression may lose, the torch composite included (its worst element
    measures 0.25 .. 0.5 of the model on the tests' inputs); the project's comp rule wants the composite at or under a
    quarter of a bound, hence the factor 4 on the model.  What the bound must catch is far above it: one dropped
    eps / V is 1e-4 |g| at V = 1003 against abs_term ~ 1e-6 |g|, a misplaced label (1 - eps) |g|.

    p, t and lse are the fp64 reference's.  A row that is not valid has gradient exactly 0 in every kernel: its term is
    the smallest positive double, so that the bound stays > 0 and nothing but 0 passes."""
    x = logits.double()
    b = bias.double().view(1, V) if bias is not None else torch.zeros(1, V, dtype=torch.float64, device=x.device)
    lse = torch.logsumexp(x + b, dim=1).view(-1, 1)
    t = x + b - lse
    p = torch.exp(t)
    t = torch.where(torch.isfinite(t), t, torch.zeros_like(t))  # a -inf logit: p = 0, no exp error at all
    xa = torch.where(torch.isfinite(x + b), x.abs() + b.abs(), torch.zeros_like(x))
    term = COMP_MARGIN * abs(float(g)) * U32 * (p * (xa + lse.abs() + 2.0 * t.abs() + EXP_ULPS) + 4.0)
    valid = valid_rows(labels, ignore, V).view(-1, 1)
    return torch.where(valid, term, torch.full_like(term, 5e-324))


def grad_bound(ref, abs_term, dtype):
    """Per-element bound (the form of gemm_refs.assert_elem_bound): BF16_REL |ref| + abs_term for a bf16 store,
    abs_term alone (it holds the fp32 store's rounding) for an fp32 store."""
    if dtype == BF16:
        return G.BF16_REL * ref.double().abs() + abs_term
    assert dtype == F32
    return abs_term


def grad_worst(got, ref, bound):
    """Worst |got - ref| / bound over the elements (<= 1 passes) and where it is."""
    worst, where, _, _ = G.elem_bound(got, ref, bound)
    return worst, where


# ---------------------------------------------------------------------------------------------------------- generators
IGNORE = -100


def peak_columns(V):
    """A few columns that get the boost: one near each end and one in the middle."""
    return sorted({min(1, V - 1), V // 2, max(V - 2, 0)})


def peaked_logits(N, V, device, generator, scale=1.5, boost=4.0):
    """fp32 [N, V]: scale * randn with +boost on ``peak_columns(V)`` (near-uniform softmax would hide a dropped column:
    a peak carries O(1) of the row's mass)."""
    x = scale * torch.randn(N, V, device=device, generator=generator)
    x[:, peak_columns(V)] += boost
    return x


def edge_labels(N, V, device, generator):
    """int64 [N]: the first rows walk the edge cases (last column, ignored, column 0, y = V, the peak inside a scalar
    head, y = -1, a scalar-tail column, the middle peak, an off-peak column), the rest are random with every third on
    a peak."""
    pat = [V - 1, IGNORE, 0, V, min(1, V - 1), -1, max(V - 2, 0), V // 2, V // 3]
    lab = torch.randint(0, V, (N,), device=device, generator=generator)
    pk = torch.tensor(peak_columns(V), device=device)
    third = torch.arange(N, device=device) % 3 == 0
    lab = torch.where(third, pk[torch.arange(N, device=device) % len(pk)], lab)
    n = min(N, len(pat))
    lab[:n] = torch.tensor(pat[:n], device=device)
    return lab


def dyadic_bias(V, device, generator, boost=4.0):
    """fp32 [V] of k/8 values (exact to add to an exact accumulator) with +boost on the peak columns."""
    b = G.dyadic(V, device, generator=generator).float()
    b[peak_columns(V)] += boost
    return b


def lm_operands(N, d, V, device, generator, peaks=None):
    """Dyadic h [N, d] and w [V, d] (gemm_refs.dyadic): every logit is exact in an fp32 accumulator (64 (d + bias) <
    2^24), so only exp / log error remains.  w keeps ~16 entries per row (logits of std ~1.5); the first eight columns
    of h are 1 and the peak rows of w carry 1 there: a +8 boost without a bias."""
    h = G.dyadic((N, d), device, generator=generator)
    w = G.dyadic((V, d), device, min(1.0, 16.0 / d), generator=generator)
    h[:, :8] = 1.0
    w[peak_columns(V) if peaks is None else peaks, :8] = 1.0
    return h, w


def embed_operands(T, d, V, device, generator):
    """dy [T, d] bf16 and out0 [V, d] fp32 of multiples of 2^-3 with |x| <= 4: every per-id sum of <= 4099 terms plus
    its prior is a multiple of 2^-3 below 2^24 * 2^-3, exact in fp32 in any order."""
    dy = (torch.randint(-32, 33, (T, d), device=device, generator=generator).float() / 8.0).to(BF16)
    out0 = torch.randint(-32, 33, (V, d), device=device, generator=generator).float() / 8.0
    return dy, out0


def embed_headroom(ids, dy, out0, V):
    """8 * max |out0| + sum over an id's rows of |dy|: callers assert it is < 2^24 (gemm_refs.EXACT_LIMIT)."""
    mass = embed_bwd_ref(ids, dy.abs(), V, -1, out0.abs())
    return 8.0 * mass.max().item()


# Hand-made chunk tables (first column, width, leading columns to skip) for the chunk kernels, whose own grid is 4
# columns.  HAND_TABLE (V = 1032): skip 1 and 3 leave a partially skipped 4-group, 4 a wholly skipped one, 7 one of
# each.  WIDE_TABLE (V = 2056): width 1028 is one full trip of 256 lanes x 4 plus one group in the second trip.
HAND_TABLE = [(0, 256, 0), (255, 264, 1), (516, 256, 3), (768, 260, 4), (1021, 8, 7), (1028, 4, 1)]
WIDE_TABLE = [(0, 1028, 0), (1028, 1028, 0)]


# ------------------------------------------------------------------------------- the chunk-state merge, emulated in fp64
def chunk_merge_ref(logits, labels, bias, eps, ignore, V, chunks):
    """(loss_rows, lse) by the algorithm of the vocabulary-chunked forward, in fp64: per chunk (c0, n, skip) the
    columns c0 + skip .. c0 + n - 1 give {max, sum exp(x - max), sum x, x_label if the label is among them}, merged
    into a running state; the last chunk turns it into lse and loss.  Validates the algorithm and a chunk table apart
    from the kernel."""
    x = logits.double()
    if bias is not None:
        x = x + bias.double().view(1, V)
    N = x.shape[0]
    m = torch.full((N,), float("-inf"), dtype=torch.float64, device=x.device)
    s, sx, xl = (torch.zeros(N, dtype=torch.float64, device=x.device) for _ in range(3))
    for c0, n, skip in chunks:
        xc = x[:, c0 + skip:c0 + n]
        cm = xc.max(dim=1).values
        nm = torch.maximum(m, cm)
        s = s * torch.exp(m - nm) + torch.exp(xc - nm.view(-1, 1)).sum(1)
        m = nm
        sx = sx + xc.sum(1)
        own = (labels >= c0 + skip) & (labels < c0 + n)
        xl = torch.where(own, x.gather(1, labels.clamp(0, V - 1).view(-1, 1)).view(-1), xl)
    lse = m + torch.log(s)
    loss = lse - (1.0 - eps) * xl - (eps * sx / V if eps != 0.0 else 0.0)
    return torch.where(valid_rows(labels, ignore, V), loss, torch.zeros_like(loss)), lse
