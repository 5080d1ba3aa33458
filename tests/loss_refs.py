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

The distillation loss (csrc/kd.hip; ``kd_ref``, ``kd_chunk_merge_ref``, ``kd_loss_abs_term``, ``kd_abs_term``; oracle of
tests/test_kd_kernels_gpu.py) adds  kl = sum_v p_v (log p_v - log q_v),  p = softmax(t/T), q = softmax(s/T), with the
same row validity, and this contract for ``-inf`` logits (banned tokens, through a bias or in the logits themselves):

* a column with p_v = 0 contributes 0 to kl, whatever s_v is, -inf included (0 * -inf is never formed);
* a column with p_v > 0 and s_v = -inf makes kl = +inf, not NaN;
* with eps == 0 the smoothing term is absent, so ce stays finite with -inf on columns other than the label;
* the gradient  w_ce (softmax(s) - eps/V - (1-eps)[v==y]) + w_kl T (q - p)  is finite wherever stats is.
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


def _kd_logits(student, teacher, bias_s, bias_t, V):
    s, t = student.double(), teacher.double()
    assert s.dim() == 2 and s.shape[1] == V and t.shape == s.shape, (s.shape, t.shape, V)
    if bias_s is not None:
        s = s + bias_s.double().view(1, V)
    if bias_t is not None:
        t = t + bias_t.double().view(1, V)
    return s, t


def kd_ref(student, teacher, labels, bias_s, bias_t, eps, ignore, V, T, w_ce=1.0, w_kl=1.0):
    """(ce_rows [N], kl_rows [N], stats [N, 3] = {lse(s), lse(s/T), lse(t/T)}, ds [N, V]) in fp64 of the logits as
    given (+ biases [V]), from the definition:  ce is ``ce_ref``'s;  kl = sum_v p_v (log p_v - log q_v) with
    p = softmax(t/T), q = softmax(s/T);  ds = w_ce (softmax(s) - eps/V - (1-eps)[v==y]) + w_kl T (q - p).  Rows that
    are not ``valid_rows`` have ce 0, kl 0 and gradient 0; ``stats`` is defined for every row.  -inf (module docstring):
    a column with p_v = 0 adds 0 whatever s_v is; p_v > 0 with s_v = -inf adds +inf."""
    s, t = _kd_logits(student, teacher, bias_s, bias_t, V)
    ce, lse_s, ds = ce_ref(s, labels, None, eps, ignore, V, w_ce)
    lse_sT = torch.logsumexp(s / T, dim=1)
    lse_tT = torch.logsumexp(t / T, dim=1)
    logq = s / T - lse_sT.view(-1, 1)
    logp = t / T - lse_tT.view(-1, 1)
    p, q = torch.exp(logp), torch.exp(logq)
    kl = torch.where(p > 0, p * (logp - logq), torch.zeros_like(p)).sum(1)
    valid = valid_rows(labels, ignore, V)
    kl = torch.where(valid, kl, torch.zeros_like(kl))
    ds = ds + float(w_kl) * float(T) * (q - p) * valid.view(-1, 1).double()
    return ce, kl, torch.stack([lse_s, lse_sT, lse_tT], 1), ds


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


LOG_ULPS = 8.0  # allowance for the log intrinsic (log2 to 1 ulp, times ln 2), in units of U32 of |log Z|, like EXP_ULPS


def kd_steps(V, dtype, chunks=None):
    """Worst-case number of sequential accumulation steps a column's weight goes through in the distillation forward:
    the 16-B groups one of 256 lanes walks (8 bf16 or 4 fp32 columns each; the chunk kernels walk 4), plus one merge
    per chunk for the chunked form."""
    if chunks is None:
        per = 256 * (8 if dtype == BF16 else 4)
        return -(-V // per) + 2  # + the scalar head and tail
    return max(-(-n // 1024) for _, n, _ in chunks) + len(chunks)


def _online_softmax_model(x, b, T, steps):
    """Error model, in units of U32, of one online softmax  Z = sum_v exp((x_v + b_v - m) / T)  as csrc/kd.hip forms it
    (running maxima per lane, then per block, then per chunk).  Returns (p [N, V] exact weights, delta [N, V], Lerr
    [N]) with delta_v the relative error of column v's weight as it arrives in Z and Lerr the absolute error of
    lse = m / T + log Z.

      the weight's exponent: a column is first taken relative to its lane's running maximum m0 >= x_v and then rescaled
        by exp((m0 - m1) / T), exp((m1 - m2) / T), ... up to the row's maximum m.  The maxima only grow, so every
        argument is <= 0 and their magnitudes add up to exactly |a_v|, a_v = (x_v + b_v - m) / T.  Each argument
        carries four roundings of its own magnitude (the subtraction; 1 / T, itself rounded, and the product with it;
        the product with log2 e inside the fast exp):  4 |a_v|.  fl(x_v + b_v) adds (|x_v| + |b_v|) / T when there
        is a bias (a stored logit is exact in fp32).
      the intrinsics: EXP_ULPS for the column's own exponential, and EXP_ULPS + 1 (the product) for every rescale;
        a lane's maximum can change at every step, the block and chunk merges are counted in ``steps``.
      the sum: every addition rounds the partial sum once: steps + 3 (inside a 16-B group) + 8 (the block tree).
      delta_v = [(|x_v| + |b_v|) / T] + 4 |a_v| + EXP_ULPS + (EXP_ULPS + 1) steps + steps + 11

      log Z inherits the p-weighted mean of delta; m / T is a product with a rounded 1 / T (2 |m| / T); the log
      intrinsic LOG_ULPS |log Z|; the final addition |lse|:
      Lerr = E_p[delta] + 2 |m| / T + LOG_ULPS |log Z| + |lse|

    A -inf column has weight 0 and no error."""
    xb = x if b is None else x + b
    m = xb.max(dim=1, keepdim=True).values
    a = (xb - m) / T
    lse = torch.logsumexp(xb / T, dim=1, keepdim=True)
    p = torch.exp(xb / T - lse)
    fin = torch.isfinite(xb)
    aa = torch.where(fin, a.abs(), torch.zeros_like(a))
    delta = 4.0 * aa + EXP_ULPS + (EXP_ULPS + 1.0) * steps + steps + 11.0
    if b is not None:
        delta = delta + torch.where(fin, (x.abs() + b.abs()) / T, torch.zeros_like(a))
    logz = lse - m / T
    lerr = (p * delta).sum(1) + (2.0 * m.abs() / T + LOG_ULPS * logz.abs() + lse.abs()).view(-1)
    return p, delta, lerr


def kd_loss_abs_term(student, teacher, labels, bias_s, bias_t, eps, ignore, V, T, steps):
    """(ce_term [N], kl_term [N]): per-row ABSOLUTE bounds of the distillation forward's two losses in fp32.

    The row losses are not relative-error quantities.  A one-pass kernel cannot form sum_v p_v (log p_v - log q_v)
    (it has no lse until the row ends); it evaluates  kl = E_p[t - s] / T - lse(t/T) + lse(s/T),  a difference of
    terms of magnitude  mag = E_p|t - s| / T + |lse(t/T)| + |lse(s/T)|  that can sit orders above kl itself, and so
    does the composite's sum of p_v (log p_v - log q_v), each log p_v = t_v / T - lse(t/T) rounded at that magnitude.
    With u = 2^-24 and ``_online_softmax_model``'s delta (relative error of a column's teacher weight) and Lerr:

      E = A / Zt, A = sum_v w_v d_v, d_v = t_v - s_v:  the weights' errors move the mean by at most
          E_p[(|d_v| + |E|) delta_v]  (A and Zt are separate sums: no cancellation between them is assumed);
          fl(t_v - s_v), the product w_v d_v and its accumulation: 3 E_p|d_v|, plus fl(x + b) of both logits where
          there is a bias: E_p[|t_v| + |bt_v| + |s_v| + |bs_v|];  the division and the product with the rounded 1 / T:
          3 |E|                                                                          -> all of it over T
      the two lse:  Lerr(t/T) + Lerr(s/T)
      the combination  E / T - lse(t/T) + lse(s/T)  and the store: two roundings of partial results <= mag:  2 mag

      kl model = u (E_p[(|d| + |E|) delta + 3 |d| + bias magnitudes] / T + 3 |E| / T + Lerr_t + Lerr_s + 2 mag)

    ce = lse(s) - (1 - eps) s_y - eps sum(s) / V  with  mag_ce = |lse(s)| + (1 - eps) |s_y| + eps |sum(s)| / V:
      Lerr(s) at T = 1;  (1 - eps) s_y: the rounded factor and the product, 2 (1 - eps) |s_y|, plus fl(x_y + b_y);
      sum(s): every addition rounds a partial sum of magnitude <= sum|s_v|, steps + 11 of them on a column's way (plus
      fl(x + b)), then eps / V: two more on |sum(s)|;  the two subtractions: 2 mag_ce

      ce model = u (Lerr_s1 + 2 (1 - eps) |s_y| + |x_y| + |b_y| + eps / V ((steps + 12) sum|s_v| + 2 |sum(s)|)
                    + 2 mag_ce)

    Both terms are COMP_MARGIN times their model: the model is what a faithful fp32 evaluation may lose, the comp rule
    wants the fp32 composite at or under a quarter of a bound (tests/test_loss_refs_cpu.py measures the composite and
    a plain fp32 evaluation of the cancelling form against it on the GPU tests' inputs).  What the bounds must catch
    is far above them: one dropped 16-B group of a V = 1003 row moves lse by ~1e-2 of its mass, a missing 1 / T in a
    rescale by O(1).  Rows that are not valid have both losses exactly 0: their term is the smallest positive double.
    -inf columns: weight 0, no error; a row whose reference kl is +inf has an infinite term (the test compares such
    rows for equality instead)."""
    s, t = _kd_logits(student, teacher, None, None, V)
    bs = None if bias_s is None else bias_s.double().view(1, V)
    bt = None if bias_t is None else bias_t.double().view(1, V)
    sb = s if bs is None else s + bs
    tb = t if bt is None else t + bt
    zero = torch.zeros_like(s)
    # kl
    p, delta, lerr_t = _online_softmax_model(t, bt, T, steps)
    _, _, lerr_s = _online_softmax_model(s, bs, T, steps)
    live = p > 0
    d = torch.where(live, (tb - sb).abs(), zero)
    E = torch.where(live, p * (tb - sb), zero).sum(1)
    mags = zero
    if bs is not None:
        mags = mags + torch.where(torch.isfinite(sb), s.abs() + bs.abs(), zero)
    if bt is not None:
        mags = mags + torch.where(torch.isfinite(tb), t.abs() + bt.abs(), zero)
    mean = (p * ((d + E.abs().view(-1, 1)) * delta + 3.0 * d + mags)).sum(1)
    lse_sT, lse_tT = torch.logsumexp(sb / T, 1), torch.logsumexp(tb / T, 1)
    mag = (p * d).sum(1) / T + lse_tT.abs() + lse_sT.abs()
    kl_model = U32 * ((mean + 3.0 * E.abs()) / T + lerr_t + lerr_s + 2.0 * mag)
    # ce
    _, _, lerr_1 = _online_softmax_model(s, bs, 1.0, steps)
    y = labels.clamp(0, V - 1).view(-1, 1)
    sy = sb.gather(1, y).view(-1).abs()
    xy = torch.zeros_like(sy) if bs is None else (s.abs() + bs.abs()).gather(1, y).view(-1)  # fl(x_y + b_y)
    ce_model = lerr_1 + 2.0 * (1.0 - eps) * sy + xy + 2.0 * (torch.logsumexp(sb, 1).abs() + (1.0 - eps) * sy)
    if eps != 0.0:
        sabs, ssum = sb.abs().sum(1), sb.sum(1).abs()
        ce_model = ce_model + eps / V * ((steps + 12.0) * sabs + 2.0 * ssum) + 2.0 * eps * ssum / V
    ce_model = U32 * ce_model
    valid = valid_rows(labels, ignore, V)
    tiny = torch.full_like(kl_model, 5e-324)
    return torch.where(valid, COMP_MARGIN * ce_model, tiny), torch.where(valid, COMP_MARGIN * kl_model, tiny)


def kd_abs_term(student, teacher, labels, bias_s, bias_t, eps, ignore, V, T, w_ce=1.0, w_kl=1.0):
    """Per-element fp32 evaluation error of  ds = w_ce (exp(s - lse(s)) - eps / V - (1 - eps) [v == y]) +
    w_kl T (exp(s / T - lse(s/T)) - exp(t / T - lse(t/T)))  given the stored logits, fp32 biases and the three lse
    rounded to fp32: ``ce_abs_term`` (with g = w_ce) extended by the two extra exponentials.  For e = exp(x / T - L),
    x = the logit + bias, L = its lse, r = x / T - L:

      argument:  fl(logit + b) adds (|logit| + |b|) u / T;  1 / T is rounded and the product rounds: 2 (|logit| + |b|)
                 u / T;  L, held in fp32, |L| u;  the subtraction |r| u;  the product with log2 e in the fast exp |r| u
      -> e (3 (|logit| + |b|) / T + |L| + 2 |r|) u,  the intrinsic e EXP_ULPS u
      final roundings:  fl(q - p), w_kl T (a rounded product), its product with the difference, and the sum with the
                 ce part, on magnitudes <= |w_kl| T:  4 u

      model    = ce model(w_ce) + |w_kl| T u (sum over {q, p} of e (3 (|logit| + |b|) / T + |L| + 2 |r| + EXP_ULPS) + 4)
      abs_term = COMP_MARGIN model

    A -inf column has e = 0 and no error; rows that are not valid get the smallest positive double (``ce_abs_term``)."""
    s, t = _kd_logits(student, teacher, None, None, V)
    term = ce_abs_term(s, labels, bias_s, eps, ignore, V, w_ce)
    extra = torch.zeros_like(s)
    for x, bias in ((s, bias_s), (t, bias_t)):
        b = bias.double().view(1, V) if bias is not None else torch.zeros(1, V, dtype=torch.float64, device=x.device)
        L = torch.logsumexp((x + b) / T, dim=1).view(-1, 1)
        r = (x + b) / T - L
        e = torch.exp(r)
        fin = torch.isfinite(x + b)
        r = torch.where(fin, r, torch.zeros_like(r))
        xa = torch.where(fin, x.abs() + b.abs(), torch.zeros_like(x))
        extra = extra + e * (3.0 * xa / T + L.abs() + 2.0 * r.abs() + EXP_ULPS)
    extra = COMP_MARGIN * abs(float(w_kl)) * float(T) * U32 * (extra + 4.0)
    valid = valid_rows(labels, ignore, V).view(-1, 1)
    return torch.where(valid, term + extra, torch.full_like(term, 5e-324))


def abs_worst(got, ref, term):
    """Worst |got - ref| / term over the rows (<= 1 passes); a non-finite ``got`` counts as infinite."""
    g, r = got.detach().double().view(-1), ref.double().view(-1)
    err = (g - r).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    return (err / term).max().item()


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


def kd_chunk_merge_ref(student, teacher, labels, bias_s, bias_t, eps, ignore, V, T, chunks):
    """(ce_rows, kl_rows, stats [N, 3], state [N, 8]) by the algorithm of the vocabulary-chunked distillation forward,
    in fp64: per chunk (c0, n, skip) the columns c0 + skip .. c0 + n - 1 give the student's {max, sum exp(s - max),
    sum exp((s - max) / T), sum s, s_label if the label is among them} and the teacher's {max, sum w, A = sum w (t - s)}
    with w = exp((t - max) / T), a column with w = 0 adding nothing to A; all merged into the running state
    {m_s, Z_s, sum s, s_label, Z_sT, m_t, Z_t, A}, which the last chunk turns into ce, kl and stats.  Validates the
    algorithm and a chunk table apart from the kernel."""
    s, t = _kd_logits(student, teacher, bias_s, bias_t, V)
    N = s.shape[0]
    ninf = torch.full((N,), float("-inf"), dtype=torch.float64, device=s.device)
    ms, mt = ninf.clone(), ninf.clone()
    zs, zsT, sx, sy, zt, A = (torch.zeros(N, dtype=torch.float64, device=s.device) for _ in range(6))

    def scale(old, new, invT=1.0):  # exp((old - new) / T), 0 where old is -inf (new may be -inf too)
        return torch.where(old == float("-inf"), torch.zeros_like(old), torch.exp((old - new) * invT))

    def carry(a, f):  # a * f with an underflowed (or -inf-born) factor taking an infinite a to 0
        return torch.where(f != 0, a * f, torch.zeros_like(a))

    for c0, n, skip in chunks:
        sc, tc = s[:, c0 + skip:c0 + n], t[:, c0 + skip:c0 + n]
        ns, nt = torch.maximum(ms, sc.max(1).values), torch.maximum(mt, tc.max(1).values)
        es = torch.where(sc == float("-inf"), torch.zeros_like(sc), sc - ns.view(-1, 1))  # -inf: weight 0 below
        ws = torch.where(sc == float("-inf"), torch.zeros_like(sc), torch.exp(es))
        wsT = torch.where(sc == float("-inf"), torch.zeros_like(sc), torch.exp(es / T))
        wt = torch.where(tc == float("-inf"), torch.zeros_like(tc), torch.exp((tc - nt.view(-1, 1)) / T))
        zs = zs * scale(ms, ns) + ws.sum(1)
        zsT = zsT * scale(ms, ns, 1.0 / T) + wsT.sum(1)
        f = scale(mt, nt, 1.0 / T)
        zt = zt * f + wt.sum(1)
        A = carry(A, f) + torch.where(wt != 0, wt * (tc - sc), torch.zeros_like(tc)).sum(1)
        ms, mt = ns, nt
        sx = sx + sc.sum(1)
        own = (labels >= c0 + skip) & (labels < c0 + n)
        sy = torch.where(own, s.gather(1, labels.clamp(0, V - 1).view(-1, 1)).view(-1), sy)
    lse_s, lse_sT, lse_tT = ms + torch.log(zs), ms / T + torch.log(zsT), mt / T + torch.log(zt)
    ce = lse_s - (1.0 - eps) * sy - (eps * sx / V if eps != 0.0 else 0.0)
    kl = A / zt / T - lse_tT + lse_sT
    valid = valid_rows(labels, ignore, V)
    zero = torch.zeros_like(ce)
    return (torch.where(valid, ce, zero), torch.where(valid, kl, zero), torch.stack([lse_s, lse_sT, lse_tT], 1),
            torch.stack([ms, zs, sx, sy, zsT, mt, zt, A], 1))


# ------------------------------------------------------------------------------------------ distillation test inputs
HOT_SCALE = 20.0  # one row of both models scaled by this: the running maxima and the rescales matter


def kd_logits(N, V, device, generator, dtype, hot=None, hot_scale=HOT_SCALE):
    """(student, teacher) [N, V] in ``dtype``: the student is ``peaked_logits``, the teacher 0.7 x + noise (as the
    reference model of tests/test_dpo_gpu.py), so that kl is neither 0 nor huge; row ``hot`` (default: row 1, or the
    only row at N = 1 when V is odd) of both is scaled by ``hot_scale``."""
    x = peaked_logits(N, V, device, generator)
    t = 0.7 * x + peaked_logits(N, V, device, generator, scale=1.0, boost=0.0)
    if hot is None:
        hot = 1 if N > 1 else (0 if V % 2 else None)
    if hot is not None:
        x[hot] *= hot_scale
        t[hot] *= hot_scale
    return x.to(dtype), t.to(dtype)


W_CE, W_KL = 0.375, 0.15625  # gradient weights of the kd tests: different from each other, both exact in fp32
KD_TEMPS = (1.0, 2.0, 0.7)   # the T == 1 template arm, a dyadic and a non-dyadic temperature, one of them < 1
KD_SHAPES = [(N, V) for V in (7, 1001, 1003, 2056) for N in (1, 5, 300)] + [(5, 50265)]


def kd_case(N, V, dtype, labels=None, hot_scale=HOT_SCALE):
    """The inputs of one (N, V, dtype) of the distillation kernel tests, drawn on the CPU so that the CPU validation of
    the bounds (tests/test_loss_refs_cpu.py) sees exactly what the GPU tests feed the kernels: ``kd_logits`` (rounded
    to ``dtype``, held in it), ``edge_labels`` (or ``labels(N, V, generator)``), a student and a teacher
    ``dyadic_bias``.  Returns a dict of CPU tensors."""
    gen = torch.Generator().manual_seed(V * 1000 + N)
    s, t = kd_logits(N, V, "cpu", gen, dtype, hot_scale=hot_scale)
    lab = edge_labels(N, V, "cpu", gen) if labels is None else labels(N, V, gen)
    return dict(s=s, t=t, labels=lab, bs=dyadic_bias(V, "cpu", gen), bt=dyadic_bias(V, "cpu", gen, boost=1.0))


def kd_biases(case, bias):
    """(bias_s, bias_t) of ``kd_case`` for bias in {"none", "student", "both"}."""
    return (None if bias == "none" else case["bs"]), (case["bt"] if bias == "both" else None)


KD_CHUNK_ROWS = (1, 40)
INF_HOT_SCALE = 3.0  # the -inf cases: every banned column keeps a teacher weight fp32 can hold (asserted: > 1e-30)


def kd_chunk_labels(N, V, chunks, generator):
    """edge_labels, then per chunk its first and last column and, where it skips, the last re-covered column (owned by
    the earlier chunk) and the first column it owns: labels on both sides of every skip boundary."""
    labels = edge_labels(N, V, "cpu", generator)
    special = []
    for c0, n, skip in chunks:
        special += [c0, c0 + n - 1] + ([c0 + skip - 1, c0 + skip] if skip else [])
    if N == 1:
        labels[0] = next((c0 + skip for c0, _, skip in chunks if skip), chunks[-1][0])
    else:
        assert N >= 9 + len(special), (N, len(special))
        labels[9:9 + len(special)] = torch.tensor(special)
    return labels


def kd_banned_columns(V, chunks=None):
    """Columns that get -inf: column 0 (a scalar head); columns 0..15, which hold the whole first 16-B group of lane 0
    at any phase of the row (a head of <= 7 columns, then 8 bf16 or 4 fp32), so that a lane's running maximum is still
    -inf after a group; the last column (scalar tail); the middle peak; and, with a chunk table, the first column every
    skipping chunk owns when it lies inside a 4-group that straddles the skip boundary.  V = 7: columns 0, 3, 6."""
    if V < 32:
        return sorted({0, V // 2, V - 1})
    ban = set(range(16)) | {V // 2, V - 1}
    for c0, _, skip in chunks or []:
        if skip % 4:
            ban.add(c0 + skip)
    return sorted(ban)


def kd_ban(case, bias_s, bias_t, ban, who, V):
    """(bias_s, bias_t, labels) with -inf on the columns ``ban`` of the fp32 bias of ``who`` in {"teacher", "both",
    "student"} (a missing bias becomes zeros first) and every label that sits on a banned column moved to the nearest
    column that is not banned: -inf never lies on a valid row's label."""
    z = torch.zeros(V, dtype=F32, device=case["s"].device)
    b_s = (z if bias_s is None else bias_s).clone()
    b_t = (z if bias_t is None else bias_t).clone()
    if who in ("student", "both"):
        b_s[ban] = float("-inf")
    if who in ("teacher", "both"):
        b_t[ban] = float("-inf")
    free = torch.ones(V, dtype=torch.bool)
    free[ban] = False
    free = free.nonzero().view(-1)
    lab = case["labels"].clone()
    for i, y in enumerate(lab.tolist()):
        if 0 <= y < V and y in ban:
            lab[i] = free[(free - y).abs().argmin()].item()
    return b_s, b_t, lab
