"""The fp64 oracle of one beam-search step (csrc/beam.hip ``beam_topk``), its error bound, the checks the GPU tests
apply to a returned candidate list, and the input generators those tests share with tests/test_gen_refs_cpu.py.

Plain torch, CPU or GPU; the extension is never imported here.  Not a conftest: imported by name.
"""
import math

import torch

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
NINF = float("-inf")
U32 = 2.0 ** -24       # fp32 unit roundoff: |fl(a) - a| <= U32 |a|
EXP_ULPS = 1.0         # device expf / logf: 1 ulp (HIP's documented accuracy of both), i.e. 2 U32 relative
LOG_ULPS = 1.0
COMP_MARGIN = 4.0      # the project's comp rule: bound = 4 x what one fp32 evaluation may lose (tests/loss_refs.py)
BLOCK = 256            # threads of a beam_topk workgroup
VW_MAX = 8             # elements of one 16-B group (8 bf16 / 4 fp32)


# ---------------------------------------------------------------------------------------------------------- reference
def beam_step_ref(logits, beam_scores, seqs, cur, nb, ngram, ban_tok, force_tok):
    """cand64 [B, nb * V]: beam score + processed fp64 log-probability of every (beam, token) of every batch entry.

    logits [B * nb, V] as stored (bf16 / fp32) -> fp64 -> log_softmax over the whole row (processors act after the
    normaliser) -> bans (-inf): ``ban_tok`` (>= 0: the min_length eos ban) and no_repeat_ngram (``ngram`` = n > 0 and
    ``cur`` >= n: for every window i in 0 .. cur - n whose first n - 1 tokens equal the last n - 1 generated ones,
    seqs[row, cur - n + 1 : cur], the window's last token seqs[row, i + n - 1] is banned when it is a token id,
    0 <= id < V; any other id there is ignored) -> ``force_tok`` >= 0: the row becomes -inf but 0 at that token (a
    forced token wins over a ban) -> + beam score.  The bans are a direct loop over windows, written apart from
    models/generation.py."""
    rows, V = logits.shape
    B = rows // nb
    assert rows == B * nb
    logp = torch.log_softmax(logits.to(F64), dim=-1)
    if 0 <= ban_tok < V:
        logp[:, ban_tok] = NINF
    n = int(ngram)
    if n > 0 and cur >= n:
        for r, row in enumerate(seqs[:, :cur].tolist()):
            tail = row[cur - n + 1:cur]
            banned = sorted({row[i + n - 1] for i in range(cur - n + 1)
                             if row[i:i + n - 1] == tail and 0 <= row[i + n - 1] < V})
            if banned:
                logp[r, banned] = NINF
    if force_tok >= 0:
        logp = torch.full_like(logp, NINF)
        logp[:, force_tok] = 0.0
    return (beam_scores.to(F64).reshape(rows, 1) + logp).view(B, nb * V)


def beam_step_bound(logits, beam_scores, V):
    """Per-candidate absolute bound [B, nb * V] (``beam_scores`` is [B, nb]) on the kernel's fp32 score

        r = fl(bs + fl(fl(x - M) - logf(S^)))        M: the row maximum (exact), S^: the kernel's sum of exp(x - M)

    against the fp64 value bs + (x - M) - log S.  With u = 2^-24 (|fl(a) - a| <= u |a|):

      the three roundings     fl(x - M), fl(. - log S), fl(bs + .): each at most u on a magnitude that is at most
                              A = |bs| + |x - M| + |log S|                                             -> 3 u A
      logf                    LOG_ULPS ulp = 2 LOG_ULPS u relative on |log S|                 -> 2 LOG_ULPS u |log S|
      the error of S^         log turns a relative error dS of its argument into dS (first order; the factor
                              1 / (1 - dS) below covers the rest)                                      -> dS
      dS, the longest sequential chain into S^.  Every term is positive, so the relative error of the sum is at most
      that of its worst term, and a term collects:
        * one thread's walk: n_vis visits.  A thread owns whole 16-B groups (VW_MAX = 8 elements at most) at a stride
          of 256 groups and then one element of the tail: n_vis <= ceil(V / 256) + VW_MAX.  A visit that moves the
          running maximum is s = fl(fl(s e) + 1), two roundings and one expf; any other is s = fl(s + e), one rounding
          and one expf: at most (2 + 2 EXP_ULPS) u per visit;
        * the block reduction: fl(s expf(m - M)) (one rounding, one expf), the 6-step wave tree and 3 adds over the 4
          waves: (1 + 2 EXP_ULPS + 6 + 3) u;
        * expf's ARGUMENT error, once: the arguments a term passes through — its own v - m, every later rescale
          m_old - m_new, the final m - M — are all <= 0 and sum to v - M, each one rounded by at most u of itself, so
          together they are off by at most u |v - M| <= u R, R = max |x - M| over the row's finite logits; exp turns
          that absolute error into the same relative one                                               -> u R
      dS = u (n_vis (2 + 2 EXP_ULPS) + 10 + 2 EXP_ULPS + R)

      model = 3 u A + 2 LOG_ULPS u |log S| + dS / (1 - dS)
      bound = COMP_MARGIN model

    The model is what any fp32 evaluation of that chain may lose; the project's comp rule (tests/loss_refs.py) wants
    the fp32 torch composite at or under a quarter of a bound, hence COMP_MARGIN = 4 on the model.  What the bound must
    catch is far above it: logits rounded to bf16 first move a score by ~4e-3 |x|, a normaliser taken after the bans
    by the banned mass, against a bound of ~1e-5 at |score| ~ 30.

    A -inf logit is no candidate (bound 0: only -inf passes); a row without a finite logit likewise.  A forced token's
    score is bs itself, which the bound of its entry covers.  M, S, R are the fp64 reference's."""
    rows = logits.shape[0]
    assert logits.shape[1] == V and beam_scores.dim() == 2 and beam_scores.numel() == rows
    x = logits.to(F64)
    fin = torch.isfinite(x)
    M = x.max(dim=1, keepdim=True).values
    d = torch.where(fin, (x - M).abs(), torch.zeros_like(x))
    logS = torch.log(torch.exp(torch.where(fin, x - M, torch.full_like(x, NINF))).sum(1, keepdim=True))
    logS = torch.where(torch.isfinite(logS), logS.abs(), torch.zeros_like(logS))
    R = d.max(dim=1, keepdim=True).values
    n_vis = math.ceil(V / BLOCK) + VW_MAX
    dS = U32 * (n_vis * (2.0 + 2.0 * EXP_ULPS) + 10.0 + 2.0 * EXP_ULPS + R)
    A = beam_scores.to(F64).reshape(rows, 1).abs() + d + logS
    model = 3.0 * U32 * A + 2.0 * LOG_ULPS * U32 * logS + dS / (1.0 - dS)
    bound = COMP_MARGIN * model
    return torch.where(fin, bound, torch.zeros_like(bound)).view(beam_scores.shape[0], -1)


def fp64_order(cand64):
    """Every candidate of every batch entry by (score descending, flat index ascending): (values, indices)."""
    return torch.sort(cand64, dim=1, descending=True, stable=True)


def topk_ref(cand64, k_out, V):
    """A correct answer in the kernel's output form: the first k_out of ``fp64_order``, scores rounded to fp32; a slot
    without a finite candidate holds -inf."""
    v, i = fp64_order(cand64)
    pad = k_out - v.shape[1]
    if pad > 0:
        v = torch.cat([v, v.new_full((v.shape[0], pad), NINF)], 1)
        i = torch.cat([i, i.new_zeros((i.shape[0], pad))], 1)
    return v[:, :k_out].to(F32).contiguous(), i[:, :k_out].contiguous()


# -------------------------------------------------------------------------------------------------------------- checks
def check_beam_step(got_s, got_i, cand64, bound, nb, V, k_out):
    """Asserts, for every batch entry, that (got_s, got_i) [B, k_out] is a valid top-k_out of cand64 [B, nb * V]:

    * every non-finite score is -inf, and the finite ones come first: got_s is non-increasing, compared in fp32;
    * the finite entries' indices are distinct, each with beam < nb and 0 <= token < V;
    * each finite score is within ``bound`` of cand64 at its own index (a banned token, -inf there, can never pass);
    * the number of finite entries is min(k_out, number of finite candidates);
    * the list is complete: every candidate c that was not returned has
      cand64[c] <= cand64[last finite returned] + bound[c] + bound[last] (the kernel orders fp32 scores, each within
      its own bound of cand64: 2 x bound where the two bounds are equal).

    Returns the worst |score - cand64| / bound over all finite entries."""
    B = cand64.shape[0]
    assert got_s.shape == (B, k_out) and got_i.shape == (B, k_out), (got_s.shape, got_i.shape)
    assert got_s.dtype == F32 and got_i.dtype == torch.long
    assert cand64.shape == (B, nb * V) and bound.shape == cand64.shape and cand64.dtype == F64
    worst = 0.0
    for b in range(B):
        s, i, c, bd = got_s[b], got_i[b], cand64[b], bound[b]
        fin = torch.isfinite(s)
        assert (s[~fin] == NINF).all(), (b, s)
        assert (s[:-1] >= s[1:]).all(), (b, s)
        nf = int(fin.sum())
        want = min(k_out, int(torch.isfinite(c).sum()))
        assert nf == want, (b, nf, want)
        assert fin[:nf].all()
        if nf == 0:
            continue
        idx = i[:nf]
        assert (idx >= 0).all() and (idx // V < nb).all(), (b, idx)  # token = idx % V < V by construction of idx >= 0
        assert idx.unique().numel() == nf, (b, idx)
        ref, lim = c[idx], bd[idx]
        assert torch.isfinite(ref).all(), (b, idx, ref)
        err = (s[:nf].to(F64) - ref).abs()
        assert (err <= lim).all(), (b, idx, s[:nf], ref, lim)
        worst = max(worst, float((err / lim).max()))
        left = torch.ones_like(c, dtype=torch.bool)
        left[idx] = False
        last = idx[-1]
        over = left & (c > c[last] + bd + bd[last])
        assert not over.any(), (b, over.nonzero().view(-1)[:8], c[over][:8], c[last])
    return worst


def check_beam_order_exact(got_i, cand64, sep):
    """For inputs built with well-separated scores: got_i [B, k_out] equals the fp64 order by (score descending, flat
    index ascending) over the finite candidates, exactly.  ``sep`` is the per-candidate bound [B, nb * V]; the input is
    separated when any two DISTINCT fp64 scores among the first k_out + 1 of that order differ by more than 4 x the
    larger of their bounds — then rounding cannot reorder them, and equal fp64 scores (equal logits of one row, or of
    two identical rows with equal beam scores) are equal fp32 scores whose order is the tie rule's.  An input that is
    not separated fails here; it is not skipped."""
    B, k_out = got_i.shape
    v, order = fp64_order(cand64)
    for b in range(B):
        top = min(k_out + 1, int(torch.isfinite(v[b]).sum()))
        tv, tb = v[b, :top], sep[b][order[b, :top]]
        gap, lim = tv[:-1] - tv[1:], 4.0 * torch.maximum(tb[:-1], tb[1:])
        assert ((gap == 0) | (gap > lim)).all(), ("not separated", b, tv, lim)
        nf = min(k_out, top)
        assert torch.equal(got_i[b, :nf], order[b, :nf]), (b, got_i[b], order[b, :nf], tv)


# ---------------------------------------------------------------------------------------------------------- generators
def gen_of(seed):
    return torch.Generator().manual_seed(seed)


def step_inputs(B, nb, V, L, dtype, gen, alphabet=5, scale=3.0):
    """(logits [B * nb, V] in ``dtype``, beam_scores [B, nb] fp32, seqs [B * nb, L] int64) on the CPU: randn logits,
    and prefixes over a small token alphabet so that earlier n-grams repeat and bans fire."""
    logits = (torch.randn(B * nb, V, generator=gen) * scale).to(dtype)
    beam_scores = torch.randn(B, nb, generator=gen) * 2.0
    seqs = torch.randint(0, max(1, min(alphabet, V)), (B * nb, L), generator=gen)
    return logits, beam_scores, seqs


def plant_bad_ids(seqs, cur, V):
    """Ids that are no token (>= V, -1) at a few prefix positions of every row, the last generated one among them on
    the odd rows: as a window's last token they are ignored, inside a prefix they are values like any other."""
    seqs = seqs.clone()
    for r in range(seqs.shape[0]):
        for k, bad in enumerate((V, -1, V + 7)):
            p = (3 * r + 5 * k) % cur if cur else 0
            if cur:
                seqs[r, p] = bad
        if cur and r % 2:
            seqs[r, cur - 1] = -1
    return seqs


def echo_tail(seqs, cur, n, V, bad_ids):
    """Makes the n-gram ban fire in a known place: the last n - 1 generated tokens are copied to the row's start, so
    window 0 matches and bans the id at position n - 1, which is set to a token (row % 3), or with ``bad_ids``, on rows
    1, 5, 9, .., to V + 7: a matching window whose last id is no token and bans nothing.  Needs cur >= 2 n."""
    assert cur >= 2 * n
    seqs = seqs.clone()
    for r in range(seqs.shape[0]):
        seqs[r, :n - 1] = seqs[r, cur - n + 1:cur]
        seqs[r, n - 1] = V + 7 if (bad_ids and r % 4 == 1) else r % 3
    return seqs


LATE_WINDOW = 270  # a window index of the cur = 300 cases past the block's 256 threads: the loop's second trip


def late_window(logits, seqs, cur, n):
    """Makes the n-gram ban depend on a window only the window loop's SECOND trip reaches: window LATE_WINDOW (>= 256)
    is made to match the last n - 1 generated tokens, and its last id is token 100 + row, which appears nowhere else
    in the prefix and is raised to be the row's best logit by far.  A kernel that stops after 256 windows, or indexes
    the later ones wrongly, returns that token first.  Returns (logits, seqs, tokens [rows])."""
    assert LATE_WINDOW >= BLOCK and LATE_WINDOW + n - 1 < cur - n + 1 and logits.shape[1] > 100 + logits.shape[0]
    logits, seqs = logits.clone(), seqs.clone()
    toks = torch.arange(logits.shape[0]) + 100
    for r in range(seqs.shape[0]):
        seqs[r, LATE_WINDOW:LATE_WINDOW + n - 1] = seqs[r, cur - n + 1:cur]
        seqs[r, LATE_WINDOW + n - 1] = toks[r]
        logits[r, toks[r]] = 20.0
    return logits, seqs, toks


def ban_set(row, cur, n, V, windows=None):
    """The token ids one row's n-gram ban removes, from the first ``windows`` windows only (None: all cur - n + 1)."""
    if n <= 0 or cur < n:
        return set()
    row = [int(t) for t in row[:cur]]
    last = cur - n + 1 if windows is None else min(windows, cur - n + 1)
    return {row[i + n - 1] for i in range(last) if row[i:i + n - 1] == row[cur - n + 1:cur] and 0 <= row[i + n - 1] < V}


def best_token(logits):
    """The best token of row 0 (to aim ``ban_tok`` at)."""
    return int(logits[0].float().argmax())


def ninf_third(logits, gen):
    """A third of every row at -inf."""
    mask = torch.rand(logits.shape, generator=gen) < 1.0 / 3.0
    return logits.masked_fill(mask, NINF)


def ninf_head(logits, head=300):
    """Row 1's first ``head`` logits at -inf: thread 0's running maximum starts at -inf and stays there a while."""
    logits = logits.clone()
    logits[1, :head] = NINF
    return logits


def step1_scores(B, nb):
    """The beam scores of the first step (_beam_search_device): 0 for beam 0, -1e9 for the others."""
    s = torch.full((B, nb), -1e9)
    s[:, 0] = 0.0
    return s


def dead_row(logits, seqs, cur, row):
    """With ngram = 1 every token of the prefix is banned; ``row``'s other logits become -inf, so the row has no
    candidate at all."""
    logits = logits.clone()
    V = logits.shape[1]
    seen = torch.zeros(V, dtype=torch.bool)
    ids = seqs[row, :cur]
    seen[ids[(ids >= 0) & (ids < V)]] = True
    logits[row] = torch.where(seen, logits[row], torch.full_like(logits[row], NINF))
    return logits


TIE_TOKENS = (7, 8, 255, 256, 511, 512, 2050)  # pairs across a 16-B group (thread) boundary, 7|8 and 255|256, across a
#                                               wave boundary, 511|512 (64 threads x 8 bf16), and the last tail token


def tie_inputs(B, nb, V, gen):
    """bf16 logits on a grid of 0.5 in [-8, 2] with the top value 4.0 at TIE_TOKENS and 3.5 at two more tokens of
    every row; beams 0 and 1 of every batch entry hold identical rows and equal beam scores; beam scores on a grid of
    0.25.  Equal scores are then exact ties and distinct ones lie far apart (tests check that)."""
    assert V > max(TIE_TOKENS) and nb >= 2
    x = torch.randint(-16, 5, (B * nb, V), generator=gen).to(F32) * 0.5
    x[:, list(TIE_TOKENS)] = 4.0
    x[:, [100, 1033]] = 3.5
    x = x.view(B, nb, V)
    x[:, 1] = x[:, 0]
    bs = torch.randint(-8, 1, (B, nb), generator=gen).to(F32) * 0.25
    bs[:, 1] = bs[:, 0]
    if nb > 2:  # a third beam below the tied pair on even entries (the pair's tie decides the list), above it on odd
        bs[:, 2] = bs[:, 0] + torch.where(torch.arange(B) % 2 == 0, -0.25, 0.25)
    seqs = torch.randint(0, 5, (B * nb, 8), generator=gen)
    return x.view(B * nb, V).to(BF16), bs, seqs


# ---- kv_reorder
def kv_bits(lk, rows, max_len, hd, gen):
    """A cache of random BIT PATTERNS (NaNs and infinities included) as bf16 [lk, rows, max_len, hd]."""
    return torch.randint(-32768, 32768, (lk, rows, max_len, hd), generator=gen, dtype=torch.int32).to(torch.int16) \
        .view(BF16)


def kv_perm(kind, B, nb, gen):
    """src [B * nb]: row r takes row src[r] of its own group.  ``kind``: identity, swap (the first two rows), cycle3,
    first (every row takes the group's row 0), last, random, mixed (even groups keep their rows, odd ones move)."""
    j = torch.arange(nb)
    if kind == "identity":
        g = j
    elif kind == "swap":
        g = j.clone()
        if nb >= 2:
            g[0], g[1] = 1, 0
    elif kind == "cycle3":
        g = j.clone()
        if nb >= 3:
            g[0], g[1], g[2] = 1, 2, 0
        elif nb == 2:
            g[0], g[1] = 1, 0
    elif kind == "first":
        g = torch.zeros(nb, dtype=torch.long)
    elif kind == "last":
        g = torch.full((nb,), nb - 1, dtype=torch.long)
    else:
        g = None
    base = torch.arange(B).view(B, 1) * nb
    if g is not None:
        return (base + g.view(1, nb)).reshape(-1)
    src = base + torch.randint(0, nb, (B, nb), generator=gen)
    if kind == "mixed":
        keep = (torch.arange(B) % 2 == 0).view(B, 1)
        src = torch.where(keep, base + j.view(1, nb), src)
    else:
        assert kind == "random"
    return src.reshape(-1)


def kv_reorder_ref(cache, src, n):
    """index_select of the live prefix on a clone; positions >= n untouched."""
    ref = cache.clone()
    ref[:, :, :n] = cache[:, :, :n].index_select(1, src)
    return ref


# ---- the adversarial top-k row of tests/test_sampling_gpu.py
def edge_topk_row(V, top_k):
    """One fp32 row for the sampling kernel's coarse pre-temperature top-k cut.  Sorted by score it is: top_k - 1
    tokens well above 2.0; the k-th at exactly 2.0 (the lowest value of a binade: a radix bin edge in any binning of
    the bit pattern); then the values 1, 2 and 3 ulps below 2.0 (in the binade below the edge), twice each; the body
    below 1.0.  Returns (row [1, V], the k-th token, the six below-edge tokens).  After division by a temperature such
    as 1.7 some of the below-edge values round to the quotient of 2.0 itself, and the composite keeps those ties with
    the k-th value (tests/test_gen_refs_cpu.py confirms that it does; at 3.0 none ties: 2/3 rounds up by a third of
    an ulp and the next value below lands exactly one ulp under it)."""
    assert V >= top_k + 64
    x = torch.linspace(-3.0, 0.9, V, dtype=F32).view(1, V).clone()
    pos = [(37 * q + 11) % V for q in range(top_k + 6)]
    assert len(set(pos)) == len(pos)
    for q in range(top_k - 1):
        x[0, pos[q]] = 2.5 + 0.25 * q
    x[0, pos[top_k - 1]] = 2.0
    two = torch.tensor(2.0, dtype=F32)
    below = []
    v = two
    for _ in range(3):
        v = torch.nextafter(v, torch.tensor(0.0, dtype=F32))
        below.append(v)
    for q in range(6):
        x[0, pos[top_k + q]] = below[q % 3]
    return x, pos[top_k - 1], pos[top_k:]


# ---- the cases of tests/test_beam_kernels_gpu.py, shared with tests/test_gen_refs_cpu.py
ARMS = [(1, 2), (2, 4), (3, 6), (4, 8), (5, 10), (8, 16), (1, 1), (2, 3), (1, 16)]  # (nb, k_out): K = 2, 4, 8, 16
WALK_V = [5, 250, 2051, 4105]  # < a block; a tail only; one 16-B trip + tail; two trips (256 x 8 bf16 = 2048 a trip)
BIG_V = 250112                 # the largest real vocabulary (mt5): the longest bitmap
BAN_N = [1, 2, 3, 5]
BAN_CUR = ["n-1", "n", 17, 300]  # no window yet; exactly one; a few; more windows than the block's 256 threads


def _case(logits, beam_scores, seqs, cur, nb, k_out, ngram=0, ban_tok=-1, force_tok=-1):
    return dict(logits=logits, beam_scores=beam_scores, seqs=seqs, cur=cur, nb=nb, k_out=k_out, ngram=ngram,
                ban_tok=ban_tok, force_tok=force_tok)


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def beam_case(name, bad_ids=True):
    """The inputs of one named case, on the CPU.  ``bad_ids`` False leaves the prefixes of the ban cases free of ids
    that are no token (the torch composite cannot index with them)."""
    g = gen_of(_seed(name))
    kind, _, rest = name.partition("-")
    if kind == "arm":
        nb, k_out = map(int, rest.split("-"))
        lg, bs, sq = step_inputs(3, nb, 2051, 24, BF16, g)
        return _case(lg, bs, sq, 17, nb, k_out, ngram=2)
    if kind == "walk":
        v, dt = rest.split("-")
        V, dtype = int(v), {"bf16": BF16, "fp32": F32}[dt]
        lg, bs, sq = step_inputs(2 if V == BIG_V else 3, 2, V, 24, dtype, g)
        return _case(lg, bs, sq, 17, 2, 4, ngram=3)
    if kind == "tiny":  # V < k_out: fewer candidates than slots
        nb, k_out = map(int, rest.split("-"))
        lg, bs, sq = step_inputs(3, nb, 5, 24, F32, g)
        return _case(lg, bs, sq, 17, nb, k_out, ngram=2)
    if kind == "ban":
        n, c = rest.split("-", 1)
        n = int(n)
        cur = {"n-1": n - 1, "n": n}.get(c) if c in ("n-1", "n") else int(c)
        V = 250
        lg, bs, sq = step_inputs(3, 2, V, 320, F32, g, alphabet=3)
        if bad_ids:
            sq = plant_bad_ids(sq, cur, V)
        if cur >= 2 * n:
            sq = echo_tail(sq, cur, n, V, bad_ids)
        if cur == 300:
            lg, sq, _ = late_window(lg, sq, cur, n)
        return _case(lg, bs, sq, cur, 2, 4, ngram=n)
    if kind == "bantok":
        lg, bs, sq = step_inputs(3, 2, 2051, 24, BF16, g)
        return _case(lg, bs, sq, 17, 2, 4, ngram=2, ban_tok=best_token(lg))
    if kind == "dead":  # "dead-2": beam 1 of entry 0 has no candidate; "dead-1": entry 1 has none at all
        nb = int(rest)
        lg, bs, sq = step_inputs(3, nb, 250, 24, F32, g)
        return _case(dead_row(lg, sq, 17, 1), bs, sq, 17, nb, 2 * nb, ngram=1)
    if kind == "ninf":
        lg, bs, sq = step_inputs(3, 2, 2051, 24, BF16 if rest == "third" else F32, g)
        lg = ninf_third(lg, g) if rest == "third" else ninf_head(lg, 300)
        return _case(lg, bs, sq, 17, 2, 4, ngram=2)
    if kind == "step1":
        lg, _, sq = step_inputs(3, 4, 2051, 24, BF16, g)
        return _case(lg, step1_scores(3, 4), sq, 1, 4, 8, ngram=2)
    if kind == "force":  # bans active, and aimed at the forced token: the forced token wins
        lg, bs, sq = step_inputs(3, 2, 2051, 24, BF16, g)
        if rest == "bos":
            return _case(lg, step1_scores(3, 2), sq, 1, 2, 4, ngram=1, ban_tok=0, force_tok=0)
        sq[:, :17] = 2  # every window of the prefix bans token 2, the forced one
        return _case(lg, bs, sq, 17, 2, 4, ngram=2, ban_tok=2, force_tok=2)
    if kind == "tie":
        if rest == "wide":  # k_out past the 7 tied tokens of a beam: both tied beams and the tail token in one list
            lg, bs, sq = tie_inputs(3, 2, 2051, g)
            return _case(lg, bs, sq, 5, 2, 16)
        lg, bs, sq = tie_inputs(3, 3, 2051, g)
        return _case(lg, bs, sq, 5, 3, 6)
    raise KeyError(name)


ARM_CASES = [f"arm-{nb}-{k}" for nb, k in ARMS]
WALK_CASES = ([f"walk-{V}-{dt}" for V in WALK_V for dt in ("bf16", "fp32")] + [f"walk-{BIG_V}-bf16"]
              + ["tiny-1-8", "tiny-1-16", "tiny-2-16"])
BAN_CASES = [f"ban-{n}-{c}" for n in BAN_N for c in BAN_CUR] + ["bantok-best", "dead-2", "dead-1"]
SPECIAL_CASES = ["ninf-third", "ninf-head", "step1-scores", "force-bos", "force-eos"]
TIE_CASES = ["tie-grid", "tie-wide"]
ALL_CASES = ARM_CASES + WALK_CASES + BAN_CASES + SPECIAL_CASES + TIE_CASES


def case_ref(c):
    """(cand64, bound) of a case."""
    V = c["logits"].shape[1]
    cand = beam_step_ref(c["logits"], c["beam_scores"], c["seqs"], c["cur"], c["nb"], c["ngram"], c["ban_tok"],
                         c["force_tok"])
    return cand, beam_step_bound(c["logits"], c["beam_scores"], V)
