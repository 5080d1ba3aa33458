"""Sliding-window attention kernels (csrc/attn_hd.hip, csrc/attn_f32.hip with ``window``): forward + backward against
the composite ``A._reference(..., window=w)`` on fp32 copies of the same values, at the bounds of
tests/test_attn_hd_gpu.py (bf16: rel-L2 2e-2 on the output, 3e-2 on dq / dk / dv, the bias gradient on the bucket
table) and of tests/test_attn_f32_gpu.py (fp32 against an fp64 composite: 2e-6 / 2e-5).  A spy asserts which binding
ran.  Two properties beyond parity: blocks outside the band are skipped, not masked (NaN poison outside the band never
reaches rows whose band blocks are clean), and row / key indices hold at 16K tokens."""
import pytest
import torch

from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops import attention as A
from distributed_llms_example_amd.ops.rng import attention_keep_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
_NAMES = ("attn_fwd", "attn_bwd", "attn_hd_fwd", "attn_hd_bwd", "attn_f32_fwd", "attn_f32_bwd")


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


class _Spy:
    """The native module with the attention bindings' calls recorded as (name, window argument)."""

    def __init__(self, calls, real):
        self.calls = calls
        self.real = real

    def __getattr__(self, n):
        real = getattr(self.real, n)
        if n in _NAMES:
            def f(*a, **kw):
                w = None
                if n not in ("attn_fwd", "attn_bwd"):  # the trailing `window` of attn_hd_* / attn_f32_*
                    pos = 9 if n.endswith("fwd") else 16
                    w = a[pos] if len(a) > pos else kw.get("window", -1)
                self.calls.append((n, w))
                return real(*a, **kw)
            return f
        return real


@pytest.fixture
def calls(monkeypatch):
    out = []
    spy = _Spy(out, _ext.native())
    monkeypatch.setattr(A._ext, "native", lambda: spy)
    return out


def _inputs(B, H, S, D, bias, kpm, seed, dtype=torch.bfloat16):
    torch.manual_seed(seed)
    qkv = torch.randn(B, S, 3, H, D, device=DEV).to(dtype)
    table = torch.randn(32, H, device=DEV) * 0.5 if bias else None
    mask = None
    if kpm:
        mask = torch.ones(B, S, dtype=torch.bool, device=DEV)
        if kpm == "first70":  # batch 0: only the first 70 keys are real
            mask[0, 70:] = False
        else:
            mask[0, S - S // 5:] = False
    return qkv, table, mask


def _run(qkv, table, mask, w, p, seed, packed, g, scale=1.0):
    """One native forward + backward: (o, dq, dk, dv, dtable)."""
    S = qkv.shape[1]
    x = qkv.clone().requires_grad_(True)
    tab = table.clone().requires_grad_(True) if table is not None else None
    lut = A.relative_bias_lut(tab, S, S, True, 32, 128) if tab is not None else None
    kw = dict(scale=scale, key_padding_mask=mask, bias_lut=lut, dropout_p=p, seed=seed, window=w)
    if packed:
        o = A.attention_qkv(x, **kw)
    else:
        o = A.attention(x[:, :, 0], x[:, :, 1], x[:, :, 2], **kw)
    (o.float() * g.float()).sum().backward()
    return o.detach(), x.grad[:, :, 0], x.grad[:, :, 1], x.grad[:, :, 2], (tab.grad if tab is not None else None)


def _oracle(qkv, table, mask, w, p, seed, g, scale=1.0):
    """The composite on fp32 copies: (o, dq, dk, dv, dtable)."""
    S = qkv.shape[1]
    x = qkv.detach().float().requires_grad_(True)
    tab = table.clone().requires_grad_(True) if table is not None else None
    lut = A.relative_bias_lut(tab, S, S, True, 32, 128) if tab is not None else None
    o = A._reference(x[:, :, 0], x[:, :, 1], x[:, :, 2], scale, False, mask, lut, p, seed, window=w)
    (o * g.float()).sum().backward()
    return o.detach(), x.grad[:, :, 0], x.grad[:, :, 1], x.grad[:, :, 2], (tab.grad if tab is not None else None)


def _check(tag, got, ref, tol_o=2e-2, tol_g=3e-2):
    errs = {n: _rel(a, b) for n, a, b in zip(("o", "dq", "dk", "dv", "dtable"), got, ref) if a is not None}
    print(f"[{tag}] {errs}")
    for n, e in errs.items():
        assert e < (tol_o if n == "o" else tol_g), (tag, n, e)


def _visible_rows(mask, B, S, w):
    """[B, S] bool: the query row has a key inside the window that is not padding."""
    ar = torch.arange(S, device=DEV)
    band = (ar[None, :] - ar[:, None]).abs() <= w
    keys = mask if mask is not None else torch.ones(B, S, dtype=torch.bool, device=DEV)
    return (band[None] & keys[:, None, :]).any(-1)


BF16_CASES = [
    # B, H, S, w, D, bias, kpm, p, packed
    (2, 3, 200, 127, 64, True, True, 0.1, True),      # LongT5's own call; D = 64 + window must not reach attn_fwd
    (2, 2, 333, 63, 64, True, False, 0.0, False),     # the loop bounds one short of, at and one past a block boundary
    (2, 2, 333, 64, 64, True, False, 0.0, False),
    (2, 2, 333, 65, 64, True, False, 0.0, False),
    (2, 2, 130, 5, 128, False, True, 0.0, False),     # band inside one block, ragged tail
    (1, 2, 300, 20, 96, True, True, 0.1, True),       # DP = 96; several band blocks with dropout
]


@pytest.mark.parametrize("B,H,S,w,D,bias,kpm,p,packed", BF16_CASES)
def test_window_bf16(B, H, S, w, D, bias, kpm, p, packed, calls):
    qkv, table, mask = _inputs(B, H, S, D, bias, kpm, seed=S * 7 + w + D)
    g = torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16)
    # padded rows further than w from the last real key see no key: the kernels return 0 there and the composite an
    # average over masked keys (the contract of csrc/attn_params.h; nothing downstream reads such rows), so they are
    # left out of the output comparison and carry no output gradient on either side
    vis = _visible_rows(mask, B, S, w)
    g[~vis] = 0
    got = _run(qkv, table, mask, w, p, 4242, packed, g)
    assert calls == [("attn_hd_fwd", w), ("attn_hd_bwd", w)], calls
    assert got[0].dtype == torch.bfloat16 and got[0].shape == (B, S, H, D)
    assert got[0][~vis].abs().max().item() == 0 if (~vis).any() else True
    ref = _oracle(qkv, table, mask, w, p, 4242, g)
    _check(f"window bf16 S={S} w={w} D={D}", (got[0][vis],) + got[1:], (ref[0][vis],) + ref[1:])


def test_window_zero_returns_the_values(calls):
    """w = 0: every row sees its own key only, so without dropout the output is v (P = 1 exactly; v passes through
    the fp32 accumulator and one bf16 rounding of a value that already is bf16)."""
    qkv, _, _ = _inputs(2, 2, 100, 40, False, False, seed=1)
    g = torch.randn(2, 100, 2, 40, device=DEV).to(torch.bfloat16)
    got = _run(qkv, None, None, 0, 0.0, 0, False, g, scale=40 ** -0.5)
    assert calls == [("attn_hd_fwd", 0), ("attn_hd_bwd", 0)], calls
    torch.testing.assert_close(got[0].float(), qkv[:, :, 2].float(), atol=0, rtol=2 ** -8)
    # dV = dO on the diagonal.  dS = P (dP - delta) with dP = delta = dO . v, formed by two different fp32 summations
    # of the same 40 products (an MFMA and the delta kernel): |dS| <= 40 * 2^-23 * sum |dO_d v_d| < 40 * 1.2e-7 * 40 * 1
    # on average terms, ~2e-4 at the extremes, and dQ = dS k / sqrt(40), dK = dS q / sqrt(40) with |k|, |q| < 5
    torch.testing.assert_close(got[3].float(), g.float(), atol=0, rtol=2 ** -8)
    assert got[1].abs().max().item() < 2e-4 and got[2].abs().max().item() < 2e-4
    ref = _oracle(qkv, None, None, 0, 0.0, 0, g, scale=40 ** -0.5)
    _check("window bf16 w=0", (got[0], got[3]), (ref[0], ref[3]))


def test_window_wider_than_the_sequence_is_no_window(calls):
    """w >= S masks nothing and skips nothing: bitwise the same call with window=None in the same family (head dim 40,
    csrc/attn_hd.hip either way).  The bias gradient is accumulated with fp32 atomics whose order differs between two
    launches of the very same call, so it is held to fp32 summation noise (1e-5) instead of bits."""
    B, H, S, D = 2, 3, 150, 40
    qkv, table, mask = _inputs(B, H, S, D, True, False, seed=2)
    g = torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16)
    a = _run(qkv, table, mask, 1000, 0.1, 77, False, g, scale=D ** -0.5)
    b = _run(qkv, table, mask, None, 0.1, 77, False, g, scale=D ** -0.5)
    c = _run(qkv, table, mask, S - 1, 0.1, 77, True, g, scale=D ** -0.5)
    assert [n for n, _ in calls] == ["attn_hd_fwd", "attn_hd_bwd"] * 3, calls
    assert [x for _, x in calls] == [1000, 1000, -1, -1, S - 1, S - 1], calls
    for n, x, y, z in zip(("o", "dq", "dk", "dv"), a, b, c):
        assert torch.equal(x, y), n
        assert torch.equal(z, y), n
    assert _rel(a[4], b[4]) < 1e-5 and _rel(c[4], b[4]) < 1e-5


def test_window_rows_without_a_visible_key(calls):
    """Batch 0 keeps keys < 70 only; with w = 20 its query rows >= 91 see no key (row 90, whose window starts at key 70,
    is the first such row): output row 0, LSE +inf, zero gradients, everything finite.  The other rows match the
    composite (whose rows without a visible key average over
    masked keys instead: their output gradient is zeroed on both sides, as nothing downstream reads such rows)."""
    B, H, S, D, w = 2, 2, 300, 64, 20
    qkv, _, mask = _inputs(B, H, S, D, False, "first70", seed=3)
    g = torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16)
    vis = _visible_rows(mask, B, S, w)
    assert vis[0, :90].all() and not vis[0, 90:].any() and vis[1].all()
    g[~vis] = 0
    got = _run(qkv, None, mask, w, 0.0, 0, True, g, scale=D ** -0.5)
    assert calls == [("attn_hd_fwd", w), ("attn_hd_bwd", w)], calls
    for t in got[:4]:
        assert torch.isfinite(t.float()).all()
    assert got[0][0, 90:].abs().max().item() == 0
    assert got[1][0, 90:].abs().max().item() == 0                                           # dq of the blind rows
    assert got[2][0, 70:].abs().max().item() == 0 and got[3][0, 70:].abs().max().item() == 0  # masked keys
    ref = _oracle(qkv, None, mask, w, 0.0, 0, g, scale=D ** -0.5)
    _check("window bf16 blind rows", (got[0][vis],) + got[1:4], (ref[0][vis],) + ref[1:4])
    x = qkv.detach()
    _, lse = _ext.native().attn_hd_fwd(x[:, :, 0], x[:, :, 1], x[:, :, 2], mask.to(torch.uint8), None, D ** -0.5, False,
                                       0.0, 0, w)
    assert torch.isposinf(lse[0, :, 90:]).all() and torch.isfinite(lse[0, :, :90]).all()
    assert torch.isfinite(lse[1]).all()


# ---------------------------------------------------------------------------------------------------------- fp32
def _ref64(q, k, v, scale, kpm, lut, p, seed, window):
    """fp64 composite with the band mask (tests/test_attn_f32_gpu.py _ref64 + ``|j - i| <= window``)."""
    B, S, H, D = q.shape
    qf, kf, vf = (t.double().permute(0, 2, 1, 3) for t in (q, k, v))
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    ar = torch.arange(S, device=q.device)
    if lut is not None:
        s = s + lut.double()[:, ar[None, :] - ar[:, None] + (S - 1)].unsqueeze(0)
    neg = torch.finfo(torch.float64).min
    if kpm is not None:
        s = s.masked_fill(~kpm.bool()[:, None, None, :], neg)
    s = s.masked_fill((ar[None, :] - ar[:, None]).abs() > window, neg)
    pr = torch.softmax(s, dim=-1)
    if p > 0.0:
        pr = pr * attention_keep_mask(seed, p, B, H, S, S, q.device).double() / (1.0 - p)
    return torch.matmul(pr, vf).permute(0, 2, 1, 3)


@pytest.mark.parametrize("S,w", [(200, 127), (333, 64)])
def test_window_fp32_matches_fp64(S, w, calls):
    B, H = 2, 3
    torch.manual_seed(S)
    q, k, v = (torch.randn(B, S, H, 64, device=DEV, requires_grad=True) for _ in range(3))
    kpm = torch.ones(B, S, dtype=torch.bool, device=DEV)
    kpm[0, -37:] = False
    lut = (torch.randn(H, 2 * S - 1, device=DEV) * 0.5).requires_grad_(True)
    o = A.attention(q, k, v, scale=1.0, key_padding_mask=kpm, bias_lut=lut, dropout_p=0.1, seed=1234, window=w)
    assert o.dtype == torch.float32
    g = torch.randn_like(o)
    grads = torch.autograd.grad(o, [q, k, v, lut], g)
    assert calls == [("attn_f32_fwd", w), ("attn_f32_bwd", w)], calls
    q64, k64, v64, lut64 = (t.detach().double().requires_grad_(True) for t in (q, k, v, lut))
    o64 = _ref64(q64, k64, v64, 1.0, kpm, lut64, 0.1, 1234, w)
    grads64 = torch.autograd.grad(o64, [q64, k64, v64, lut64], g.double())
    errs = {"o": _rel(o, o64)}
    errs.update({n: _rel(a, b) for n, a, b in zip(("dq", "dk", "dv", "dlut"), grads, grads64)})
    print(f"[window fp32 S={S} w={w}] {errs}")
    assert errs.pop("o") < 2e-6
    for n, e in errs.items():
        assert e < 2e-5, (n, e)
    # the composite (fp32) agrees with the fp64 one on the same band: the oracle of the bf16 cases
    oc = A._reference(q.detach(), k.detach(), v.detach(), 1.0, False, kpm, lut.detach(), 0.1, 1234, window=w)
    assert _rel(oc, o64) < 1e-5


# ------------------------------------------------------------------------------------------- skipping, not masking
def test_blocks_outside_the_band_are_not_loaded(calls):
    """K, V and dO rows 300 .. 699 are NaN.  With w = 10 the band blocks of query rows < 192 and >= 832 (and of keys
    < 128 and >= 896 in dK / dV) lie wholly outside the poisoned range, so a kernel that skips the other blocks gives
    finite values there, equal to the run on zero-filled inputs; one that loads and masks them gives NaN (0 * NaN in
    P V and dS^T Q)."""
    B, H, S, D, w = 1, 2, 1024, 64, 10
    qkv, _, _ = _inputs(B, H, S, D, False, False, seed=4)
    g = torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16)
    clean, gclean = qkv.clone(), g.clone()
    clean[:, 300:700, 1:] = 0
    gclean[:, 300:700] = 0
    qkv[:, 300:700, 1:] = float("nan")
    g[:, 300:700] = float("nan")
    x = qkv.clone().requires_grad_(True)
    o = A.attention(x[:, :, 0], x[:, :, 1], x[:, :, 2], scale=D ** -0.5, window=w)
    o.backward(g)
    assert calls == [("attn_hd_fwd", w), ("attn_hd_bwd", w)], calls
    dq, dk, dv = x.grad[:, :, 0], x.grad[:, :, 1], x.grad[:, :, 2]
    assert torch.isnan(o[:, 300:700].float()).all()  # the poison is real
    rows = torch.cat([torch.arange(0, 192), torch.arange(832, S)]).to(DEV)
    keys = torch.cat([torch.arange(0, 128), torch.arange(896, S)]).to(DEV)
    for n, t, idx in (("o", o, rows), ("dq", dq, rows), ("dk", dk, keys), ("dv", dv, keys)):
        assert torch.isfinite(t[:, idx].float()).all(), n
    ref = _oracle(clean, None, None, w, 0.0, 0, gclean, scale=D ** -0.5)
    got = (o.detach()[:, rows], dq[:, rows], dk[:, keys], dv[:, keys])
    _check("window bf16 poison", got, (ref[0][:, rows], ref[1][:, rows], ref[2][:, keys], ref[3][:, keys]))


# ------------------------------------------------------------------------------------------------- long indices
def _banded_oracle(qkv, table, w, g, chunk=1024):
    """The composite in ``chunk``-row pieces over the key slice [r0 - w, r1 + w] each: O(S w) memory.  The bias is
    built from the bucket table per piece (not through the LUT the kernel reads)."""
    B, S, _, H, D = qkv.shape
    x = qkv.detach().float().requires_grad_(True)
    tab = table.clone().requires_grad_(True)
    outs = []
    for r0 in range(0, S, chunk):
        r1 = min(S, r0 + chunk)
        k0, k1 = max(0, r0 - w), min(S, r1 + w)
        q = x[:, r0:r1, 0].permute(0, 2, 1, 3)
        k = x[:, k0:k1, 1].permute(0, 2, 1, 3)
        v = x[:, k0:k1, 2].permute(0, 2, 1, 3)
        rel = torch.arange(k0, k1, device=DEV)[None, :] - torch.arange(r0, r1, device=DEV)[:, None]
        s = torch.matmul(q, k.transpose(-1, -2)) + tab[A.relative_position_bucket(rel, True, 32, 128)].permute(2, 0, 1)
        s = s.masked_fill(rel.abs() > w, torch.finfo(torch.float32).min)
        outs.append(torch.matmul(torch.softmax(s, -1), v).permute(0, 2, 1, 3))
    o = torch.cat(outs, 1)
    (o * g.float()).sum().backward()
    return o.detach(), x.grad[:, :, 0], x.grad[:, :, 1], x.grad[:, :, 2], tab.grad


def test_window_at_16k_tokens(calls):
    B, H, S, D, w = 1, 2, 16384, 64, 127
    qkv, table, _ = _inputs(B, H, S, D, True, False, seed=5)
    g = torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16)
    got = _run(qkv, table, None, w, 0.0, 0, True, g)
    assert calls == [("attn_hd_fwd", w), ("attn_hd_bwd", w)], calls
    ref = _banded_oracle(qkv, table, w, g)
    _check("window bf16 S=16384", got, ref)
    # the last rows on their own: an index error far from the origin cannot hide in a whole-tensor norm
    _check("window bf16 S=16384 tail", tuple(t[:, -200:] for t in got[:4]), tuple(t[:, -200:] for t in ref[:4]))


# --------------------------------------------------------------------------------------------------- the binding
@pytest.mark.parametrize("family,dtype", [("attn_hd", torch.bfloat16), ("attn_f32", torch.float32)])
def test_binding_rejects_window_with_causal_or_rectangular(family, dtype):
    C = _ext.native()
    fwd, bwd = getattr(C, family + "_fwd"), getattr(C, family + "_bwd")
    q = torch.randn(1, 128, 2, 64, device=DEV).to(dtype)
    k = torch.randn(1, 192, 2, 64, device=DEV).to(dtype)
    k1, v1 = k[:, :128], k[:, 64:]
    o, lse = fwd(q, k1, v1, None, None, 0.125, False, 0.0, 0, 5)
    assert o.shape == q.shape
    o2, _ = fwd(q, k1, v1, None, None, 0.125, False, 0.0, 0)  # the trailing argument defaults to no window
    o3, _ = fwd(q, k1, v1, None, None, 0.125, False, 0.0, 0, window=-1)
    assert torch.equal(o2, o3) and not torch.equal(o, o2)
    with pytest.raises(RuntimeError, match="causal"):
        fwd(q, q, q, None, None, 1.0, True, 0.0, 0, 5)
    with pytest.raises(RuntimeError, match="Sq == Sk"):
        fwd(q, k, k, None, None, 1.0, False, 0.0, 0, 5)
    with pytest.raises(RuntimeError, match="causal"):
        bwd(o, q, q, q, o, lse, None, None, 1.0, True, 0.0, 0, False, window=5)
    with pytest.raises(RuntimeError, match="Sq == Sk"):
        bwd(o, q, k, k, o, lse, None, None, 1.0, False, 0.0, 0, False, window=5)
    torch.cuda.synchronize()


def test_unserved_windowed_call_takes_the_composite(calls):
    """Head dim 16 with a window: no kernel, the composite with the band mask (and no binding call)."""
    x = torch.randn(1, 70, 2, 16, device=DEV, dtype=torch.bfloat16)
    o = A.attention(x, x, x, window=3)
    assert calls == []
    assert torch.equal(o, A._reference(x, x, x, 1.0, False, None, None, 0.0, 0, window=3))
