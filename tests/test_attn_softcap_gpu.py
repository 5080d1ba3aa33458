"""Soft-capped attention kernels (csrc/attn_hd.hip, csrc/attn_f32.hip with ``softcap``): forward + backward with the
method, spy and bounds of tests/test_attn_window_gpu.py / tests/test_attn_global_gpu.py — bf16 against the composite
``A._reference(..., softcap=c)`` on fp32 copies of the same values (rel-L2 2e-2 on the output, 3e-2 on dq / dk / dv), fp32
against an fp64 composite written here (2e-6 / 2e-5).

Inputs: ``randn`` q and k at ``scale = 1`` and ``c = 5``, so the scores have a standard deviation of sqrt(D) (8 at head
dim 64) and about half of the visible ones lie beyond the cap — every case asserts on the reference's scores that
between 20 % and 80 % do, so that the saturated and the linear range of the tanh are both exercised.  One case per family
runs ``c = 50`` at ``scale = D ** -0.5`` (|s| / c < 0.1: the near-linear range, where a tanh built as ``1 - 2 / (1 +
exp(2z))`` cancels — in fp32 that is an error above the bound).

Rows without a visible key are compared on neither side; every case names them, and in the cases here there are none
(``vis.all()``: padding is a suffix of the keys, and no window case is padded)."""
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
    """The native module with the attention bindings' calls recorded as (name, softcap keyword or None)."""

    def __init__(self, calls, real):
        self.calls = calls
        self.real = real

    def __getattr__(self, n):
        real = getattr(self.real, n)
        if n in _NAMES:
            def f(*a, **kw):
                self.calls.append((n, kw.get("softcap")))
                return real(*a, **kw)
            return f
        return real


@pytest.fixture
def calls(monkeypatch):
    out = []
    spy = _Spy(out, _ext.native())
    monkeypatch.setattr(A._ext, "native", lambda: spy)
    return out


def _inputs(B, H, Sq, Sk, D, pad, seed, dtype=torch.bfloat16):
    """q [B, Sq, H, D], kv [B, Sk, 2, H, D] (for Sq == Sk also usable as one packed qkv) and a suffix padding mask."""
    torch.manual_seed(seed)
    q = torch.randn(B, Sq, H, D, device=DEV).to(dtype)
    kv = torch.randn(B, Sk, 2, H, D, device=DEV).to(dtype)
    mask = None
    if pad:
        mask = torch.ones(B, Sk, dtype=torch.bool, device=DEV)
        mask[0, Sk - Sk // 5:] = False
    return q, kv, mask


def _visible(mask, B, Sq, Sk, causal, window):
    """[B, Sq, Sk] bool: key j is visible to query i."""
    i = torch.arange(Sq, device=DEV)[:, None]
    j = torch.arange(Sk, device=DEV)[None, :]
    vis = torch.ones(Sq, Sk, dtype=torch.bool, device=DEV)
    if causal:
        vis &= j <= i + (Sk - Sq)
    if window is not None:
        vis &= (j - i).abs() <= window
    vis = vis[None].expand(B, -1, -1)
    return vis & mask[:, None, :] if mask is not None else vis


def _beyond_cap(q, kv, scale, c, vis):
    """Fraction of the visible scores of the reference with |s| > c."""
    s = torch.einsum("bihd,bjhd->bhij", q.float(), kv[:, :, 0].float()) * scale
    sel = vis[:, None].expand_as(s)
    return ((s.abs() > c) & sel).sum().item() / sel.sum().item()


def _run(q, kv, mask, c, g, scale, causal=False, window=None, p=0.0, seed=0, mode="sep"):
    """One native forward + backward: (o, dq, dk, dv)."""
    qx = q.clone().requires_grad_(True)
    kx = kv.clone().requires_grad_(True)
    kw = dict(scale=scale, causal=causal, key_padding_mask=mask, dropout_p=p, seed=seed, window=window, softcap=c)
    if mode == "qkv":  # one packed tensor, as the fused projection gives it
        x = torch.cat((q.unsqueeze(2), kv), 2).clone().requires_grad_(True)
        o = A.attention_qkv(x, **kw)
        (o.float() * g.float()).sum().backward()
        return o.detach(), x.grad[:, :, 0], x.grad[:, :, 1], x.grad[:, :, 2]
    if mode == "q_kv":
        o = A.attention_q_kv(qx, kx, **kw)
    else:
        o = A.attention(qx, kx[:, :, 0], kx[:, :, 1], **kw)
    (o.float() * g.float()).sum().backward()
    return o.detach(), qx.grad, kx.grad[:, :, 0], kx.grad[:, :, 1]


def _oracle(q, kv, mask, c, g, scale, causal=False, window=None, p=0.0, seed=0):
    """The composite on fp32 copies: (o, dq, dk, dv)."""
    qx = q.detach().float().requires_grad_(True)
    kx = kv.detach().float().requires_grad_(True)
    o = A._reference(qx, kx[:, :, 0], kx[:, :, 1], scale, causal, mask, None, p, seed, window=window, softcap=c)
    (o * g.float()).sum().backward()
    return o.detach(), qx.grad, kx.grad[:, :, 0], kx.grad[:, :, 1]


def _check(tag, got, ref, tol_o=2e-2, tol_g=3e-2):
    errs = {n: _rel(a, b) for n, a, b in zip(("o", "dq", "dk", "dv"), got, ref)}
    print(f"[{tag}] {errs}")
    for n, e in errs.items():
        assert e < (tol_o if n == "o" else tol_g), (tag, n, e)


BF16_CASES = [
    # tag, B, H, Sq, Sk, D, pad, causal, window, p, mode
    ("plain packed", 2, 3, 333, 333, 64, False, False, None, 0.0, "qkv"),
    ("padded", 2, 3, 333, 333, 64, True, False, None, 0.0, "sep"),
    ("padded dropout packed", 2, 3, 333, 333, 64, True, False, None, 0.1, "qkv"),
    ("dropout", 2, 3, 333, 333, 64, False, False, None, 0.1, "sep"),
    ("causal", 2, 3, 200, 200, 64, False, True, None, 0.0, "qkv"),
    ("decode 1", 2, 3, 1, 70, 64, False, True, None, 0.0, "sep"),
    ("decode 5", 2, 3, 5, 70, 64, False, True, None, 0.0, "sep"),
    ("cross padded", 2, 3, 9, 333, 64, True, False, None, 0.0, "q_kv"),
    ("window 63", 2, 3, 333, 333, 64, False, False, 63, 0.0, "qkv"),
    ("window 64", 2, 3, 333, 333, 64, False, False, 64, 0.0, "sep"),
    ("window 65", 2, 3, 333, 333, 64, False, False, 65, 0.1, "qkv"),
    ("head dim 40", 2, 3, 333, 333, 40, True, False, None, 0.0, "sep"),
    ("head dim 96", 2, 3, 200, 200, 96, False, True, None, 0.1, "qkv"),
    ("head dim 128", 2, 3, 333, 333, 128, False, False, 64, 0.0, "qkv"),
]


@pytest.mark.parametrize("tag,B,H,Sq,Sk,D,pad,causal,window,p,mode", BF16_CASES, ids=[c[0] for c in BF16_CASES])
def test_softcap_bf16(tag, B, H, Sq, Sk, D, pad, causal, window, p, mode, calls):
    c, scale = 5.0, 1.0
    q, kv, mask = _inputs(B, H, Sq, Sk, D, pad, seed=Sq * 7 + Sk + D)
    vis = _visible(mask, B, Sq, Sk, causal, window)
    assert vis.any(-1).all()  # no row without a visible key in these cases
    frac = _beyond_cap(q, kv, scale, c, vis)
    assert 0.2 < frac < 0.8, frac
    g = torch.randn(B, Sq, H, D, device=DEV).to(torch.bfloat16)
    got = _run(q, kv, mask, c, g, scale, causal, window, p, 4242, mode)
    assert calls == [("attn_hd_fwd", c), ("attn_hd_bwd", c)], calls  # head dim 64 included: csrc/attn.hip has no cap
    assert got[0].dtype == torch.bfloat16 and got[0].shape == (B, Sq, H, D)
    ref = _oracle(q, kv, mask, c, g, scale, causal, window, p, 4242)
    _check(f"softcap bf16 {tag} beyond={frac:.2f}", got, ref)
    # the cap is what is being tested: the uncapped call computes something else
    assert _rel(A._reference(q.float(), kv[:, :, 0].float(), kv[:, :, 1].float(), scale, causal, mask, None, 0.0, 0,
                             window=window), ref[0]) > 0.1 or p > 0


def test_softcap_bf16_near_linear(calls):
    """c = 50 at scale = D ** -0.5: |s| / c stays below 0.1."""
    B, H, S, D, c = 2, 3, 333, 64, 50.0
    q, kv, mask = _inputs(B, H, S, S, D, True, seed=11)
    g = torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16)
    got = _run(q, kv, mask, c, g, D ** -0.5, mode="qkv")
    assert calls == [("attn_hd_fwd", c), ("attn_hd_bwd", c)], calls
    _check("softcap bf16 c=50", got, _oracle(q, kv, mask, c, g, D ** -0.5))


def test_no_cap_is_the_call_without_the_argument(calls):
    """``softcap=None`` is bit for bit the call without the argument, in the kernels that served it before (head dim
    64: csrc/attn.hip; a window: csrc/attn_hd.hip without a cap argument); only a cap reaches the capped instantiation."""
    B, H, S, D = 2, 3, 200, 64
    q, kv, mask = _inputs(B, H, S, S, D, True, seed=12)
    g = torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16)
    for window, names in ((None, ["attn_fwd", "attn_bwd"]), (20, ["attn_hd_fwd", "attn_hd_bwd"])):
        del calls[:]
        a = _run(q, kv, mask, None, g, 0.125, window=window, p=0.1, seed=5, mode="qkv")
        x = torch.cat((q.unsqueeze(2), kv), 2).clone().requires_grad_(True)
        o = A.attention_qkv(x, scale=0.125, key_padding_mask=mask, dropout_p=0.1, seed=5, window=window)
        (o.float() * g.float()).sum().backward()
        assert calls == [(n, None) for n in names] * 2, calls
        for t, u in zip(a, (o.detach(), x.grad[:, :, 0], x.grad[:, :, 1], x.grad[:, :, 2])):
            assert torch.equal(t, u)
    del calls[:]
    b = _run(q, kv, mask, 5.0, g, 0.125, mode="qkv")
    assert calls == [("attn_hd_fwd", 5.0), ("attn_hd_bwd", 5.0)], calls
    plain = _run(q, kv, mask, None, g, 0.125, mode="qkv")  # the same call (no window, no dropout) without the cap
    assert not torch.equal(b[0], plain[0])


# ---------------------------------------------------------------------------------------------------------- fp32
def _ref64(q, k, v, scale, c, kpm, causal, window, p, seed):
    """fp64 composite with the cap before every mask."""
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    qf, kf, vf = (t.double().permute(0, 2, 1, 3) for t in (q, k, v))
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    s = c * torch.tanh(s / c)
    neg = torch.finfo(torch.float64).min
    vis = _visible(kpm, B, Sq, Sk, causal, window)
    s = s.masked_fill(~vis[:, None], neg)
    pr = torch.softmax(s, dim=-1)
    if p > 0.0:
        pr = pr * attention_keep_mask(seed, p, B, H, Sq, Sk, q.device).double() / (1.0 - p)
    return torch.matmul(pr, vf).permute(0, 2, 1, 3)


FP32_CASES = [
    # tag, Sq, Sk, pad, causal, window, p, c, scale
    ("padded dropout", 333, 333, True, False, None, 0.1, 5.0, 1.0),
    ("causal", 200, 200, False, True, None, 0.0, 5.0, 1.0),
    ("decode 5", 5, 70, False, True, None, 0.0, 5.0, 1.0),
    ("cross padded", 9, 333, True, False, None, 0.0, 5.0, 1.0),
    ("window 64", 333, 333, False, False, 64, 0.0, 5.0, 1.0),
    ("near linear", 333, 333, True, False, None, 0.0, 50.0, 0.125),  # exposes a cancelling tanh
]


@pytest.mark.parametrize("tag,Sq,Sk,pad,causal,window,p,c,scale", FP32_CASES, ids=[c[0] for c in FP32_CASES])
def test_softcap_fp32_matches_fp64(tag, Sq, Sk, pad, causal, window, p, c, scale, calls):
    B, H, D = 2, 3, 64
    q, kv, mask = _inputs(B, H, Sq, Sk, D, pad, seed=Sq + 3 * Sk, dtype=torch.float32)
    vis = _visible(mask, B, Sq, Sk, causal, window)
    assert vis.any(-1).all()
    frac = _beyond_cap(q, kv, scale, c, vis)
    assert (0.2 < frac < 0.8) if c == 5.0 else frac == 0.0, frac
    q, k, v = (t.clone().requires_grad_(True) for t in (q, kv[:, :, 0], kv[:, :, 1]))
    o = A.attention(q, k, v, scale=scale, causal=causal, key_padding_mask=mask, dropout_p=p, seed=1234, window=window,
                    softcap=c)
    assert o.dtype == torch.float32
    g = torch.randn_like(o)
    grads = torch.autograd.grad(o, [q, k, v], g)
    assert calls == [("attn_f32_fwd", c), ("attn_f32_bwd", c)], calls
    q64, k64, v64 = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    o64 = _ref64(q64, k64, v64, scale, c, mask, causal, window, p, 1234)
    grads64 = torch.autograd.grad(o64, [q64, k64, v64], g.double())
    errs = {"o": _rel(o, o64)}
    errs.update({n: _rel(a, b) for n, a, b in zip(("dq", "dk", "dv"), grads, grads64)})
    print(f"[softcap fp32 {tag} beyond={frac:.2f}] {errs}")
    assert errs.pop("o") < 2e-6
    for n, e in errs.items():
        assert e < 2e-5, (n, e)
    # the composite (fp32) agrees with the fp64 one: the oracle of the bf16 cases
    oc = A._reference(q.detach(), k.detach(), v.detach(), scale, causal, mask, None, p, 1234, window=window, softcap=c)
    assert _rel(oc, o64) < 1e-5


# --------------------------------------------------------------------------------------------------- the binding
@pytest.mark.parametrize("family,dtype", [("attn_hd", torch.bfloat16), ("attn_f32", torch.float32)])
def test_binding_rejects_what_the_cap_does_not_compose_with(family, dtype):
    C = _ext.native()
    fwd, bwd = getattr(C, family + "_fwd"), getattr(C, family + "_bwd")
    B, S, H, D = 1, 128, 2, 64
    q = torch.randn(B, S, H, D, device=DEV).to(dtype)
    o, lse = fwd(q, q, q, None, None, 0.125, False, 0.0, 0, softcap=5.0)
    o0, _ = fwd(q, q, q, None, None, 0.125, False, 0.0, 0)  # the trailing keyword defaults to no cap
    o1, _ = fwd(q, q, q, None, None, 0.125, False, 0.0, 0, softcap=0.0)
    assert torch.equal(o0, o1) and not torch.equal(o, o0)
    lut = torch.zeros(H, 2 * S - 1, device=DEV)
    sg = A.segments(torch.zeros(B, S, dtype=torch.int32, device=DEV))
    gk = A.global_keys(torch.zeros(B, S, dtype=torch.uint8, device=DEV))
    bl = A.block_lists([[[0, 1], [0, 1]]], block=64).tables(q.device, S, S)
    extra = {
        "bias LUT": dict(args=(lut,), kw={}),
        "segments": dict(args=(None,), kw=dict(q_seg=sg.ids, k_seg=sg.ids, q_blk=sg.blk, k_blk=sg.blk)),
        "global keys": dict(args=(None,), kw=dict(window=5, k_glob=gk.flags, k_gblk=gk.blk)),
        "block lists": dict(args=(None,), kw=bl),
    }
    for what, e in extra.items():
        with pytest.raises(RuntimeError, match=f"soft cap with .*{what}"):
            fwd(q, q, q, None, *e["args"], 0.125, False, 0.0, 0, softcap=5.0, **e["kw"])
        with pytest.raises(RuntimeError, match=f"soft cap with .*{what}"):
            bwd(o, q, q, q, o, lse, None, *e["args"], 0.125, False, 0.0, 0, False, softcap=5.0, **e["kw"])
        fwd(q, q, q, None, *e["args"], 0.125, False, 0.0, 0, **e["kw"])  # served without the cap
    with pytest.raises(RuntimeError, match="softcap"):
        fwd(q, q, q, None, None, 0.125, False, 0.0, 0, softcap=-1.0)
    if family == "attn_hd":
        q32 = torch.randn(B, S, H, 32, device=DEV).to(dtype)
        with pytest.raises(RuntimeError, match="soft cap at head dim 32"):
            fwd(q32, q32, q32, None, None, 0.125, False, 0.0, 0, softcap=5.0)
        fwd(q32, q32, q32, None, None, 0.125, False, 0.0, 0)
    torch.cuda.synchronize()


def test_unserved_capped_calls_take_the_composite(calls):
    """A cap with a bias LUT, segments, global keys or block lists, and bf16 at head dims 32 and 16: the composite, and
    no binding call."""
    B, S, H, D = 1, 128, 2, 64
    x = torch.randn(B, S, H, D, device=DEV, dtype=torch.bfloat16)
    table = torch.randn(32, H, device=DEV)
    lut = A.relative_bias_lut(table, S, S, True, 32, 128)
    ids = torch.zeros(B, S, dtype=torch.int32, device=DEV)
    flags = torch.zeros(B, S, dtype=torch.uint8, device=DEV)
    flags[0, 3] = 1
    bl = A.block_lists([[[0, 1], [1]]], block=64)
    variants = [dict(bias_lut=lut), dict(q_segments=ids, k_segments=ids), dict(window=5, global_keys=flags),
                dict(block_lists=bl)]
    for kw in variants:
        o = A.attention(x, x, x, scale=0.125, softcap=5.0, **kw)
        assert calls == [], (kw.keys(), calls)
        ref = A._reference(x, x, x, 0.125, False, None, kw.get("bias_lut"), 0.0, 0, window=kw.get("window"),
                           q_seg=kw.get("q_segments"), k_seg=kw.get("k_segments"), gk=kw.get("global_keys"),
                           bl=kw.get("block_lists"), softcap=5.0)
        assert torch.equal(o, ref)
        A.attention(x, x, x, scale=0.125, **kw)  # without the cap: a kernel
        assert len(calls) == 1, (kw.keys(), calls)
        del calls[:]
    for d in (32, 16):
        y = x[..., :d].contiguous()
        o = A.attention(y, y, y, scale=0.125, softcap=5.0)
        assert calls == []
        assert torch.equal(o, A._reference(y, y, y, 0.125, False, None, None, 0.0, 0, softcap=5.0))
    with pytest.raises(ValueError, match="softcap"):
        A.attention(x, x, x, softcap=0.0)
