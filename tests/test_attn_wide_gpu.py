"""csrc/attn_wide.hip through ``attention_grouped``: forward + backward against an fp64 composite on the same bf16
values.  K / V (randn, distinct per K/V head) are repeated per query head INSIDE the oracle only; a spy asserts that the
kernel got the H_kv heads and that nothing but attn_wide_* ran.  Bounds: rel-L2 2e-2 on o, 3e-2 on dq / dk / dv
(tests/test_attn_softcap_gpu.py) and ``attn_refs.row_err`` < ``attn_refs.ROW_CAP`` per row.  Cap cases: scale 1, c = 10
(39 - 53 % of the scores beyond the cap, asserted within 0.2 .. 0.8); uncapped: scale D ** -0.5."""
import pytest
import torch

import attn_refs as R
from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops import attention as A
from distributed_llms_example_amd.ops import routing

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture
def calls(monkeypatch):
    out, real = [], _ext.native()

    class Spy:
        def __getattr__(self, n):
            f = getattr(real, n)
            if not (n.startswith("attn") and n.endswith(("_fwd", "_bwd"))):  # every attention binding
                return f

            def g(*a, **kw):
                out.append((n, a[2 if n.endswith("bwd") else 1].shape[2], kw.get("softcap")))
                return f(*a, **kw)
            return g

    spy = Spy()
    monkeypatch.setattr(A._ext, "native", lambda: spy)
    ref = A._reference
    monkeypatch.setattr(A, "_reference", lambda *a, **kw: (out.append(("composite", a[1].shape[2], None)), ref(*a, **kw))[1])
    return out


def _visible(mask, B, Sq, Sk, causal, window):
    i, j = torch.arange(Sq, device=DEV)[:, None], torch.arange(Sk, device=DEV)[None, :]
    vis = torch.ones(Sq, Sk, dtype=torch.bool, device=DEV)
    if causal:
        vis &= j <= i + (Sk - Sq)
    if window is not None:
        vis &= (j - i).abs() <= window
    vis = vis[None].expand(B, -1, -1)
    return vis & mask[:, None, :] if mask is not None else vis


def _ref64(q, k, v, g, scale, c, vis):
    """fp64 composite, cap before the mask; k / v are repeated HERE, so autograd sums dk / dv over each group."""
    q, k, v = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    G = q.shape[2] // k.shape[2]
    qf, kf, vf = (t.permute(0, 2, 1, 3) for t in (q, k.repeat_interleave(G, 2), v.repeat_interleave(G, 2)))
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    raw = s.detach()
    if c is not None:
        s = c * torch.tanh(s / c)
    s = s.masked_fill(~vis[:, None], torch.finfo(torch.float64).min)
    pr = torch.softmax(s, dim=-1) * vis[:, None].any(-1, keepdim=True)
    o = torch.matmul(pr, vf).permute(0, 2, 1, 3)
    return (o.detach(),) + torch.autograd.grad(o, [q, k, v], g.double()), raw


CASES = [
    # tag, H, Hkv, Sq, Sk, D, pad (None | "suffix" | "row1"), causal, window, c, packed
    ("packed ragged", 4, 2, 200, 200, 256, None, False, None, 10.0, True),
    ("G1 padded", 2, 2, 333, 333, 256, "suffix", False, None, None, False),
    ("G4", 4, 1, 130, 130, 256, None, False, None, 10.0, False),
    ("causal", 4, 2, 200, 200, 256, None, True, None, 10.0, False),
    ("decode 1", 4, 2, 1, 70, 256, None, True, None, 10.0, False),
    ("decode 5", 4, 2, 5, 70, 256, None, True, None, 10.0, False),
    ("cross short query", 4, 2, 9, 333, 256, "suffix", False, None, None, False),
    ("window 63", 4, 2, 333, 333, 256, None, False, 63, 10.0, False),
    ("window 64", 4, 2, 333, 333, 256, None, False, 64, 10.0, False),
    ("window 65", 4, 2, 333, 333, 256, None, False, 65, 10.0, False),
    ("head dim 192", 4, 2, 200, 200, 192, "suffix", False, None, 10.0, False),
    ("head dim 136", 4, 2, 200, 200, 136, "suffix", False, None, 10.0, False),
    ("row without a key", 4, 2, 70, 70, 256, "row1", False, None, None, False),
]


@pytest.mark.parametrize("tag,H,Hkv,Sq,Sk,D,pad,causal,window,c,packed", CASES, ids=[x[0] for x in CASES])
def test_attn_wide_matches_fp64(tag, H, Hkv, Sq, Sk, D, pad, causal, window, c, packed, calls):
    """Measured (MI355X, profiles/attn_wide.txt): rel-L2 <= 2.4e-3 and worst row <= 4.3e-3 on every output of every
    case.  "causal" is the case that tells where delta comes from: its rows 1 .. 7 have a one-hot softmax and a dq
    below the rounding of the stored bf16 output (worst row 2.46 with delta = rowsum(dO o O), 4.3e-3 as it is)."""
    B, scale = 2, (1.0 if c is not None else D ** -0.5)
    torch.manual_seed(Sq * 7 + Sk + D + H)
    x = torch.randn(B, Sk, H + 2 * Hkv, D, device=DEV).to(torch.bfloat16).requires_grad_(True)
    if packed:
        q, k, v = x[:, :, :H], x[:, :, H:H + Hkv], x[:, :, H + Hkv:]
    else:
        q = torch.randn(B, Sq, H, D, device=DEV).to(torch.bfloat16).requires_grad_(True)
        k, v = (x.detach()[:, :, H + i * Hkv:H + (i + 1) * Hkv].clone().requires_grad_(True) for i in (0, 1))
    mask = None
    if pad is not None:
        mask = torch.ones(B, Sk, dtype=torch.bool, device=DEV)
        if pad == "suffix":
            mask[0, Sk - Sk // 5:] = False
        else:
            mask[1] = False
    vis = _visible(mask, B, Sq, Sk, causal, window)
    g = torch.randn(B, Sq, H, D, device=DEV).to(torch.bfloat16)
    o = A.attention_grouped(q, k, v, scale=scale, causal=causal, key_padding_mask=mask, window=window, softcap=c)
    got = (o.detach(),) + torch.autograd.grad(o, [q, k, v], g)
    assert calls == [("attn_wide_fwd", Hkv, c), ("attn_wide_bwd", Hkv, c)], calls
    assert o.dtype == torch.bfloat16 and got[2].shape == (B, Sk, Hkv, D) and got[3].shape == (B, Sk, Hkv, D)
    ref, raw = _ref64(q, k, v, g, scale, c, vis)
    if c is not None:
        sel = vis[:, None].expand_as(raw)
        frac = ((raw.abs() > c) & sel).sum().item() / sel.sum().item()
        assert 0.2 < frac < 0.8, frac
    if pad == "row1":  # batch row 1 has no key: exactly 0 everywhere, LSE +inf; batch row 0 is held to the bounds
        assert all(not t[1].float().any() for t in got)
        _, lse = _ext.native().attn_wide_fwd(q.detach(), k.detach(), v.detach(), mask.to(torch.uint8), None, scale,
                                             False, 0.0, 0)
        assert torch.isposinf(lse[1]).all() and torch.isfinite(lse[0]).all()
        got, ref = [t[:1] for t in got], [t[:1] for t in ref]
    else:
        assert vis.any(-1).all()
    errs = {n: (R.rel_l2(a, b), R.row_err(a, b)) for n, a, b in zip(("o", "dq", "dk", "dv"), got, ref)}
    print(f"[attn_wide {tag}] " + " ".join(f"{n}: l2 {e[0]:.2e} row {e[1]:.2e}" for n, e in errs.items()))
    for n, (l2, row) in errs.items():
        assert l2 < (2e-2 if n == "o" else 3e-2) and row < R.ROW_CAP, (tag, n, l2, row)


def test_binding_refuses_by_name():
    C = _ext.native()
    B, S, H, Hkv, D = 1, 128, 4, 2, 256
    q, k = (torch.randn(B, S, n, D, device=DEV).to(torch.bfloat16) for n in (H, Hkv))
    o, lse = C.attn_wide_fwd(q, k, k, None, None, 0.06, False, 0.0, 0)
    sg = A.segments(torch.zeros(B, S, dtype=torch.int32, device=DEV))
    gk = A.global_keys(torch.zeros(B, S, dtype=torch.uint8, device=DEV))
    refused = {
        "bias LUT": dict(lut=torch.zeros(H, 2 * S - 1, device=DEV)),
        "segments": dict(kw=dict(q_seg=sg.ids, k_seg=sg.ids, q_blk=sg.blk, k_blk=sg.blk)),
        "global keys": dict(kw=dict(window=5, k_glob=gk.flags, k_gblk=gk.blk)),
        "block lists": dict(kw=A.block_lists([[[0, 1], [0, 1]]], block=64).tables(q.device, S, S)),
        "dropout": dict(p=0.1),
        "window with causal": dict(causal=True, kw=dict(window=5)),
        "no multiple of the 3 K/V heads": dict(k=k[:, :, :1].repeat(1, 1, 3, 1)),
        "head dim must be in 136 .. 256.*128": dict(q=q[..., :128].contiguous(), k=k[..., :128].contiguous()),
        "head dim must be in 136 .. 256.*264": dict(q=q.repeat(1, 1, 1, 2)[..., :264].contiguous(),
                                                     k=k.repeat(1, 1, 1, 2)[..., :264].contiguous()),
        "head dim must be in 136 .. 256.*140": dict(q=q[..., :140].contiguous(), k=k[..., :140].contiguous()),
    }
    for what, e in refused.items():
        qq, kk = e.get("q", q), e.get("k", k)
        args = (kk, kk, None, e.get("lut"), 0.06, e.get("causal", False), e.get("p", 0.0), 0)
        with pytest.raises(RuntimeError, match=what):
            C.attn_wide_fwd(qq, *args, **e.get("kw", {}))
        if qq is q:
            with pytest.raises(RuntimeError, match=what):
                C.attn_wide_bwd(o, q, kk, kk, o, lse, *args[2:], False, **e.get("kw", {}))
    torch.cuda.synchronize()


def test_route_off_is_the_fallback(calls, monkeypatch):
    B, S, H, Hkv, D = 2, 70, 4, 2, 256
    q = torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16)
    k, v = (torch.randn(B, S, Hkv, D, device=DEV).to(torch.bfloat16) for _ in range(2))
    kw = dict(scale=1.0, causal=True, softcap=10.0)
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(attn_wide=0))
    o = A.attention_grouped(q, k, v, **kw)
    assert [c[0] for c in calls] == ["composite"], calls
    assert torch.equal(o, A.attention(q, k.repeat_interleave(2, 2), v.repeat_interleave(2, 2), **kw))
