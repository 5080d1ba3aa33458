"""``attention_grouped`` off the GPU is ``attention`` on repeated K / V, bit for bit; ``attention_grouped_route``."""
import pytest
import torch

from distributed_llms_example_amd.ops import attention as A
from distributed_llms_example_amd.ops import routing


@pytest.mark.parametrize("H,Hkv", [(4, 2), (4, 4)])
def test_cpu_is_attention_on_repeated_kv(H, Hkv):
    torch.manual_seed(H + Hkv)
    B, Sq, Sk, D, G = 2, 7, 11, 16, H // Hkv
    q = torch.randn(B, Sq, H, D, requires_grad=True)
    k, v = (torch.randn(B, Sk, Hkv, D, requires_grad=True) for _ in range(2))
    mask = torch.ones(B, Sk, dtype=torch.bool)
    mask[0, 8:] = False
    kw = dict(scale=0.25, causal=True, key_padding_mask=mask, softcap=3.0)
    g = torch.randn(B, Sq, H, D)
    o = A.attention_grouped(q, k, v, **kw)
    dq, dk, dv = torch.autograd.grad(o, [q, k, v], g)
    kr, vr = (t.detach().repeat_interleave(G, 2).requires_grad_(True) for t in (k, v))
    o2 = A.attention(q, kr, vr, **kw)
    dq2, dk2, dv2 = torch.autograd.grad(o2, [q, kr, vr], g)
    assert torch.equal(o, o2) and torch.equal(dq, dq2)
    assert dk.shape == k.shape and dv.shape == v.shape
    assert torch.equal(dk, dk2.view(B, Sk, Hkv, G, D).sum(3)) and torch.equal(dv, dv2.view(B, Sk, Hkv, G, D).sum(3))


def test_grouped_route(monkeypatch):
    r = routing.attention_grouped_route
    assert r(256) == r(192, True, 64) == r(136, True, softcap=True) == "attn_wide.hip"
    for args, kw in (((128,), {}), ((264,), {}), ((140,), {}), ((256, False), {}), ((256,), dict(dropout=True))):
        assert r(*args, **kw) == "fallback", (args, kw)
    assert routing.attention_route(256, True, softcap=True) == "composite"  # attention() itself is unchanged
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(attn_wide=0))
    assert r(256) == "fallback"
