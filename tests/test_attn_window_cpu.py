"""Sliding-window attention on the CPU: the composite's band mask (the oracle of tests/test_attn_window_gpu.py), the
op's argument checks and the routing table."""
import pytest
import torch

from distributed_llms_example_amd.ops import attention as A, routing

_STEP = ("long-t5-local-base", 16384, 512, 768, 2048, "gated-gelu", 32128)


def _brute(q, k, v, scale, kpm, lut, window):
    """Row by row, key by key: softmax over exactly the visible keys (fp64), 0 for a row without one."""
    B, S, H, D = q.shape
    o = torch.zeros(B, S, H, D, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            for i in range(S):
                js = [j for j in range(S) if abs(j - i) <= window and (kpm is None or bool(kpm[b, j]))]
                if not js:
                    continue
                s = torch.stack([(q[b, i, h].double() * k[b, j, h].double()).sum() * scale +
                                 (lut[h, j - i + S - 1].double() if lut is not None else 0.0) for j in js])
                p = torch.softmax(s, 0)
                o[b, i, h] = (p[:, None] * torch.stack([v[b, j, h].double() for j in js])).sum(0)
    return o


def _case(S=23, D=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(2, S, 3, D, generator=g) for _ in range(3))
    lut = torch.randn(3, 2 * S - 1, generator=g)
    kpm = torch.ones(2, S, dtype=torch.bool)
    kpm[1, 17:] = False
    return q, k, v, lut, kpm


@pytest.mark.parametrize("window", [0, 1, 5, 22, 100])
@pytest.mark.parametrize("bias,pad", [(False, False), (True, True)])
def test_reference_window_is_a_masked_softmax(window, bias, pad):
    q, k, v, lut, kpm = _case()
    lut, kpm = (lut if bias else None), (kpm if pad else None)
    o = A._reference(q, k, v, 0.5, False, kpm, lut, 0.0, 0, window=window)
    ref = _brute(q, k, v, 0.5, kpm, lut, window)
    valid = torch.ones(2, 23, dtype=torch.bool) if kpm is None else kpm  # padded rows can still see valid keys
    torch.testing.assert_close(o.double()[valid], ref[valid], atol=1e-5, rtol=1e-5)
    if window == 0 and kpm is None:  # the diagonal only: every row returns its own value
        torch.testing.assert_close(o, v, atol=1e-6, rtol=1e-6)


def test_reference_without_window_is_unchanged():
    q, k, v, lut, kpm = _case()
    a = A._reference(q, k, v, 0.5, False, kpm, lut, 0.1, 7)
    b = A._reference(q, k, v, 0.5, False, kpm, lut, 0.1, 7, window=None)
    assert torch.equal(a, b)
    # a window no key falls outside of changes nothing either
    c = A._reference(q, k, v, 0.5, False, kpm, lut, 0.1, 7, window=22)
    assert torch.equal(a, c)
    assert not torch.equal(a, A._reference(q, k, v, 0.5, False, kpm, lut, 0.1, 7, window=21))


def test_ops_carry_the_window_on_cpu():
    q, k, v, lut, kpm = _case()
    ref = A._reference(q, k, v, 1.0, False, kpm, lut, 0.1, 3, window=4)
    kw = dict(scale=1.0, key_padding_mask=kpm, bias_lut=lut, dropout_p=0.1, seed=3, window=4)
    assert torch.equal(A.attention(q, k, v, **kw), ref)
    assert torch.equal(A.attention_qkv(torch.stack([q, k, v], 2), **kw), ref)
    assert torch.equal(A.attention_q_kv(q, torch.stack([k, v], 2), **kw), ref)


def test_window_rejects_causal_and_rectangular_calls():
    q, k, v, _, _ = _case()
    with pytest.raises(ValueError, match="causal"):
        A.attention(q, k, v, causal=True, window=3)
    with pytest.raises(ValueError, match="Sq == Sk"):
        A.attention(q[:, :9], k, v, window=3)
    with pytest.raises(ValueError, match="Sq == Sk"):
        A.attention_q_kv(q[:, :9], torch.stack([k, v], 2), window=3)
    with pytest.raises(ValueError, match=">= 0"):
        A.attention(q, k, v, window=-2)


def test_windowed_routes():
    assert routing.attention_route(64, True, window=127) == "attn_hd.hip"
    assert routing.attention_route(64, False, window=127) == "attn_f32.hip"
    for d in (32, 40, 96, 128):
        assert routing.attention_route(d, True, window=5) == "attn_hd.hip", d
    assert routing.attention_route(16, True, window=127) == "composite"
    assert routing.attention_route(16, False, window=127) == "composite"
    assert routing.attention_route(128, False, window=127) == "composite"
    assert routing.attention_route(136, True, window=0) == "composite"


def test_unwindowed_routes_are_unchanged():
    assert routing.attention_route(64) == "attn.hip"
    assert routing.attention_route(64, True) == "attn.hip"
    assert routing.attention_route(64, True, None) == "attn.hip"
    assert routing.attention_route(64, False) == "attn_f32.hip"
    assert routing.attention_route(128, True) == "attn_hd.hip"
    assert routing.attention_route(128, False) == "composite"
    assert routing.attention_route(16, True) == "composite"


def test_route_switches_apply_to_windowed_calls(monkeypatch):
    monkeypatch.setenv("DLLM_ROUTE", "attn_hd=0,attn_f32=0")
    assert routing.attention_route(64, True, window=127) == "composite"
    assert routing.attention_route(64, False, window=127) == "composite"
    assert routing.attention_route(64, True) == "attn.hip"


def test_plan_reports_the_window():
    p = routing.plan(*_STEP, head_dim=64, window=127)
    assert p["attention.window"] == 127
    assert p["enc.self_attention"] == "attn_hd.hip"
    assert p["attention"] == "attn.hip"  # decoder self-attention and cross-attention stay on the tuned kernels
    assert routing.plan(*_STEP, head_dim=16, window=127)["enc.self_attention"] == "composite"
    q = routing.plan(*_STEP, head_dim=64)
    assert "attention.window" not in q and "enc.self_attention" not in q
    assert q == {k: v for k, v in p.items() if k not in ("attention.window", "enc.self_attention")}


def test_cpu_tensors_take_the_composite_with_a_window():
    q, k, v, _, _ = _case(D=64)
    assert A._route(q, k, v, window=5) is None
    assert A._route(q.bfloat16(), window=5) is None
