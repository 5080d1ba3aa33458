"""Routing of attention by head dim (ops/routing.py, ops/attention.py): what the table reports, and that CPU tensors keep
the composite at any head dim."""
import pytest
import torch

from distributed_llms_example_amd.ops import attention as A, routing

_STEP = ("t5-base", 8192, 2048, 768, 3072, "relu", 32128)


def test_plan_reports_attention_kernel_by_head_dim():
    assert routing.plan(*_STEP)["attention"] == "attn.hip"
    assert routing.plan(*_STEP, head_dim=64)["attention"] == "attn.hip"
    for d in (32, 40, 80, 96, 128):
        assert routing.plan(*_STEP, head_dim=d)["attention"] == "attn_hd.hip", d
    for d in (16, 24, 36, 136, 256):
        assert routing.plan(*_STEP, head_dim=d)["attention"] == "composite", d


def test_attn_hd_is_a_route_key(monkeypatch):
    assert routing.DEFAULTS["attn_hd"] == 1
    monkeypatch.setenv("DLLM_ROUTE", "attn_hd=0")
    assert routing.get("attn_hd") == 0
    assert routing.plan(*_STEP, head_dim=128)["attention"] == "composite"
    assert routing.plan(*_STEP, head_dim=64)["attention"] == "attn.hip"
    monkeypatch.setenv("DLLM_ROUTE", "attn_hdx=0")
    with pytest.raises(KeyError):
        routing.get("attn_hd")


def test_cpu_attention_head_dim_128_is_the_composite():
    torch.manual_seed(0)
    q = torch.randn(2, 9, 2, 128)
    k = torch.randn(2, 13, 2, 128)
    v = torch.randn(2, 13, 2, 128)
    mask = torch.ones(2, 13, dtype=torch.bool)
    mask[0, 10:] = False
    assert A._route(q, k, v) is None
    o = A.attention(q, k, v, scale=128 ** -0.5, key_padding_mask=mask, dropout_p=0.1, seed=3)
    ref = A._reference(q, k, v, 128 ** -0.5, False, mask, None, 0.1, 3)
    assert torch.equal(o, ref)
