"""``attention_decode`` off the GPU: it is ``attention`` (on repeated K / V for grouped heads), forward only, behind the
route key ``attn_decode``; and cached generation through it gives the tokens of the route switched off."""
import pytest
import torch

from distributed_llms_example_amd.models import PRESETS, build_model
from distributed_llms_example_amd.ops import attention as A
from distributed_llms_example_amd.ops import routing


@pytest.mark.parametrize("H,Hkv,Sq,lut,cap", [(4, 4, 1, True, None), (4, 2, 3, False, 10.0), (4, 1, 2, True, None)])
def test_cpu_is_attention_on_repeated_kv(H, Hkv, Sq, lut, cap):
    torch.manual_seed(0)
    B, Sk, D = 2, 37, 16
    q, k, v = torch.randn(B, Sq, H, D), torch.randn(B, Sk, Hkv, D), torch.randn(B, Sk, Hkv, D)
    mask = torch.ones(B, Sk, dtype=torch.bool)
    mask[1, 30:] = False
    kw = dict(scale=0.25, key_padding_mask=mask, bias_lut=torch.randn(H, Sq + Sk - 1) if lut else None, softcap=cap)
    assert not A.decode_served(q, k)
    want = A.attention(q, k.repeat_interleave(H // Hkv, 2), v.repeat_interleave(H // Hkv, 2), **kw)
    assert torch.equal(A.attention_decode(q, k, v, **kw), want)


def test_forward_only_and_route_key(monkeypatch):
    q, k = torch.randn(1, 1, 2, 16, requires_grad=True), torch.randn(1, 5, 2, 16)
    with pytest.raises(RuntimeError, match="forward only"):
        A.attention_decode(q, k, k)
    with torch.no_grad():
        A.attention_decode(q, k, k)
    assert routing.get("attn_decode") == 1
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(attn_decode=0))
    assert routing.get("attn_decode") == 0


@pytest.mark.parametrize("preset", ["t5-tiny", "bart-tiny", "t5gemma-tiny-gqa"])
@pytest.mark.parametrize("beams", [1, 2])
def test_generate_gives_the_tokens_of_the_route_off(preset, beams, monkeypatch):
    cfg = PRESETS[preset]
    torch.manual_seed(0)
    m = build_model(cfg).eval()
    ids = torch.randint(3, cfg.vocab_size, (3, 23), generator=torch.Generator().manual_seed(1))
    am = torch.ones_like(ids)
    am[2, 15:] = 0
    ids[2, 15:] = cfg.pad_token_id
    kw = dict(attention_mask=am, max_length=8, num_beams=beams)
    got = m.generate(ids, **kw)
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(attn_decode=0))
    assert torch.equal(got, m.generate(ids, **kw))
