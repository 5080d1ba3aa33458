"""FP8 K/V off the GPU: the number format of ``quantize_kv`` (the torch composite), ``attention_decode`` on a QuantKV
(dequantised in fp32, then today's fallback) and ``generate(cross_kv_dtype=)``."""
import pytest
import torch

from distributed_llms_example_amd.models import PRESETS, build_model
from distributed_llms_example_amd.ops import attention as A


def test_quantize_kv_composite_properties():
    torch.manual_seed(0)
    x = (torch.randn(2, 70, 2, 3, 64) * 2 ** torch.empty(2, 70, 2, 3, 1).uniform_(-3, 3)).to(torch.bfloat16)
    x[1, 5, 0, 2] = 0
    x[0, 9, 1, 1, 3] = 1e-4
    q = A.quantize_kv(x)
    assert isinstance(q, A.QuantKV) and q.codes.dtype == torch.float8_e4m3fn and q.codes.shape == x.shape
    assert q.scales.dtype == torch.float32 and q.scales.shape == x.shape[:-1]
    assert q.scales[1, 5, 0, 2] == 1 and not q.codes[1, 5, 0, 2].float().any()
    am = x.float().abs().amax(-1)
    assert torch.equal(q.scales, torch.where(am == 0, torch.ones_like(am), am / torch.full_like(am, 448.0)))
    assert torch.equal(q.codes.float().to(torch.bfloat16).float(), q.codes.float())  # a code is exact in bf16
    xd = x.double()
    err = (q.dequantize(torch.float64) - xd).abs()
    bound = torch.maximum(2.0 ** -4 * xd.abs(), 2.0 ** -10 * q.scales.double().unsqueeze(-1)) * (1 + 1e-5)
    assert bool((err <= bound).all())
    assert float((err.amax(-1) / xd.abs().amax(-1).clamp_min(1e-30)).max()) <= 1 / 28 * (1 + 1e-5)


@pytest.mark.parametrize("H,Hkv,Sq", [(4, 4, 1), (4, 2, 3)])
def test_cpu_attention_decode_on_quantkv_is_attention_on_the_dequantised(H, Hkv, Sq):
    torch.manual_seed(1)
    B, Sk, D = 2, 37, 32
    q = torch.randn(B, Sq, H, D)
    kq, vq = (A.quantize_kv(torch.randn(B, Sk, Hkv, D) * 2 ** torch.empty(B, Sk, Hkv, 1).uniform_(-e, e)) for e in (1, 3))
    mask = torch.ones(B, Sk, dtype=torch.bool)
    mask[1, 30:] = False
    got = A.attention_decode(q, kq.codes, vq.codes, scale=D ** -0.5, key_padding_mask=mask, k_scale=kq.scales,
                             v_scale=vq.scales)
    G = H // Hkv
    k, v = (t.dequantize(torch.float64).repeat_interleave(G, 2).permute(0, 2, 1, 3) for t in (kq, vq))
    s = torch.matmul(q.double().permute(0, 2, 1, 3), k.transpose(-1, -2)) * D ** -0.5
    want = torch.matmul(torch.softmax(s.masked_fill(~mask[:, None, None, :], float("-inf")), -1), v).permute(0, 2, 1, 3)
    assert float((got.double() - want).norm() / want.norm()) < 1e-5  # fp32 arithmetic on exact inputs
    with pytest.raises(ValueError, match="come with k_scale and v_scale"):
        A.attention_decode(q, kq.codes, vq.codes)


@pytest.mark.parametrize("preset", ["t5-tiny", "bart-tiny", "t5gemma-tiny-gqa"])
def test_generate_with_fp8_cross_kv(preset):
    cfg = PRESETS[preset]
    torch.manual_seed(0)
    m = build_model(cfg).eval()
    ids = torch.randint(3, cfg.vocab_size, (3, 23), generator=torch.Generator().manual_seed(1))
    am = torch.ones_like(ids)
    am[2, 15:] = 0
    out = m.generate(ids, attention_mask=am, max_length=8, num_beams=2, cross_kv_dtype="fp8")
    assert out.shape[0] == 3 and 1 < out.shape[1] <= 8
    with pytest.raises(ValueError, match="cross_kv_dtype"):
        m.generate(ids, attention_mask=am, max_length=8, cross_kv_dtype="int3")
