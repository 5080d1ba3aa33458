"""FP8 (e4m3fn) K/V on csrc/attn_decode.hip: the quantise kernel bit for bit against the torch composite of the number
format, and the FP8 instantiation of the decode kernel, through the binding and ``attention_decode``, against the fp64
attention over the dequantised values (K / V quantised by the composite, so the second test does not rest on the first).
Bounds of the kernel test: the project's own for this kernel, ``attn_refs.rel_l2`` < 2e-2 and ``attn_refs.row_err`` <
``attn_refs.ROW_CAP`` — dequantising is exact and the one new rounding (P * v_scale to bf16) is the size of the one
already there.  Each case is the smallest shape at which its part of the kernel can go wrong."""
import pytest
import torch

import attn_refs as R
from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops import attention as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn


@pytest.mark.parametrize("D", [32, 64, 144, 256])
def test_quantiser_is_the_composite_bit_for_bit(D):
    """Error bound: half an ulp of a 3-bit mantissa (2^-4 |x|) or half the subnormal spacing (2^-10 scale)."""
    torch.manual_seed(D)
    buf = torch.randn(2, 70, 2, 3, D + 24, device=DEV) * 2 ** torch.empty(2, 70, 2, 3, 1, device=DEV).uniform_(-3, 3)
    buf[1, 5, 0, 2] = 0
    buf[0, 9, 1, 1, 3] = 1e-4
    kv = buf.to(torch.bfloat16)[..., :D]  # rows one row stride apart, not dense
    codes, scales = _ext.native().kv_quant_fp8(kv)
    want = A._quantize_kv_ref(kv.cpu())  # on the CPU: an IEEE division whatever the device library does
    assert codes.dtype == F8 and codes.shape == kv.shape and scales.dtype == torch.float32
    assert torch.equal(scales.cpu(), want.scales) and scales[1, 5, 0, 2] == 1
    assert torch.equal(codes.cpu().view(torch.uint8), want.codes.view(torch.uint8))
    op = A.quantize_kv(kv)
    assert torch.equal(op.codes.view(torch.uint8), codes.view(torch.uint8)) and torch.equal(op.scales, scales)
    x = kv.double()
    err = (op.dequantize(torch.float64) - x).abs()
    bound = torch.maximum(2.0 ** -4 * x.abs(), 2.0 ** -10 * scales.double().unsqueeze(-1)) * (1 + 1e-5)
    assert bool((err <= bound).all()), float((err - bound).max())


def _ref64(q, k, v, scale, c, mask, lut):
    """tests/test_attn_decode_gpu.py's composite: cap, then bias lut[h][(j - i) + Sq - 1], then the mask."""
    B, Sq, H, _ = q.shape
    Sk, G = k.shape[1], H // k.shape[2]
    qf, kf, vf = (t.double().permute(0, 2, 1, 3) for t in (q, k.repeat_interleave(G, 2), v.repeat_interleave(G, 2)))
    s = raw = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if c is not None:
        s = c * torch.tanh(s / c)
    if lut is not None:
        i, j = torch.arange(Sq, device=DEV)[:, None], torch.arange(Sk, device=DEV)[None, :]
        s = s + lut.double()[:, j - i + Sq - 1][None]
    vis = (mask if mask is not None else torch.ones(B, Sk, dtype=torch.bool, device=DEV))[:, None, None, :]
    s = s.masked_fill(~vis, torch.finfo(torch.float64).min)
    pr = torch.softmax(s, dim=-1) * vis.any(-1, keepdim=True)
    return torch.matmul(pr, vf).permute(0, 2, 1, 3), raw, vis.expand_as(raw)


CASES = [
    # tag, H, Hkv, Sq, Sk, D, splits, extra
    ("first step", 4, 4, 1, 1, 64, 1, None),
    ("ragged tail", 4, 4, 1, 70, 64, 1, None),
    ("forced splits, cache view", 4, 4, 1, 300, 64, 3, "view"),  # batch stride != Sk stride, codes and scales
    ("beam-shared, kpm suffix", 4, 4, 4, 333, 64, 2, "suffix"),
    ("batch row without a key", 4, 4, 2, 70, 64, 1, "row1"),
    ("grouped, 16 rows", 8, 4, 8, 70, 128, 1, None),
    ("T5 bias LUT", 4, 4, 3, 200, 64, 2, "lut"),
    ("soft cap", 4, 2, 1, 200, 256, 2, "cap"),
] + [(f"head dim {D}", 4, 2, 2, 70, D, 1, None) for D in (48, 80, 144)]  # padding inside an instantiation


@pytest.mark.parametrize("tag,H,Hkv,Sq,Sk,D,splits,extra", CASES, ids=[x[0] for x in CASES])
def test_fp8_decode_matches_fp64(tag, H, Hkv, Sq, Sk, D, splits, extra):
    """K rows scaled per (key, head) by 2 ** U(-1, 1) and V rows by 2 ** U(-3, 3): a swapped, mis-indexed or dropped
    scale cannot pass.  Measured (MI355X, profiles/attn_decode_fp8.txt): see the profile's "accuracy" lines."""
    B, c = 2, (10.0 if extra == "cap" else None)
    scale = 1.0 if c is not None else D ** -0.5
    torch.manual_seed(Sq * 7 + Sk + D + H)
    Sb = 512 if extra == "view" else Sk
    q = torch.randn(B, Sq, H, D, device=DEV).to(torch.bfloat16)
    kq, vq = (A._quantize_kv_ref((torch.randn(B, Sb, Hkv, D, device=DEV)
                                  * 2 ** torch.empty(B, Sb, Hkv, 1, device=DEV).uniform_(-e, e)).to(torch.bfloat16))
              for e in (1, 3))
    k, v, ks, vs = kq.codes[:, :Sk], vq.codes[:, :Sk], kq.scales[:, :Sk], vq.scales[:, :Sk]
    mask = None
    if extra in ("suffix", "row1"):
        mask = torch.ones(B, Sk, dtype=torch.bool, device=DEV)
        if extra == "suffix":
            mask[0, Sk - Sk // 5:] = False
        else:
            mask[1] = False
    lut = torch.randn(H, Sq + Sk - 1, device=DEV) if extra == "lut" else None
    kpm = mask.to(torch.uint8) if mask is not None else None
    C = _ext.native()
    got = C.attn_decode(q, k, v, kpm, lut, scale, c or 0.0, splits, False, ks, vs)
    assert got.dtype == torch.bfloat16 and got.shape == q.shape
    if splits > 1:  # the merge has a fixed order: the same bits on a second run
        assert torch.equal(got, C.attn_decode(q, k, v, kpm, lut, scale, c or 0.0, splits, False, ks, vs))
    ref, raw, vis = _ref64(q, k.double() * ks.double().unsqueeze(-1), v.double() * vs.double().unsqueeze(-1), scale, c,
                           mask, lut)
    if c is not None:
        frac = ((raw.abs() > c) & vis).sum().item() / vis.sum().item()
        assert 0.2 < frac < 0.8, frac
    assert A.decode_served(q, k, bias_lut=lut, softcap=c)
    op = A.attention_decode(q, k, v, scale=scale, key_padding_mask=mask, bias_lut=lut, softcap=c, k_scale=ks, v_scale=vs)
    for name, o in (("binding", got), ("op", op)):
        if extra == "row1":  # batch row 1 has no key: exactly 0; batch row 0 is held to the bounds
            assert not o[1].float().any()
            o, want = o[:1], ref[:1]
        else:
            want = ref
        l2, row = R.rel_l2(o, want), R.row_err(o, want)
        print(f"[attn_decode fp8 {tag} / {name}] l2 {l2:.2e} row {row:.2e}")
        assert l2 < 2e-2 and row < R.ROW_CAP, (tag, name, l2, row)


def test_binding_refuses_by_name():
    C = _ext.native()
    q = torch.randn(1, 1, 4, 64, device=DEV).to(torch.bfloat16)
    kv = A._quantize_kv_ref(torch.randn(1, 70, 4, 64, device=DEV))
    q40 = torch.randn(1, 1, 4, 40, device=DEV).to(torch.bfloat16)
    kv40 = A._quantize_kv_ref(torch.randn(1, 70, 4, 40, device=DEV))
    refused = {
        "need k_scale and v_scale": (q, kv.codes, kv.codes, None, None),
        "multiple of 16, got 40": (q40, kv40.codes, kv40.codes, kv40.scales, kv40.scales),
        "k_scale: expected \\[B, Sk, Hkv\\]": (q, kv.codes, kv.codes, kv.scales[:, :69], kv.scales),
        "v_scale: scales are fp32": (q, kv.codes, kv.codes, kv.scales, kv.scales.half()),
        "k and v must have one dtype": (q, kv.codes, kv.dequantize(torch.bfloat16), kv.scales, kv.scales),
        "come with float8_e4m3fn k / v only": (q, kv.dequantize(torch.bfloat16), kv.dequantize(torch.bfloat16),
                                               kv.scales, kv.scales),
    }
    for what, (qq, k, v, ks, vs) in refused.items():
        with pytest.raises(RuntimeError, match=what):
            C.attn_decode(qq, k, v, None, None, 0.125, 0.0, 0, False, ks, vs)
    with pytest.raises(RuntimeError, match="multiple of 16, got 40"):
        C.kv_quant_fp8(q40)
    torch.cuda.synchronize()
