"""csrc/attn_decode.hip through ``attention_decode`` and its binding: the forward against an fp64 composite on the same
bf16 values (K / V repeated per query head INSIDE the oracle only).  Bounds: the project's own for a bf16 forward,
``attn_refs.rel_l2`` < 2e-2 and ``attn_refs.row_err`` < ``attn_refs.ROW_CAP``.  Uncapped cases: scale D ** -0.5; capped:
scale 1, c = 10 (0.2 .. 0.8 of the visible scores beyond the cap, asserted).  Each case is the smallest shape at which
its part of the kernel can go wrong."""
import pytest
import torch

import attn_refs as R
from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops import attention as A

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ref64(q, k, v, scale, c, mask, lut):
    """fp64 composite: cap, then bias lut[h][(j - i) + Sq - 1], then the mask; a row without a visible key is 0."""
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
    ("first step", 4, 4, 1, 1, 64, 1, None),              # three waves without a key
    ("ragged tail", 4, 4, 1, 70, 64, 1, None),            # keys not a multiple of 32 or 128
    ("forced splits", 4, 4, 1, 300, 64, 3, None),         # short last split
    ("cache view", 4, 4, 1, 300, 64, 3, "view"),          # batch stride != Sk stride
    ("beam-shared cross", 4, 4, 4, 333, 64, 2, "suffix"),  # row packing, kpm
    ("split without a visible key", 4, 4, 2, 300, 64, 3, "from128"),
    ("batch row without any key", 4, 4, 2, 70, 64, 1, "row1"),
    ("grouped G2 16 rows", 8, 4, 8, 70, 128, 1, None),    # R = 16, full tile
    ("grouped G4 Sq3", 4, 1, 3, 70, 128, 1, None),        # R = 12, row order i G + g
    ("T5 bias Sq1", 4, 4, 1, 200, 64, 2, "lut"),
    ("T5 bias Sq3", 4, 4, 3, 200, 64, 2, "lut"),
    ("soft cap", 4, 2, 1, 200, 256, 2, "cap"),            # cap before the mask
] + [(f"head dim {D}", 4, 2, 2, 70, D, 1, None) for D in (40, 80, 136, 192, 256)]  # padding inside an instantiation


@pytest.mark.parametrize("tag,H,Hkv,Sq,Sk,D,splits,extra", CASES, ids=[x[0] for x in CASES])
def test_attn_decode_matches_fp64(tag, H, Hkv, Sq, Sk, D, splits, extra):
    """Measured (MI355X, profiles/attn_decode.txt): rel-L2 <= 2.2e-3 and worst row <= 2.9e-3 on every case."""
    B, c = 2, (10.0 if extra == "cap" else None)
    scale = 1.0 if c is not None else D ** -0.5
    torch.manual_seed(Sq * 7 + Sk + D + H)
    q = torch.randn(B, Sq, H, D, device=DEV).to(torch.bfloat16)
    kbuf, vbuf = (torch.randn(B, 512 if extra == "view" else Sk, Hkv, D, device=DEV).to(torch.bfloat16) for _ in (0, 1))
    k, v = kbuf[:, :Sk], vbuf[:, :Sk]
    mask = None
    if extra in ("suffix", "from128", "row1"):
        mask = torch.ones(B, Sk, dtype=torch.bool, device=DEV)
        if extra == "suffix":
            mask[0, Sk - Sk // 5:] = False
        elif extra == "from128":
            mask[:, 128:] = False
        else:
            mask[1] = False
    lut = torch.randn(H, Sq + Sk - 1, device=DEV) if extra == "lut" else None
    kpm = mask.to(torch.uint8) if mask is not None else None
    C = _ext.native()
    got = C.attn_decode(q, k, v, kpm, lut, scale, c or 0.0, splits)
    assert got.dtype == torch.bfloat16 and got.shape == q.shape
    if splits > 1:  # the merge has a fixed order: the same bits on a second run
        assert torch.equal(got, C.attn_decode(q, k, v, kpm, lut, scale, c or 0.0, splits))
    ref, raw, vis = _ref64(q, k, v, scale, c, mask, lut)
    if c is not None:
        frac = ((raw.abs() > c) & vis).sum().item() / vis.sum().item()
        assert 0.2 < frac < 0.8, frac
    runs = {"binding": got, "op": A.attention_decode(q, k, v, scale=scale, key_padding_mask=mask, bias_lut=lut, softcap=c)}
    if tag == "forced splits":
        runs["auto"] = C.attn_decode(q, k, v, kpm, lut, scale, 0.0, 0)
    for name, o in runs.items():
        if extra == "row1":  # batch row 1 has no key: exactly 0; batch row 0 is held to the bounds
            assert not o[1].float().any()
            o, want = o[:1], ref[:1]
        else:
            want = ref
        l2, row = R.rel_l2(o, want), R.row_err(o, want)
        print(f"[attn_decode {tag} / {name}] l2 {l2:.2e} row {row:.2e}")
        assert l2 < 2e-2 and row < R.ROW_CAP, (tag, name, l2, row)


def test_binding_refuses_by_name():
    C = _ext.native()

    def t(S, n, D):
        return torch.randn(1, S, n, D, device=DEV).to(torch.bfloat16)

    refused = {
        "R = Sq \\* \\(H / Hkv\\) = 17": (t(17, 4, 64), t(70, 4, 64), {}),
        "causal with Sq > 1": (t(2, 4, 64), t(70, 4, 64), dict(causal=True)),
        "soft cap with a bias LUT": (t(1, 4, 64), t(70, 4, 64), dict(softcap=10.0, lut=torch.zeros(4, 70, device=DEV))),
        "head dim must be in 32 .. 256.*264": (t(1, 4, 264), t(70, 4, 264), {}),
        "head dim must be in 32 .. 256.*36": (t(1, 4, 36), t(70, 4, 36), {}),
        "no multiple of the 3 K/V heads": (t(1, 4, 64), t(70, 3, 64), {}),
    }
    for what, (q, k, e) in refused.items():
        with pytest.raises(RuntimeError, match=what):
            C.attn_decode(q, k, k, None, e.get("lut"), 0.125, e.get("softcap", 0.0), 0, e.get("causal", False))
    torch.cuda.synchronize()
