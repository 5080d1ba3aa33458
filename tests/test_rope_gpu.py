"""The rotary position embedding kernel (csrc/rope.hip ``rope_fwd``) on the GPU against fp64: packed qkv and lone
views, positions as ``[S]`` and as ``[B, S]`` with an offset, bf16 and fp32, forward and backward.

Bounds.  bf16: every element within one bf16 ulp of the fp64 result rounded to bf16 — the kernel's fp32 products and sum
are exact to far below half a bf16 ulp, so they can move the final rounding only at a tie.  fp32: per rotated pair
(x1', x2') an error of at most 2^-21 of the pair's norm — three roundings of 2^-24 each (two products, one sum; the
rotation keeps the norm), with a margin of 2 and the table's own fp32 rounding of cos / sin inside it.

The backward (sign -1) is held to the same bounds against fp64 of the inverse rotation of what it is given (the
forward's stored output), and backward(forward(x)) is x up to the two stores in between: per pair 2 x 2^-8 of its norm
in bf16 (each store moves an element by at most 2^-9 of its magnitude, hence the pair by at most 2^-9 of its norm; a
margin of 2), 2 x 2^-21 in fp32."""
import pytest
import torch

from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops import rope as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, S, H = 2, 333, 3
THETA, MAXPOS = 10000.0, 512


def _ref64(x, pos, cos, sin, sign=1.0):
    """fp64 of ``x [B, S, n, H, D]`` (as stored) with the fp32 table."""
    half = x.shape[-1] // 2
    p = pos.long()
    if p.dim() == 1:
        p = p[None].expand(x.shape[0], -1)
    c = cos.double()[p][:, :, None, None, :]
    s = sin.double()[p][:, :, None, None, :] * sign
    x1, x2 = x.double()[..., :half], x.double()[..., half:]
    return torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), -1)


def _bf16_ulps(got, ref64):
    """Distance in bf16 ulps (as ordered integers) between ``got`` and ``ref64`` rounded to bf16."""
    def order(t):
        i = t.view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (order(got) - order(ref64.to(torch.bfloat16))).abs().max().item()


def _pair_err(got, ref64):
    """max over pairs of |(x1', x2') - ref| / |ref pair|."""
    half = got.shape[-1] // 2
    d = got.double() - ref64
    num = (d[..., :half] ** 2 + d[..., half:] ** 2).sqrt()
    den = (ref64[..., :half] ** 2 + ref64[..., half:] ** 2).sqrt()
    return (num / den.clamp_min(1e-300)).max().item()


def _positions(kind):
    if kind == "S":
        return torch.arange(S, device=DEV, dtype=torch.int32)
    return (torch.arange(S, device=DEV, dtype=torch.int32)[None] + torch.tensor([[0], [70]], device=DEV,
                                                                                 dtype=torch.int32)).contiguous()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("kind", ["S", "BS+70"])
def test_rope_kernel(D, dtype, kind):
    C = _ext.native()
    torch.manual_seed(D)
    cos, sin = R.rope_table(THETA, D, MAXPOS, DEV)
    assert cos.shape == (MAXPOS, D // 2) and cos.dtype == torch.float32
    pos = _positions(kind)
    qkv = torch.randn(B, S, 3, H, D, device=DEV).to(dtype)
    # packed: q and k rotated in place, v untouched bit for bit
    x = qkv.clone()
    out = C.rope_fwd(x[:, :, :2], pos, cos, sin)
    assert out.data_ptr() == x.data_ptr()
    ref = _ref64(qkv[:, :, :2], pos, cos, sin)
    assert torch.equal(x[:, :, 2], qkv[:, :, 2])
    if dtype == torch.bfloat16:
        ulps = _bf16_ulps(x[:, :, :2], ref)
        print(f"[rope bf16 D={D} {kind}] worst distance {ulps} bf16 ulp")
        assert ulps <= 1
    else:
        err = _pair_err(x[:, :, :2], ref)
        print(f"[rope fp32 D={D} {kind}] worst pair error {err:.3e} (bound {2.0 ** -21:.3e})")
        assert err <= 2.0 ** -21
    # a lone view: k of the packed tensor, as [B, S, 1, H, D]; q and v untouched
    y = qkv.clone()
    C.rope_fwd(y[:, :, 1:2], pos, cos, sin)
    assert torch.equal(y[:, :, 1], x[:, :, 1]) and torch.equal(y[:, :, 0], qkv[:, :, 0])
    assert torch.equal(y[:, :, 2], qkv[:, :, 2])
    # backward of forward is the identity (the rotation is orthogonal), to the same bounds
    back = _ref64(x[:, :, :2], pos, cos, sin, -1.0)  # fp64 inverse rotation of the stored forward output
    C.rope_fwd(x[:, :, :2], pos, cos, sin, -1.0)
    if dtype == torch.bfloat16:
        assert _bf16_ulps(x[:, :, :2], back) <= 1
        assert _pair_err(x[:, :, :2], qkv[:, :, :2].double()) <= 2 * 2.0 ** -8
    else:
        assert _pair_err(x[:, :, :2], back) <= 2.0 ** -21
        assert _pair_err(x[:, :, :2], qkv[:, :, :2].double()) <= 2 * 2.0 ** -21


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_rope_op_and_gradient(dtype):
    """The autograd op: its input is left as it is, the output is the kernel's, and the gradient is the inverse
    rotation of the output gradient (v's passes through)."""
    D = 64
    torch.manual_seed(1)
    cos, sin = R.rope_table(THETA, D, MAXPOS, DEV)
    pos = _positions("BS+70")
    qkv = torch.randn(B, S, 3, H, D, device=DEV).to(dtype)
    x = qkv.clone().requires_grad_(True)
    out = R.rope(x, pos, cos, sin, slots=2)
    assert torch.equal(x.detach(), qkv)
    y = qkv.clone()
    _ext.native().rope_fwd(y[:, :, :2], pos, cos, sin)
    assert torch.equal(out.detach(), y)
    g = torch.randn(B, S, 3, H, D, device=DEV).to(dtype)
    out.backward(g)
    gref = _ref64(g[:, :, :2], pos, cos, sin, -1.0)
    assert torch.equal(x.grad[:, :, 2], g[:, :, 2])
    if dtype == torch.bfloat16:
        assert _bf16_ulps(x.grad[:, :, :2], gref) <= 1
    else:
        assert _pair_err(x.grad[:, :, :2], gref) <= 2.0 ** -21
    # the torch reference (the CPU path) computes the same thing: per pair within one store's rounding (bf16: 2^-9 of
    # the pair's norm, margin 2) or the fp32 bound
    ref = R._reference(qkv[:, :, :2], pos, cos, sin)
    assert _pair_err(ref, _ref64(qkv[:, :, :2], pos, cos, sin)) <= (2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -21)


def test_rope_binding_checks():
    C = _ext.native()
    cos, sin = R.rope_table(THETA, 64, MAXPOS, DEV)
    x = torch.randn(1, 8, 2, 2, 64, device=DEV, dtype=torch.bfloat16)
    pos = torch.arange(8, device=DEV, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="pos"):
        C.rope_fwd(x, pos[:7], cos, sin)
    with pytest.raises(RuntimeError, match="pos"):
        C.rope_fwd(x, pos.long(), cos, sin)
    with pytest.raises(RuntimeError, match="cos / sin"):
        C.rope_fwd(x, pos, cos[:, :16], sin[:, :16])
    with pytest.raises(RuntimeError, match="head dim"):
        C.rope_fwd(x[..., :24], pos, cos[:, :12].contiguous(), sin[:, :12].contiguous())
    with pytest.raises(RuntimeError, match="B, S, n, H, D"):
        C.rope_fwd(x[0], pos, cos, sin)
    # a position past the table is clamped to it, never read out of bounds
    y = x.clone()
    C.rope_fwd(y, torch.full((8,), MAXPOS + 5, device=DEV, dtype=torch.int32), cos, sin)
    z = x.clone()
    C.rope_fwd(z, torch.full((8,), MAXPOS - 1, device=DEV, dtype=torch.int32), cos, sin)
    assert torch.equal(y, z)
    torch.cuda.synchronize()
