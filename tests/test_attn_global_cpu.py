"""Global keys in the composite attention (ops/attention.py ``_reference(..., window, gk)``, the O(S²) oracle and the
CPU path): with a window, a key flagged global is visible to every query, inside its band or not, and counts once
where it lies inside.  Checked against a dense formula written here, forward and autograd gradients, with the padding
mask, the bias LUT and dropout; the argument errors; and the two degenerate masks (none global: the window-only
result exactly; all global: full attention)."""
import pytest
import torch

from distributed_llms_example_amd.ops import attention as A
from distributed_llms_example_amd.ops.rng import attention_keep_mask


def _dense(q, k, v, scale, valid, glob, w, lut, p, seed):
    """softmax over {j : valid[b, j] and (|j - i| <= w or glob[b, j])}, row by row semantics in one dense tensor
    (fp64).  q / k / v: [B, S, H, D]."""
    B, S, H, D = q.shape
    i = torch.arange(S)[:, None]
    j = torch.arange(S)[None, :]
    see = valid[:, None, :] & (((j - i).abs() <= w)[None] | glob[:, None, :])  # [B, S, S]
    s = torch.einsum("bihd,bjhd->bhij", q.double(), k.double()) * scale
    if lut is not None:
        s = s + lut.double()[:, (j - i) + (S - 1)][None]
    s = s.masked_fill(~see[:, None], float("-inf"))
    pr = torch.softmax(s, -1)
    if p > 0:
        pr = pr * attention_keep_mask(seed, p, B, H, S, S, q.device).double() / (1.0 - p)
    return torch.einsum("bhij,bjhd->bihd", pr, v.double())


def _case(S=37, w=4, B=2, H=2, D=8, globs=((0,), (0, 13)), pad=9, seed=0):
    torch.manual_seed(seed)
    q, k, v = (torch.randn(B, S, H, D, requires_grad=True) for _ in range(3))
    valid = torch.ones(B, S, dtype=torch.bool)
    valid[1, S - pad:] = False
    glob = torch.zeros(B, S, dtype=torch.bool)
    for b, gs in enumerate(globs):
        glob[b, list(gs)] = True
    return q, k, v, valid, glob


@pytest.mark.parametrize("bias,p", [(False, 0.0), (True, 0.0), (True, 0.1)])
def test_reference_matches_a_dense_formula(bias, p):
    q, k, v, valid, glob = _case()
    S, H = q.shape[1], q.shape[2]
    lut = (torch.randn(H, 2 * S - 1) * 0.5).requires_grad_(True) if bias else None
    o = A._reference(q, k, v, 0.3, False, valid, lut, p, 11, window=4, gk=glob)
    g = torch.randn_like(o) * valid[:, :, None, None]  # padded query rows carry no gradient (nothing reads them)
    ins = [q, k, v] + ([lut] if bias else [])
    got = torch.autograd.grad(o, ins, g)
    ins64 = [t.detach().double().requires_grad_(True) for t in ins]
    o64 = _dense(*ins64[:3], 0.3, valid, glob, 4, ins64[3] if bias else None, p, 11)
    ref = torch.autograd.grad(o64, ins64, g.double())
    torch.testing.assert_close(o[valid].double(), o64[valid], atol=2e-6, rtol=1e-5)
    for a, b in zip(got, ref):
        torch.testing.assert_close(a.double(), b, atol=5e-6, rtol=1e-5)
    # a far key reaches a row only as a global one: row 30 of batch 1... is padding; use batch 0, row 30 and key 0
    o_w = A._reference(q, k, v, 0.3, False, valid, lut, 0.0, 0, window=4)
    o_g = A._reference(q, k, v, 0.3, False, valid, lut, 0.0, 0, window=4, gk=glob)
    assert not torch.allclose(o_w[0, 30], o_g[0, 30])
    assert torch.allclose(o_w[0, 2], o_g[0, 2])  # key 0 lies inside row 2's window: counted once


def test_public_ops_take_global_keys_on_the_cpu():
    q, k, v, valid, glob = _case()
    ref = _dense(q, k, v, 0.3, valid, glob, 4, None, 0.0, 0)
    kw = dict(scale=0.3, key_padding_mask=valid, window=4)
    qkv = torch.stack((q, k, v), 2)
    for o in (A.attention(q, k, v, global_keys=glob, **kw),
              A.attention(q, k, v, global_keys=glob.to(torch.uint8), **kw),
              A.attention(q, k, v, global_keys=A.global_keys(glob), **kw),
              A.attention_qkv(qkv, global_keys=glob, **kw),
              A.attention_q_kv(q, torch.stack((k, v), 2), global_keys=glob, **kw)):
        torch.testing.assert_close(o[valid].double(), ref[valid], atol=2e-6, rtol=1e-5)


def test_block_list():
    """``GlobalKeys.blk``: per batch row the number of 64-key blocks with a global key, then their indices ascending."""
    f = torch.zeros(3, 333, dtype=torch.bool)
    f[0, [0, 63, 64, 127, 128, 332]] = True
    f[2, 200] = True
    gk = A.global_keys(f)
    assert gk.flags.dtype == torch.uint8 and gk.flags.shape == (3, 333) and gk.flags.is_contiguous()
    assert gk.blk.dtype == torch.int32 and gk.blk.shape == (3, 1 + 6)
    assert gk.blk[0, :5].tolist() == [4, 0, 1, 2, 5]
    assert gk.blk[1, 0].item() == 0
    assert gk.blk[2, :2].tolist() == [1, 3]
    assert A.global_keys(gk) is gk and A.global_keys(None) is None


def test_value_errors():
    q, k, v, valid, glob = _case()
    seg = torch.zeros(2, 37, dtype=torch.int32)
    qkv = torch.stack((q, k, v), 2)
    kv = torch.stack((k, v), 2)
    for call in (lambda **kw: A.attention(q, k, v, **kw), lambda **kw: A.attention_qkv(qkv, **kw),
                 lambda **kw: A.attention_q_kv(q, kv, **kw)):
        with pytest.raises(ValueError, match="window"):
            call(global_keys=glob)
        with pytest.raises(ValueError, match="causal"):
            call(global_keys=glob, window=4, causal=True)
        with pytest.raises(ValueError, match="segments"):
            call(global_keys=glob, window=4, q_segments=seg, k_segments=seg)
        with pytest.raises(ValueError, match="segments"):
            call(global_keys=glob, q_segments=seg, k_segments=seg)
        with pytest.raises(ValueError, match=r"\[B, Sk\]"):
            call(global_keys=glob[:, :30], window=4)
        with pytest.raises(ValueError, match="bool or integer"):
            call(global_keys=glob.float(), window=4)
    with pytest.raises(ValueError, match="window"):
        A._reference(q, k, v, 1.0, False, None, None, 0.0, 0, gk=glob)


def test_no_global_key_is_the_window_and_all_global_is_full_attention():
    q, k, v, valid, glob = _case()
    args = (q, k, v, 0.3, False, valid, None, 0.1, 5)
    none = A._reference(*args, window=4, gk=torch.zeros_like(glob))
    assert torch.equal(none, A._reference(*args, window=4))
    every = A._reference(*args, window=4, gk=torch.ones_like(glob))
    assert torch.equal(every, A._reference(*args))
