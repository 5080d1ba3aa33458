"""Block lists in the attention op on the CPU (ops/attention.py ``block_lists`` / ``BlockLists`` and the composite
``_reference``): the dense definition — a key counts once per occurrence of its block in the list of the query's block,
which is ``+ log(multiplicity)`` on the scores and hidden where unlisted — against an fp64 reference written here from
that sentence, forward and gradients; the kernels' tables (CSR lists in 64-blocks and their transpose); validation and
routing.  The composite computes in fp32: its bounds are fp32 rounding on sums of a few hundred terms (1e-5 relative)."""
import math

import numpy as np
import pytest
import torch

from distributed_llms_example_amd.ops import attention as A
from distributed_llms_example_amd.ops import routing
from distributed_llms_example_amd.ops.rng import attention_keep_mask


def _dense_counts(kl, H, nq, nk):
    """[H, nq, nk] multiplicities of per-head (or shared) lists, by a plain loop."""
    heads = kl if not (len(kl[0]) == 0 or np.ndim(kl[0][0]) == 0) else [kl]
    m = torch.zeros(H, nq, nk, dtype=torch.float64)
    for h in range(H):
        for x, lst in enumerate(heads[h % len(heads)]):
            for j in lst:
                if 0 <= j < nk:
                    m[h, x, j] += 1
    return m


def _ref64(q, k, v, scale, kpm, lut, p, seed, kl, block):
    """fp64: softmax over the listed keys, a key listed n times entering n times.  Rows without a listed key: 0."""
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    qf, kf, vf = (t.double().permute(0, 2, 1, 3) for t in (q, k, v))
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if lut is not None:
        rel = torch.arange(Sk)[None, :] - torch.arange(Sq)[:, None] + (Sq - 1)
        s = s + lut.double()[:, rel].unsqueeze(0)
    m = _dense_counts(kl, H, -(-Sq // block), -(-Sk // block))
    m = m.repeat_interleave(block, 1)[:, :Sq].repeat_interleave(block, 2)[:, :, :Sk][None].expand(B, H, Sq, Sk)
    if kpm is not None:
        m = m * kpm.bool()[:, None, None, :].double()
    e = torch.exp(s - s.max(-1, keepdim=True).values.detach()) * m  # n copies of a key: n times its weight
    den = e.sum(-1, keepdim=True)
    pr = torch.where(den > 0, e / den.clamp_min(1e-300), torch.zeros_like(e))
    if p > 0.0:
        pr = pr * attention_keep_mask(seed, p, B, H, Sq, Sk, q.device).double() / (1.0 - p)
    return torch.matmul(pr, vf).permute(0, 2, 1, 3)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


# repeats (block 1 twice in row 1, block 4 three times in head 1's last row), an empty list (row 2 of head 0), an
# unlisted key block (block 3 of head 1), lists of different lengths and orders, an out-of-range entry (7: passed over)
KL = [[[0, 1], [1, 1, 2], [], [0, 4, 7], [4, 3, 0]],
      [[0], [1, 0, 1], [2], [2, 4], [4, 4, 4]]]


@pytest.mark.parametrize("bias,kpm,p", [(False, False, 0.0), (True, True, 0.0), (True, True, 0.25), (False, True, 0.25)])
def test_composite_matches_fp64_definition(bias, kpm, p):
    torch.manual_seed(0)
    B, S, H, D, block = 2, 19, 2, 8, 4  # 5 blocks, the last partial (3 keys)
    q, k, v = (torch.randn(B, S, H, D, requires_grad=True) for _ in range(3))
    lut = (torch.randn(H, 2 * S - 1) * 0.5).requires_grad_(True) if bias else None
    mask = None
    if kpm:
        mask = torch.ones(B, S, dtype=torch.bool)
        mask[1, 13:] = False
    bl = A.block_lists(KL, block=block)
    assert (bl.heads, bl.nq, bl.nk, bl.block) == (2, 5, 5, 4)
    o = A.attention(q, k, v, scale=0.3, key_padding_mask=mask, bias_lut=lut, dropout_p=p, seed=11, block_lists=bl)
    g = torch.randn(B, S, H, D)
    g[:, 8:12, 0] = 0  # head 0, block 2: the empty list (the fp64 reference has no gradient there either)
    ins = [q, k, v] + ([lut] if bias else [])
    grads = torch.autograd.grad(o, ins, g)
    ins64 = [t.detach().double().requires_grad_(True) for t in ins]
    o64 = _ref64(ins64[0], ins64[1], ins64[2], 0.3, mask, ins64[3] if bias else None, p, 11, KL, block)
    grads64 = torch.autograd.grad(o64, ins64, g.double())
    assert o[:, 8:12, 0].abs().max().item() == 0  # empty list: output 0
    assert _rel(o, o64) < 1e-5
    for n, a, b in zip(("dq", "dk", "dv", "dlut"), grads, grads64):
        assert _rel(a, b) < 1e-5, n
    # an unlisted key block gets no gradient: block 3 (keys 12 .. 15) of head 1
    assert grads[1][:, 12:16, 1].abs().max().item() == 0 and grads[2][:, 12:16, 1].abs().max().item() == 0
    assert grads[1][:, 12:16, 0].abs().max().item() > 0
    # the repeat is seen: dropping the second "1" of head 0's row 1 changes that row block and nothing else
    kl2 = [[list(r) for r in hd] for hd in KL]
    kl2[0][1] = [1, 2]
    o2 = A.attention(q, k, v, scale=0.3, key_padding_mask=mask, bias_lut=lut, dropout_p=p, seed=11,
                     block_lists=A.block_lists(kl2, block=block))
    assert not torch.equal(o2[:, 4:8, 0], o[:, 4:8, 0])
    o2[:, 4:8, 0] = o[:, 4:8, 0]
    assert torch.equal(o2, o)


def test_repeat_is_log_multiplicity():
    """One query block listing [0, 0, 1] is full attention with log 2 added to the scores of block 0's keys."""
    torch.manual_seed(1)
    B, S, H, D = 1, 8, 1, 4
    q, k, v = (torch.randn(B, S, H, D) for _ in range(3))
    o = A.attention(q, k, v, scale=0.5, block_lists=A.block_lists([[0, 0, 1], [0, 0, 1]], block=4))
    s = torch.einsum("bqhd,bkhd->bhqk", q, k).double() * 0.5
    s[..., :4] += math.log(2.0)
    ref = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v.double())
    assert _rel(o, ref) < 1e-6


def test_shared_list_and_packed_forms():
    torch.manual_seed(2)
    B, S, H, D = 2, 19, 2, 8
    qkv = torch.randn(B, S, 3, H, D)
    shared = A.block_lists(KL[0], block=4)
    assert shared.heads == 1
    per_head = A.block_lists([KL[0], KL[0]], block=4)
    a = A.attention_qkv(qkv, scale=0.3, block_lists=shared)
    b = A.attention_qkv(qkv, scale=0.3, block_lists=per_head)
    c = A.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], scale=0.3, block_lists=shared)
    d = A.attention_q_kv(qkv[:, :, 0], qkv[:, :, 1:], scale=0.3, block_lists=shared)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


def test_raw_lists_default_to_block_64():
    qkv = torch.randn(1, 19, 3, 1, 8)
    with pytest.raises(ValueError, match="5 x 5 blocks of 64"):
        A.attention_qkv(qkv, block_lists=KL[0])  # 5 lists of 64-blocks do not fit 19 tokens


def test_full_list_is_full_attention():
    torch.manual_seed(3)
    qkv = torch.randn(2, 19, 3, 2, 8)
    full = A.block_lists([list(range(5))] * 5, block=4)
    assert _rel(A.attention_qkv(qkv, scale=0.3, block_lists=full), A.attention_qkv(qkv, scale=0.3)) < 1e-6


def _csr_lists(ptr, idx, h):
    return [idx[ptr[h, x]:ptr[h, x + 1]].tolist() for x in range(ptr.shape[1] - 1)]


def test_tables_at_block_64():
    """The kernels' tables of a block-64 pattern at S = 300 (5 blocks): the lists as given minus out-of-range entries,
    and the transpose with every multiplicity."""
    kl = [[[0, 1], [1, 1, 2], [], [0, 4, 7], [4, 3, 0]], [[0], [1, 0, 1], [2], [2, 4], [4, 4, 4]]]
    bl = A.block_lists(kl)
    t = bl.tables("cpu", 300, 300)
    assert all(t[k].dtype == torch.int32 for k in t)
    assert t["kl_ptr"].shape == (2, 6) and t["ql_ptr"].shape == (2, 6)
    assert t["kl_idx"].numel() == t["ql_idx"].numel() == int(t["kl_ptr"][-1, -1])
    for h in range(2):
        got = _csr_lists(t["kl_ptr"], t["kl_idx"], h)
        assert got == [[j for j in lst if j < 5] for lst in kl[h]]
        tr = _csr_lists(t["ql_ptr"], t["ql_idx"], h)
        want = [[x for x in range(5) for j in kl[h][x] if j == kb] for kb in range(5)]
        assert tr == want
    assert _csr_lists(t["ql_ptr"], t["ql_idx"], 1)[3] == []  # the unlisted key block
    assert bl.tables("cpu", 300, 300) is t  # built once


def test_tables_expand_multiples_of_64():
    """Block 128 at S = 300: 3 blocks of 128 become 5 blocks of 64 (the sixth lies past the end), every listed block two
    wide in every row of the pair, repeats kept."""
    bl = A.block_lists([[0, 2], [1, 1], [2, 0]], block=128)
    t = bl.tables("cpu", 300, 300)
    kl = _csr_lists(t["kl_ptr"], t["kl_idx"], 0)
    assert kl == [[0, 1, 4], [0, 1, 4], [2, 3, 2, 3], [2, 3, 2, 3], [4, 0, 1]]
    ql = _csr_lists(t["ql_ptr"], t["ql_idx"], 0)
    assert ql == [[0, 1, 4], [0, 1, 4], [2, 2, 3, 3], [2, 2, 3, 3], [0, 1, 4]]
    dense = bl.counts()
    assert dense.tolist() == [[[1, 0, 1], [0, 2, 0], [1, 0, 1]]]
    with pytest.raises(ValueError, match="no multiple"):
        A.block_lists([[0]], block=8).tables("cpu", 8, 8)


def test_validation():
    q = torch.randn(2, 19, 2, 8)
    bl = A.block_lists(KL, block=4)
    kw = dict(block_lists=bl)
    with pytest.raises(ValueError, match="block_lists with causal"):
        A.attention(q, q, q, causal=True, **kw)
    with pytest.raises(ValueError, match="block_lists with a window"):
        A.attention(q, q, q, window=3, **kw)
    seg = torch.zeros(2, 19, dtype=torch.int32)
    with pytest.raises(ValueError, match="block_lists with segments"):
        A.attention(q, q, q, q_segments=seg, k_segments=seg, **kw)
    with pytest.raises(ValueError, match="1 or 3"):
        A.attention(torch.randn(2, 19, 3, 8), torch.randn(2, 19, 3, 8), torch.randn(2, 19, 3, 8), **kw)
    with pytest.raises(ValueError, match="5 x 5 blocks of 4"):
        A.attention(q[:, :16], q[:, :16], q[:, :16], **kw)
    with pytest.raises(ValueError, match="5 x 5 blocks of 4"):
        A.attention(q, q[:, :12], q[:, :12], **kw)
    with pytest.raises(ValueError, match="query blocks"):
        A.block_lists([[[0], [1]], [[0]]], block=4)
    with pytest.raises(ValueError, match="integer"):
        A.block_lists([[0.5], [1.0]], block=4)
    with pytest.raises(ValueError, match="block size"):
        A.block_lists([[0]], block=0)
    assert A.block_lists(None) is None and A.block_lists(bl) is bl
    # cross-attention shapes: 5 query blocks against 3 key blocks
    cross = A.block_lists([[0], [1], [2], [0, 2], [1]], block=4, num_key_blocks=3)
    o = A.attention(q, q[:, :12], q[:, :12], block_lists=cross)
    assert o.shape == q.shape


def test_numpy_lists():
    qkv = torch.randn(1, 16, 3, 2, 8)
    rows = np.array([[0, 1], [1, 2], [2, 3], [3, 0]])
    a = A.attention_qkv(qkv, block_lists=A.block_lists(rows, block=4))
    b = A.attention_qkv(qkv, block_lists=A.block_lists([rows, rows.tolist()], block=4))
    assert torch.equal(a, b)


def test_route_key(monkeypatch):
    assert routing.DEFAULTS["attn_lists"] == 1
    assert routing.attention_route(64, True, lists=True) == "attn_hd.hip"
    assert routing.attention_route(64, False, lists=True) == "attn_f32.hip"
    assert routing.attention_route(64, True) == "attn.hip"
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(attn_lists=0))
    assert routing.attention_route(64, True, lists=True) == "composite"
    assert routing.attention_route(64, True) == "attn.hip"
    monkeypatch.setenv("DLLM_ROUTE", "attn_list=0")
    with pytest.raises(KeyError, match="unknown key"):
        routing.get("attn_lists")
