"""Segment-masked attention on the CPU: the composite with segments (the oracle of tests/test_attn_segments_gpu.py and
the CPU path of packed training) against every segment run alone, the op's argument checks, the block tables and the
routing table."""
import pytest
import torch

from distributed_llms_example_amd.ops import attention as A, routing
from distributed_llms_example_amd.ops.rng import attention_keep_mask

B, H, D = 2, 3, 8


def _ids(bounds, S, tail):
    """ids 0, 1, 2, ... with segment starts at 0 and ``bounds`` and -1 from ``tail`` on."""
    seg = torch.zeros(S, dtype=torch.int64)
    for b in bounds:
        seg[b:] += 1
    seg[tail:] = -1
    return seg


def _alone64(q, k, v, scale, causal, lut, keep, p):
    """One segment on its own in fp64: q [n, H, D], k / v [m, H, D], lut [H, n + m - 1] in the segment's own frame
    (or None), keep [H, n, m] the packed call's dropout decisions of this (rows, keys) slice (or None)."""
    n, m = q.shape[0], k.shape[0]
    s = torch.einsum("ihd,jhd->hij", q, k) * scale
    ar_n, ar_m = torch.arange(n), torch.arange(m)
    if lut is not None:
        s = s + lut[:, ar_m[None, :] - ar_n[:, None] + (n - 1)]
    if causal:
        s = s.masked_fill(ar_m[None, :] > ar_n[:, None], float("-inf"))
    pr = torch.softmax(s, -1)
    if keep is not None:
        pr = pr * keep.double() / (1.0 - p)
    return torch.einsum("hij,jhd->ihd", pr, v)


def _per_segment64(q, k, v, qs, ks, scale, causal, lut, p, seed):
    """Every segment alone, concatenated; rows of padding (-1) stay 0.  fp64, differentiable in q / k / v / lut."""
    Sq, Sk = q.shape[1], k.shape[1]
    keep = attention_keep_mask(seed, p, B, H, Sq, Sk, q.device) if p > 0 else None
    rows = []
    for b in range(B):
        out = [torch.zeros(1, H, D, dtype=torch.float64) for _ in range(Sq)]
        for g in range(int(qs[b].max()) + 1):
            ri, ki = (qs[b] == g).nonzero().flatten(), (ks[b] == g).nonzero().flatten()
            a, c, n, m = int(ri[0]), int(ki[0]), len(ri), len(ki)
            assert (ri == torch.arange(a, a + n)).all() and (ki == torch.arange(c, c + m)).all()
            # lut_seg[h, (j' - i') + n - 1] = lut[h, (c + j') - (a + i') + Sq - 1]
            lo = c - a + Sq - 1 - (n - 1)
            o = _alone64(q[b, a:a + n], k[b, c:c + m], v[b, c:c + m], scale, causal,
                         lut[:, lo:lo + n + m - 1] if lut is not None else None,
                         keep[b, :, a:a + n, c:c + m] if keep is not None else None, p)
            for i in range(n):
                out[a + i] = o[i:i + 1]
        rows.append(torch.cat(out, 0))
    return torch.stack(rows, 0)


CASES = {
    # name: (Sq, Sk, q ids, k ids, causal)
    "self": (23, 23, (_ids([1, 9, 15], 23, 20), _ids([5, 6], 23, 23)), None, False),
    "causal": (23, 23, (_ids([1, 9, 15], 23, 20), _ids([12], 23, 19)), None, True),
    "cross": (11, 23, (_ids([2, 3], 11, 9), _ids([4], 11, 11)), (_ids([10, 14], 23, 21), _ids([7], 23, 20)), False),
}


# (the relative bias is a self-attention term: the cross shape runs without it, with and without dropout)
@pytest.mark.parametrize("case,bias,p", [("self", False, 0.0), ("self", True, 0.1), ("causal", False, 0.0),
                                         ("causal", True, 0.1), ("cross", False, 0.0), ("cross", False, 0.1)])
def test_reference_with_segments_is_every_segment_alone(case, bias, p):
    """Output and every gradient of the composite with segments (fp32) against each segment run alone in fp64 and
    concatenated.  Tolerance: fp32 rounding (2^-24 per operation) of sums of at most 23 products of O(1 .. 10) terms —
    a few 1e-6 — held at 2e-5 absolute, 1e-5 relative (tests/test_attn_window_cpu.py holds the composite to 1e-5
    against its fp64 brute force)."""
    Sq, Sk, qids, kids, causal = CASES[case]
    kids = kids if kids is not None else qids
    qs, ks = torch.stack(qids), torch.stack(kids)
    g = torch.Generator().manual_seed(Sq + Sk)
    q = torch.randn(B, Sq, H, D, generator=g).requires_grad_(True)
    k, v = (torch.randn(B, Sk, H, D, generator=g).requires_grad_(True) for _ in range(2))
    lut = torch.randn(H, Sq + Sk - 1, generator=g).requires_grad_(True) if bias else None
    go = torch.randn(B, Sq, H, D, generator=g)
    ins = [t for t in (q, k, v, lut) if t is not None]
    o = A._reference(q, k, v, 0.5, causal, None, lut, p, 11, None, qs, ks)
    grads = torch.autograd.grad(o, ins, go)
    ins64 = [t.detach().double().requires_grad_(True) for t in ins]
    o64 = _per_segment64(*ins64[:3], qs, ks, 0.5, causal, ins64[3] if bias else None, p, 11)
    grads64 = torch.autograd.grad(o64, ins64, go.double())
    assert (o[qs < 0] == 0).all()  # a padding row sees no key: output 0
    torch.testing.assert_close(o.double(), o64, atol=2e-5, rtol=1e-5)
    for n, a, b in zip(("dq", "dk", "dv", "dlut"), grads, grads64):
        torch.testing.assert_close(a.double(), b, atol=2e-5, rtol=1e-5, msg=lambda m, n=n: f"{n}: {m}")
    assert (grads[0][qs < 0] == 0).all() and (grads[1][ks < 0] == 0).all() and (grads[2][ks < 0] == 0).all()


def test_ops_carry_the_segments_on_cpu():
    Sq, Sk, qids, _, _ = CASES["self"]
    seg = torch.stack(qids)
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, Sq, H, D, generator=g) for _ in range(3))
    lut = torch.randn(H, 2 * Sq - 1, generator=g)
    ref = A._reference(q, k, v, 1.0, False, None, lut, 0.1, 3, None, seg, seg)
    kw = dict(scale=1.0, bias_lut=lut, dropout_p=0.1, seed=3)
    assert torch.equal(A.attention(q, k, v, q_segments=seg, k_segments=seg, **kw), ref)
    assert torch.equal(A.attention(q, k, v, q_segments=A.segments(seg), k_segments=seg.int(), **kw), ref)
    assert torch.equal(A.attention_qkv(torch.stack([q, k, v], 2), segments=seg, **kw), ref)
    assert torch.equal(A.attention_q_kv(q, torch.stack([k, v], 2), q_segments=seg, k_segments=seg, **kw), ref)
    assert not torch.equal(A.attention(q, k, v, **kw), ref)
    # one segment over everything masks nothing
    one = torch.zeros(B, Sq, dtype=torch.int64)
    assert torch.equal(A.attention(q, k, v, q_segments=one, k_segments=one, **kw), A.attention(q, k, v, **kw))


def test_reference_without_segments_is_unchanged():
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(B, 9, H, D, generator=g) for _ in range(3))
    assert torch.equal(A._reference(q, k, v, 0.5, True, None, None, 0.1, 7),
                       A._reference(q, k, v, 0.5, True, None, None, 0.1, 7, None, None, None))


def test_rejected_combinations():
    seg = torch.zeros(B, 9, dtype=torch.int64)
    q = torch.randn(B, 9, H, D)
    with pytest.raises(ValueError, match="together"):
        A.attention(q, q, q, q_segments=seg)
    with pytest.raises(ValueError, match="together"):
        A.attention_q_kv(q, torch.stack([q, q], 2), k_segments=seg)
    with pytest.raises(ValueError, match="window"):
        A.attention(q, q, q, q_segments=seg, k_segments=seg, window=3)
    with pytest.raises(ValueError, match="window"):
        A.attention_qkv(torch.stack([q, q, q], 2), segments=seg, window=3)
    with pytest.raises(ValueError, match="int32 or int64"):
        A.attention(q, q, q, q_segments=seg.float(), k_segments=seg)
    with pytest.raises(ValueError, match="int32 or int64"):
        A.attention(q, q, q, q_segments=seg[0], k_segments=seg)
    with pytest.raises(ValueError, match=r"k_segments must be \[B, S\]"):
        A.attention(q, q, q, q_segments=seg, k_segments=seg[:, :8])
    with pytest.raises(ValueError, match=r"q_segments must be \[B, S\]"):
        A.attention(q, q, q, q_segments=seg[:1], k_segments=seg)


def test_block_tables():
    """Per 64-block (min, max) of the non-negative ids; (INT_MAX, -1) for a block without one."""
    ids = torch.full((2, 150), -1, dtype=torch.int64)
    ids[0, :70] = torch.arange(70) // 30        # block 0: ids 0 .. 2, block 1: id 2 then padding, block 2: padding
    ids[1, 60:140] = 5
    sg = A.segments(ids)
    assert sg.ids.dtype == torch.int32 and sg.ids.is_contiguous() and sg.blk.dtype == torch.int32
    big = 2**31 - 1
    assert sg.blk.tolist() == [[[0, 2], [2, 2], [big, -1]], [[5, 5], [5, 5], [5, 5]]]
    assert A.segments(sg) is sg and A.segments(None) is None


def test_segment_routes():
    assert routing.attention_route(64, True, segments=True) == "attn_hd.hip"
    assert routing.attention_route(64, False, segments=True) == "attn_f32.hip"
    for d in (32, 40, 96, 128):
        assert routing.attention_route(d, True, segments=True) == "attn_hd.hip", d
    assert routing.attention_route(16, True, segments=True) == "composite"
    assert routing.attention_route(128, False, segments=True) == "composite"
    # without segments: unchanged
    assert routing.attention_route(64) == "attn.hip"
    assert routing.attention_route(64, True, None, segments=False) == "attn.hip"
    assert routing.attention_route(64, False) == "attn_f32.hip"
    assert routing.attention_route(64, True, 127) == "attn_hd.hip"
    assert routing.attention_route(128, True) == "attn_hd.hip"


def test_route_switches_apply_to_segmented_calls(monkeypatch):
    monkeypatch.setenv("DLLM_ROUTE", "attn_hd=0,attn_f32=0")
    assert routing.attention_route(64, True, segments=True) == "composite"
    assert routing.attention_route(64, False, segments=True) == "composite"
    assert routing.attention_route(64, True) == "attn.hip"


def test_cpu_tensors_take_the_composite_with_segments():
    q = torch.randn(1, 9, 2, 64)
    assert A._route(q, q, q, seg=True) is None
    assert A._route(q.bfloat16(), seg=True) is None
