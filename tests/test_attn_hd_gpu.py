"""csrc/attn_hd.hip: bf16 flash attention at head dims 32 .. 128 other than 64, against the fp32 composite
(``A._reference`` on fp32 copies of the same bf16 values; dropout through the shared counter-based mask, so p > 0 is
compared exactly).  Metric, construction and bounds are those of tests/test_kernels_gpu.py::test_attention: rel-L2,
2e-2 on the output, 3e-2 on the gradients (6e-2 for a single query row), the bias gradient checked on the bucket
table."""
import pytest
import torch

from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops import attention as A, rng, routing
from distributed_llms_example_amd.parallel import context as CP

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


class _Spy:
    """The native module with calls to the attention forwards recorded by name."""

    def __init__(self, calls, real):
        self.calls = calls
        self.real = real  # the module itself, taken before ``native`` is patched

    def __getattr__(self, n):
        real = getattr(self.real, n)
        if n in ("attn_fwd", "attn_hd_fwd", "attn_f32_fwd"):
            def f(*a, **kw):
                self.calls.append(n)
                return real(*a, **kw)
            return f
        return real


HD_CASES = [
    # B, H, Sq, Sk, D, bias, kpm, causal, p, scale
    (2, 3, 200, 200, 128, True, True, False, 0.1, 1.0),          # t5-3b encoder, ragged tiles
    (2, 2, 130, 130, 128, True, False, True, 0.1, 1.0),          # T5 decoder
    (1, 2, 77, 300, 128, False, True, False, 0.0, 128 ** -0.5),  # cross-attention
    (1, 2, 1, 33, 128, True, False, True, 0.0, 1.0),             # decode step, k / v slices of a longer cache buffer
    (1, 2, 64, 128, 80, False, False, True, 0.0, 80 ** -0.5),    # causal with Sk > Sq; DP = 96 with zero columns
    (2, 4, 96, 96, 40, False, False, True, 0.1, 40 ** -0.5),     # Blenderbot decoder; DP = 64 padded
    (2, 4, 64, 600, 40, False, "heavy", False, 0.1, 40 ** -0.5),  # whole key tiles padded
    (2, 2, 150, 150, 32, True, True, False, 0.0, 1.0),
]


@pytest.mark.parametrize("B,H,Sq,Sk,D,bias,kpm,causal,p,scale", HD_CASES)
def test_attn_hd(B, H, Sq, Sk, D, bias, kpm, causal, p, scale, monkeypatch):
    calls = []
    spy = _Spy(calls, _ext.native())
    monkeypatch.setattr(A._ext, "native", lambda: spy)
    torch.manual_seed(Sq * 7 + Sk + D)
    q = torch.randn(B, Sq, H, D, device=DEV).to(torch.bfloat16)
    if Sq == 1:  # the decode step reads its keys / values out of a longer cache buffer (strided views)
        kbuf = torch.randn(B, 64, H, D, device=DEV).to(torch.bfloat16)
        vbuf = torch.randn(B, 64, H, D, device=DEV).to(torch.bfloat16)
        k, v = kbuf[:, :Sk], vbuf[:, :Sk]
    else:
        k = torch.randn(B, Sk, H, D, device=DEV).to(torch.bfloat16)
        v = torch.randn(B, Sk, H, D, device=DEV).to(torch.bfloat16)
    table = torch.randn(32, H, device=DEV) * 0.5 if bias else None
    mask = None
    if kpm:
        mask = torch.ones(B, Sk, dtype=torch.bool, device=DEV)
        mask[0, Sk - Sk // 5:] = False
        if kpm == "heavy":  # batch 0: only the first 70 keys are real
            mask[0, 70:] = False
    seed = 4242
    qs = q.clone().requires_grad_(True)
    if Sq == 1:
        kbs, vbs = kbuf.clone().requires_grad_(True), vbuf.clone().requires_grad_(True)
        ks, vs = kbs[:, :Sk], vbs[:, :Sk]
    else:
        ks, vs = k.clone().requires_grad_(True), v.clone().requires_grad_(True)
    tab1 = table.clone().requires_grad_(True) if bias else None
    lut = A.relative_bias_lut(tab1, Sq, Sk, not causal, 32, 128, q_offset=Sk - Sq) if bias else None
    o = A.attention(qs, ks, vs, scale=scale, causal=causal, key_padding_mask=mask, bias_lut=lut, dropout_p=p, seed=seed)
    assert calls == ["attn_hd_fwd"], calls
    assert o.shape == (B, Sq, H, D) and o.dtype == torch.bfloat16
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    tab2 = table.clone().requires_grad_(True) if bias else None
    lut2 = A.relative_bias_lut(tab2, Sq, Sk, not causal, 32, 128, q_offset=Sk - Sq) if bias else None
    ref = A._reference(qr, kr, vr, scale, causal, mask, lut2, p, seed)
    e = _rel(o, ref)
    print(f"[attn_hd D={D} Sq={Sq} Sk={Sk}] o {e:.5f}")
    assert e < 2e-2, e
    g = torch.randn_like(o)
    (o.float() * g.float()).sum().backward()
    (ref * g.float()).sum().backward()
    tol = 6e-2 if Sq < 4 else 3e-2
    kg, vg = (kbs.grad[:, :Sk], vbs.grad[:, :Sk]) if Sq == 1 else (ks.grad, vs.grad)
    errs = {"dq": _rel(qs.grad, qr.grad), "dk": _rel(kg, kr.grad), "dv": _rel(vg, vr.grad)}
    if bias:
        errs["dtable"] = _rel(tab1.grad, tab2.grad)
    print(f"[attn_hd D={D} Sq={Sq} Sk={Sk}] {errs}")
    for name, err in errs.items():
        assert err < tol, (name, err)
    if Sq == 1:  # nothing written past the keys in use
        assert kbs.grad[:, Sk:].abs().max().item() == 0 and vbs.grad[:, Sk:].abs().max().item() == 0


def test_attn_hd_row_without_valid_key():
    """Batch row 0 has no valid key: its output rows are 0 (the kernels' convention, LSE = +inf) and every gradient
    is finite; batch row 1 matches the reference."""
    torch.manual_seed(3)
    B, H, S, D = 2, 2, 100, 128
    q, k, v = (torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16).requires_grad_(True) for _ in range(3))
    mask = torch.ones(B, S, dtype=torch.bool, device=DEV)
    mask[0] = False
    o = A.attention(q, k, v, scale=D ** -0.5, key_padding_mask=mask, dropout_p=0.1, seed=9)
    assert o[0].abs().max().item() == 0
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    ref = A._reference(qr, kr, vr, D ** -0.5, False, mask, None, 0.1, 9)
    assert _rel(o[1], ref[1]) < 2e-2
    g = torch.randn_like(o)
    (o.float() * g.float()).sum().backward()
    (ref * g.float()).sum().backward()
    for t, r in ((q, qr), (k, kr), (v, vr)):
        assert torch.isfinite(t.grad.float()).all()
        assert t.grad[0].abs().max().item() == 0
        assert _rel(t.grad[1], r.grad[1]) < 3e-2
    o2, lse = _ext.native().attn_hd_fwd(q.detach(), k.detach(), v.detach(), mask.to(torch.uint8), None, D ** -0.5,
                                        False, 0.0, 0)
    assert torch.isposinf(lse[0]).all() and torch.isfinite(lse[1]).all()


def test_attn_hd_packed_modes():
    B, S, H, D = 2, 150, 4, 40
    sc = D ** -0.5
    torch.manual_seed(1)
    qkv = torch.randn(B, S, 3, H, D, device=DEV).to(torch.bfloat16).requires_grad_(True)
    o = A.attention_qkv(qkv, scale=sc, causal=True)
    r = qkv.detach().float().requires_grad_(True)
    ref = A._reference(r[:, :, 0], r[:, :, 1], r[:, :, 2], sc, True, None, None, 0.0, 0)
    assert _rel(o, ref) < 2e-2
    g = torch.randn_like(o)
    (o.float() * g.float()).sum().backward()
    (ref * g.float()).sum().backward()
    assert qkv.grad.shape == qkv.shape
    for i in range(3):
        assert _rel(qkv.grad[:, :, i], r.grad[:, :, i]) < 3e-2, i
    kvin = torch.randn(B, 70, 2, H, D, device=DEV).to(torch.bfloat16).requires_grad_(True)
    into = torch.full_like(kvin, float("nan"))
    kvin._dllm_grad_into = into
    q = torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16).requires_grad_(True)
    o2 = A.attention_q_kv(q, kvin, scale=sc)
    kr = kvin.detach().float().requires_grad_(True)
    qr = q.detach().float().requires_grad_(True)
    ref2 = A._reference(qr, kr[:, :, 0], kr[:, :, 1], sc, False, None, None, 0.0, 0)
    assert _rel(o2, ref2) < 2e-2
    g2 = torch.randn_like(o2)
    (o2.float() * g2.float()).sum().backward()
    (ref2 * g2.float()).sum().backward()
    assert _rel(q.grad, qr.grad) < 3e-2
    assert _rel(kvin.grad, kr.grad) < 3e-2
    # dK / dV were written by the kernel straight into the buffer the producer named (it held NaN before)
    assert _rel(into[:, :, 0], kr.grad[:, :, 0]) < 3e-2 and _rel(into[:, :, 1], kr.grad[:, :, 1]) < 3e-2


def test_attn_hd_route(monkeypatch):
    calls = []
    spy = _Spy(calls, _ext.native())
    monkeypatch.setattr(A._ext, "native", lambda: spy)

    def run(D):
        del calls[:]
        x = torch.randn(1, 64, 2, D, device=DEV, dtype=torch.bfloat16)
        A.attention(x, x, x)
        return list(calls)

    assert run(128) == ["attn_hd_fwd"]
    assert run(40) == ["attn_hd_fwd"]
    assert run(64) == ["attn_fwd"]
    assert run(16) == []
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(attn_hd=0))
    assert run(128) == []
    assert run(64) == ["attn_fwd"]


def test_attn_hd_memory():
    """O(S) memory: forward + backward at S = 2048 allocates less than half of ONE fp32 score tensor of the composite
    (2 x 2048^2 x 4 B = 32 MiB); q, k, v, o, lse and their gradients together are under 10 MiB."""
    B, H, S, D = 1, 2, 2048, 128
    q, k, v = (torch.randn(B, S, H, D, device=DEV, dtype=torch.bfloat16, requires_grad=True) for _ in range(3))
    g = torch.randn(B, S, H, D, device=DEV, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    o = A.attention(q, k, v, scale=D ** -0.5, dropout_p=0.1, seed=3)
    o.backward(g)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"[attn_hd memory] rise {rise / 2**20:.2f} MiB")
    assert rise < 16 * 2**20, rise


def test_attn_hd_graph_seed_step():
    """With the device step counter set, the kernels draw the mask of seed mix_host(seed, step): equal to the reference
    run with that seed, and different between steps 0 and 1."""
    torch.manual_seed(5)
    B, H, S, D = 1, 2, 96, 128
    q, k, v = (torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16) for _ in range(3))
    seed, p = 77, 0.1
    C = _ext.native()
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    outs = []
    try:
        C.set_seed_step(step)
        for s in (0, 1):
            step.fill_(s)
            o = A.attention(q, k, v, scale=D ** -0.5, dropout_p=p, seed=seed)
            ref = A._reference(q.float(), k.float(), v.float(), D ** -0.5, False, None, None, p,
                               rng.mix_host(seed, s))
            assert _rel(o, ref) < 2e-2, (s, _rel(o, ref))
            outs.append(o)
        torch.cuda.synchronize()
    finally:
        C.set_seed_step(None)
    assert _rel(outs[0], outs[1]) > 0.1


def test_attn_hd_chunked_blocks():
    """Long-sequence blocks (parallel/context.py) at head dim 128: chunked_attention in 128-token blocks against the
    single call, output and dq / dk / dv / dtable."""
    torch.manual_seed(11)
    B, N, H, D = 1, 512, 2, 128
    q, k, v = (torch.randn(B, N, H, D, device=DEV).to(torch.bfloat16) for _ in range(3))
    table = torch.randn(32, H, device=DEV) * 0.5
    mask = torch.ones(B, N, dtype=torch.bool, device=DEV)
    mask[0, N - 100:] = False
    g = torch.randn(B, N, H, D, device=DEV).to(torch.bfloat16)
    res = []
    for chunked in (True, False):
        qs, ks, vs = (t.clone().requires_grad_(True) for t in (q, k, v))
        tab = table.clone().requires_grad_(True)
        if chunked:
            o = CP.chunked_attention(qs, ks, vs, chunk=128, scale=1.0, key_padding_mask=mask, bias_table=tab)
        else:
            lut = A.relative_bias_lut(tab, N, N, True, 32, 128)
            o = A.attention(qs, ks, vs, scale=1.0, key_padding_mask=mask, bias_lut=lut)
        (o.float() * g.float()).sum().backward()
        res.append((o, qs.grad, ks.grad, vs.grad, tab.grad))
    names = ("o", "dq", "dk", "dv", "dtable")
    for n, a, b in zip(names, res[0], res[1]):
        e = _rel(a, b)
        print(f"[attn_hd chunked] {n} {e:.5f}")
        assert e < (2e-2 if n == "o" else 3e-2), (n, e)


def test_block_fwd_unsupported_head_dim_takes_reference():
    """A head dim no kernel serves goes to the plain-torch block functions on the GPU instead of raising."""
    torch.manual_seed(2)
    q, k, v = (torch.randn(1, 64, 2, 16, device=DEV, dtype=torch.bfloat16) for _ in range(3))
    o, lse, dmask = CP._block_fwd(q, k, v, None, None, None, 0.25, 0.0, 0)
    o_ref, lse_ref = CP._ref_block_fwd(q, k, v, None, None, 0.25, 0.0, 0)
    assert dmask is None
    assert torch.equal(o, o_ref) and torch.equal(lse, lse_ref)
    do = torch.randn_like(q)
    grads = CP._block_bwd(do, q, k, v, o.to(q.dtype), lse, None, None, None, 0.25, 0.0, 0, False, None)
    assert all(torch.isfinite(t.float()).all() for t in grads[:3])


def test_composite_on_gpu_warns_once_per_reason(monkeypatch, caplog):
    """A GPU tensor that no kernel serves takes the composite with ONE warning per process and reason, naming the head
    dim and the O(Sq*Sk) memory; the head dims the kernels serve, and a route switched off on purpose, do not warn."""
    import logging
    monkeypatch.setattr(A, "_warned", set())
    x16 = torch.randn(1, 8, 2, 16, device=DEV, dtype=torch.bfloat16)
    x128 = torch.randn(1, 8, 2, 128, device=DEV, dtype=torch.bfloat16)
    with caplog.at_level(logging.WARNING, logger="distributed_llms_example_amd"):
        A.attention(x128, x128, x128)
        A.attention(x128.float(), x128.float(), x128.float())  # fp32 off head dim 64: another reason
        for _ in range(3):
            A.attention(x16, x16, x16)
        monkeypatch.setenv("DLLM_ROUTE", routing.merged(attn_hd=0))
        A.attention(x128, x128, x128)
    msgs = [r.getMessage() for r in caplog.records if r.name == "distributed_llms_example_amd"]
    assert len(msgs) == 2, msgs
    assert "head dim 128" in msgs[0] and "float32" in msgs[0] and "O(Sq*Sk)" in msgs[0]
    assert "head dim 16" in msgs[1] and "O(Sq*Sk)" in msgs[1]
