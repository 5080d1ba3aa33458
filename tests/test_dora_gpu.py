"""DoRA kernels of csrc/lora.hip against fp64 statements (the rescale and the gradient pass on EXACT operands, gemm_refs
``dyadic``: multiples of 1/512 far below 2^24, so bit for bit), and ``lora_linear`` with DoRA vs the fp32 composite."""
import pytest
import torch

import gemm_refs as R
from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops import lora as lora_op, routing
from distributed_llms_example_amd.ops.linear import Linear
from distributed_llms_example_amd.ops.lora import Adapter, lora_linear
from distributed_llms_example_amd.ops.rng import manual_seed

pytestmark = pytest.mark.gpu
DEV, BF16, NS = "cuda", torch.bfloat16, (1, 63, 257)


def _real(shape, seed, std=1.0):
    return (torch.randn(shape, device=DEV, generator=R.gen(DEV, seed)) * std).to(BF16)


@pytest.mark.parametrize("r", [1, 8, 24, 64])
@pytest.mark.parametrize("n,K,c0", [(8, 64, 0), (24, 72, 0), (64, 520, 0), (768, 768, 0), (64, 520, 128)])
def test_dora_norm(n, K, c0, r):
    """norm, c = m / norm vs fp64 of the same bf16 operands (c0 > 0: rows of a 3n-row weight): |norm - ref| <= (K + r +
    8) 2^-23 ref_abs, ref_abs the fp64 norm of |W| + s |B||A| (K + r fp32 additions; 8: products, lane sums, root)."""
    C, s = _ext.native(), 1.75
    W = _real((3 * n if c0 else n, K), 11 * n + K, 0.05)
    A, B, m = _real((r, K), r + K, 0.05), _real((n, r), n + r, 0.5), _real((n,), n).abs() + 0.5
    Ws = W[c0:c0 + n].double()
    ref = torch.linalg.vector_norm(Ws + s * B.double() @ A.double(), dim=1)
    ref_abs = torch.linalg.vector_norm(Ws.abs() + s * B.double().abs() @ A.double().abs(), dim=1)
    c = torch.full((n,), -1.0, device=DEV)
    norm = C.dora_norm(W, c0, A, B, s, m, c)
    bound = (K + r + 8) * R.ACC_U * ref_abs
    worst = R.assert_elem_bound(norm[None], ref[None], bound[None], msg=f"dora_norm n={n} K={K} r={r} c0={c0}")
    print(f"[dora_norm n={n} K={K} r={r} c0={c0}] worst |err| / bound {worst:.4f}")
    cref = m.double() / ref
    R.assert_elem_bound(c[None], cref[None], (bound / ref + 2 * R.ACC_U)[None] * cref, msg="c = m / norm")


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("n", [64, 768])
def test_rescaling_lora_up_and_dora_bwd(n, bias):
    """An [N, 2n] layer, slice 1 (c0 = n) with a DoRA adapter.  lora_up: y_s = c . ((y_s - b_s) + alpha t B^T) + b_s bit
    for bit, slice 0 keeps its bits.  dora_bwd: dY' = c_full . dY bit for bit; dm into a non-zero fp32 / bf16 sink in
    (rows + splits + 2) 2^-23 of sum |dY||y - b| / m (``rows`` fp32 additions per split, ``splits`` more, division, add)
    plus a bf16 sink's store; the last N takes several splits; two runs give the same bits."""
    C = _ext.native()
    rows = C.lora_wgrad_rows
    for N in NS + ((2 * rows + 37,) if n == 64 else ()):
        g = R.gen(DEV, 3 * N + n)
        y0, dy = R.dyadic((N, 2 * n), DEV, generator=g), R.dyadic((N, 2 * n), DEV, generator=g)
        c = R.dyadic((n,), DEV, generator=g).float()
        b = R.dyadic((2 * n,), DEV, generator=g) if bias else None
        bs = torch.zeros(n, device=DEV).double() if b is None else b[n:].double()
        for r in (8, 40):
            t, B = R.dyadic((N, r), DEV, generator=g), R.dyadic((n, r), DEV, generator=g)
            mass = c.abs().double() * (R.gemm_mass(t, B) * 2.0 + y0[:, n:].double().abs() + bs.abs()) + bs.abs()
            assert 512.0 * mass.max().item() < R.EXACT_LIMIT
            y = y0.clone()
            C.lora_up(t, B, False, 2.0, y, n, n, 0.0, 0, 0, c, None if b is None else b[n:])
            ref = c.double() * ((y0[:, n:].double() - bs) + R.gemm_ref(t, B) * 2.0) + bs
            R.assert_exact(y[:, n:].contiguous(), ref, msg=f"rescaling lora_up N={N} n={n} r={r}")
            assert torch.equal(y[:, :n].view(torch.int16), y0[:, :n].view(torch.int16))
        c_full = torch.cat([torch.ones(n, device=DEV), c])
        live = torch.cat([torch.zeros(n // 8), torch.ones(n // 8)]).to(torch.uint8).to(DEV)
        m = _real((n,), n + 1).abs() + 0.5
        out, part = C.dora_bwd(dy, y0, c_full, live, b)
        splits = C.lora_wgrad_splits(N)[0]
        assert part.shape == (splits, 2 * n) and not part[:, :n].any()
        R.assert_exact(out, c_full.double() * dy.double(), msg=f"dora_bwd dY' N={N} n={n}")
        ref = (dy[:, n:].double() * (y0[:, n:].double() - bs)).sum(0) / m.double()
        mass = (dy[:, n:].double() * (y0[:, n:].double() - bs)).abs().sum(0) / m.double()
        for dt in (torch.float32, BF16):
            g0 = R.dyadic((n,), DEV, generator=g).to(dt)
            sink = g0.clone()
            C.dora_dm(part, n, m, sink)
            want = ref + g0.double()
            bound = (min(rows, N) + splits + 2) * R.ACC_U * (mass + g0.double().abs()) + R.TINY
            bound = bound + (R.BF16_REL * want.abs() if dt == BF16 else 0.0)
            R.assert_elem_bound(sink[None], want[None], bound[None], msg=f"dm N={N} n={n} {dt}")
        assert all(torch.equal(u, v) for u, v in zip((out, part), C.dora_bwd(dy, y0, c_full, live, b)))


def _adapted_linear(dtype, K=256, n=128, r=8):
    """A frozen q|k|v layer with a bias; q and v carry DoRA adapters (k none): bf16-representable values."""
    torch.manual_seed(0)
    lin = Linear(K, 3 * n, bias=True).requires_grad_(False)
    torch.nn.init.normal_(lin.bias, std=0.5)
    for i in (0, 2):
        m = torch.linalg.vector_norm(lin.weight[i * n:(i + 1) * n], dim=1) * (1.0 + 0.2 * torch.rand(n))
        for name, v in (("A", torch.randn(r, K) * K ** -0.5), ("B", torch.randn(n, r) * 0.05), ("m", m)):
            lin.register_parameter(f"lora_{name}_{i}", torch.nn.Parameter(v.to(BF16).float()))
    lin.weight.copy_(lin.weight.to(BF16).float())
    lin.bias.copy_(lin.bias.to(BF16).float())
    lin = lin.to(DEV, dtype)
    return lin, [Adapter("qkv"[i], i * n, n, getattr(lin, f"lora_A_{i}"), getattr(lin, f"lora_B_{i}"), 2.0,
                         getattr(lin, f"lora_m_{i}")) for i in (0, 2)]


def _run(dtype, p, x, gy):
    lin, ads = _adapted_linear(dtype)
    xx = x.to(dtype).clone().requires_grad_(True)
    manual_seed(5)
    y = lora_linear(xx, lin, ads, p, 77)
    y.backward(gy.to(dtype))
    out = dict({"y": y.detach(), "dx": xx.grad}, **{n: q.grad for n, q in lin.named_parameters() if "lora_" in n})
    return {k: v.float().flatten() for k, v in out.items()}


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("route", ["fused", "lib"])
def test_lora_linear_dora(route, p, monkeypatch):
    """Output and every gradient (x; A, B, m of both adapters) on each route vs the fp32 composite, by the rule of
    test_lora_gpu.py test_native_adapters_match_reference (1.5x the torch-bf16 composite's error, floors 3e-2, 1e-3)."""
    x, gy = _real((2, 128, 256), 1).float(), _real((2, 128, 384), 2).float()
    monkeypatch.setenv("DLLM_REFERENCE_OPS", "1")
    ref32, ref16 = _run(torch.float32, p, x, gy), _run(BF16, p, x, gy)
    monkeypatch.delenv("DLLM_REFERENCE_OPS")
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(lora=route))
    before = (lora_op.fused_calls, lora_op.lib_calls)
    got = _run(BF16, p, x, gy)
    assert ((lora_op.fused_calls > before[0]), (lora_op.lib_calls > before[1])) == (route == "fused", route == "lib")
    assert len(got) == 8

    def err(a):
        return {k: (((a[k] - ref32[k]).norm() / ref32[k].norm()).item(),
                    torch.nn.functional.cosine_similarity(a[k], ref32[k], dim=0).item()) for k in ref32}

    rep, floor = err(got), err(ref16)
    print(f"[dora {route} p={p}] " + " ".join(f"{k} {v[0]:.4f}/{floor[k][0]:.4f}" for k, v in rep.items()))
    bad = [(k, v, floor[k]) for k, v in rep.items()
           if v[0] > max(3e-2, 1.5 * floor[k][0]) or 1 - v[1] > max(1e-3, 1.5 * (1 - floor[k][1]))]
    assert not bad, bad


def test_cached_scale_under_no_grad(monkeypatch):
    """Two no_grad forwards run dora_norm once per adapter; an in-place update of B runs it again."""
    C, calls = _ext.native(), []
    real = C.dora_norm
    monkeypatch.setattr(C, "dora_norm", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(lora="fused"))
    lin, ads = _adapted_linear(BF16)
    x = _real((64, 256), 3)
    with torch.no_grad():
        y1, y2 = lora_linear(x, lin, ads), lora_linear(x, lin, ads)
        assert len(calls) == 2 and torch.equal(y1, y2)
        ads[1].B.mul_(2.0)
        y3 = lora_linear(x, lin, ads)
    assert len(calls) == 4 and not torch.equal(y3[:, 256:], y1[:, 256:]) and torch.equal(y3[:, :256], y1[:, :256])
