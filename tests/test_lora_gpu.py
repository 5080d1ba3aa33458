"""LoRA kernels (csrc/lora.hip) through the binding, against fp64 references on EXACT operands (tests/gemm_refs.py),
and the adapted models: native path vs ``DLLM_REFERENCE_OPS=1``, graphed step vs eager step, routing spy.

Exact operands are k/8 values: every product and partial sum is exact in fp32 in any order, so a kernel's only
roundings are the ones its definition states (ops/lora.py) and the fp64 reference, rounded the same way, must match
bit for bit.  ``alpha`` is applied to the fp32 accumulator: where it is a power of two the product is exact; where it
is not (1 / 0.9) the reference multiplies the exact sum by the fp32 value of alpha in fp64 — exactly the correctly
rounded fp32 product once cast to fp32 (``gemm_refs.assert_exact`` casts fp64 -> fp32 -> output type).  The masked
``lora_up`` at p = 0.1 adds that fp32 product to the old value in a second fp32 operation, so it gets the per-element
bound 2^-8 |ref| (the bf16 store) + 2 * 2^-23 * mass (two fp32 roundings of magnitudes <= mass) instead.
"""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

import gemm_refs as R
from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.models import build_model, resolve_config
from distributed_llms_example_amd.ops.rng import rowwise_keep_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
NS = (1, 63, 64, 257, 1000)


def _C():
    return _ext.native()


def _f32(v):
    """The fp32 value of a Python float, as a Python float (what a kernel receives as `float alpha`)."""
    return float(np.float32(v))


@functools.lru_cache(maxsize=None)
def _x(N, K, seed=0):
    """Exact [N, K] operand, shared by the tests on that shape and never modified."""
    return R.dyadic((N, K), DEV, generator=R.gen(DEV, 1000 * seed + 7 * N + K))


@functools.lru_cache(maxsize=None)
def _keep(seed, p, N, K, row0=0):
    return rowwise_keep_mask(seed, p, N, K, DEV, row0=row0)


# ------------------------------------------------------------------------------------------------------- lora_down
DOWN_SHAPES = [(N, K) for N in NS[:-1] for K in (64, 520, 768)] + [(1000, 768)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("r", [1, 8, 16, 24, 64])
def test_lora_down(r, p):
    """t = bf16(alpha * (keep . x) A^T), bit for bit, every (N, K) of the grid, row0 != 0 with dropout."""
    for N, K in DOWN_SHAPES:
        x = _x(N, K)
        A = R.dyadic((r, K), DEV, generator=R.gen(DEV, 31 * r + K))
        assert R.exact_headroom(x, A) < R.EXACT_LIMIT
        row0 = 0 if p == 0.0 else 77 + N
        alpha = 1.0 / (1.0 - p)
        xd = x if p == 0.0 else x * _keep(1234, p, N, K, row0).to(BF16)
        ref = R.gemm_ref(xd, A) * _f32(alpha)
        got = _C().lora_down(x, A, alpha, p, 1234, row0)
        assert got.shape == (N, r) and got.dtype == BF16
        R.assert_exact(got, ref, msg=f"lora_down N={N} K={K} r={r} p={p}")


def test_lora_down_keep_mask_is_rowwise_keep_mask():
    """The decisions themselves: x = 1 and one-hot A rows read 64 columns of keep . x per call; every column of a
    [257, 768] problem at row0 = 12345 equals ``rowwise_keep_mask`` exactly."""
    N, K, p, seed, row0 = 257, 768, 0.1, 99, 12345
    x = torch.ones(N, K, device=DEV, dtype=BF16)
    keep = rowwise_keep_mask(seed, p, N, K, DEV, row0=row0)
    assert 0.05 < 1.0 - keep.float().mean().item() < 0.15
    for k0 in range(0, K, 64):
        A = torch.zeros(64, K, device=DEV, dtype=BF16)
        A[torch.arange(64), k0 + torch.arange(64)] = 1.0
        got = _C().lora_down(x, A, 1.0, p, seed, row0)
        assert torch.equal(got != 0, keep[:, k0:k0 + 64]), k0


def test_lora_down_strided_slice_input():
    """The backward's dt = s * dY[:, c0:c0+n] B: a column slice of a wider matrix as the streamed operand."""
    N, n, r = 257, 64, 8
    dY = _x(N, 3 * n, seed=3)
    Bt = R.dyadic((r, n), DEV, generator=R.gen(DEV, 5))
    for c0 in (0, n, 2 * n):
        got = _C().lora_down(dY[:, c0:c0 + n], Bt, 2.0, 0.0, 0, 0)
        R.assert_exact(got, R.gemm_ref(dY[:, c0:c0 + n], Bt) * 2.0, msg=f"c0={c0}")


# --------------------------------------------------------------------------------------------------------- lora_up
@pytest.mark.parametrize("r", [1, 8, 24, 64])
@pytest.mark.parametrize("n", [64, 768])
def test_lora_up_forward_form(n, r):
    """y[:, c0:c0+n] += alpha * t B^T with one rounding; the columns outside the slice keep their bits."""
    for N in NS:
        t = R.dyadic((N, r), DEV, generator=R.gen(DEV, N + r))
        B = R.dyadic((n, r), DEV, generator=R.gen(DEV, n + r + 1))
        y0 = _x(N, 3 * n, seed=1)
        for c0 in (0, n, 2 * n):
            assert R.exact_headroom(t, B, extra=y0[:, c0:c0 + n]) < R.EXACT_LIMIT
            y = y0.clone()
            _C().lora_up(t, B, False, 2.0, y, c0, n, 0.0, 0, 0)
            ref = R.gemm_ref(t, B) * 2.0 + y0[:, c0:c0 + n].double()
            R.assert_exact(y[:, c0:c0 + n].contiguous(), ref, msg=f"lora_up N={N} n={n} r={r} c0={c0}")
            out = torch.ones(3 * n, dtype=torch.bool, device=DEV)
            out[c0:c0 + n] = False
            assert torch.equal(y[:, out].view(torch.int16), y0[:, out].view(torch.int16)), (N, n, r, c0)


@pytest.mark.parametrize("r", [8, 64])
@pytest.mark.parametrize("p", [0.5, 0.1])
def test_lora_up_masked_dx_form(r, p):
    """dx += keep . (dt A) / (1 - p): M = A [r, K] (k-major), c0 = 0, n = K, the regenerated mask on the update.
    p = 0.5: alpha = 2, exact.  p = 0.1: the module docstring's two-rounding bound."""
    for N, K in ((1, 64), (63, 768), (257, 520), (1000, 768)):
        dt = R.dyadic((N, r), DEV, generator=R.gen(DEV, N + r + 3))
        A = R.dyadic((r, K), DEV, generator=R.gen(DEV, K + r))
        dx0 = _x(N, K, seed=2)
        keep = _keep(555, p, N, K, 9).double()
        alpha = 1.0 / (1.0 - p)
        dx = dx0.clone()
        _C().lora_up(dt, A, True, alpha, dx, 0, K, p, 555, 9)
        upd = R.gemm_ref(dt, A, kmajor=True) * keep
        ref = upd * _f32(alpha) + dx0.double()
        if p == 0.5:
            R.assert_exact(dx, ref, msg=f"masked lora_up N={N} K={K} r={r}")
        else:
            mass = R.gemm_mass(dt, A, kmajor=True) * keep * alpha + dx0.double().abs()
            R.assert_elem_bound(dx, ref, R.BF16_REL * ref.abs() + 2 * R.ACC_U * mass + R.TINY,
                                msg=f"masked lora_up N={N} K={K} r={r} p={p}")
        # an element whose update was dropped keeps its bits
        same = dx.view(torch.int16) == dx0.view(torch.int16)
        assert bool(same[keep == 0].all())


# ------------------------------------------------------------------------------------------------------ lora_wgrad
WG_NS = (1, 257, 4096 + 37)


def test_lora_wgrad_split_constant():
    C = _C()
    rows = C.lora_wgrad_rows
    assert rows % 64 == 0 and C.lora_wgrad_splits(1) == [1, rows]
    assert C.lora_wgrad_splits(2 * rows + 37) == [3, rows]  # more than one split
    assert C.lora_wgrad_splits(WG_NS[-1])[0] == -(-WG_NS[-1] // rows) > 1
    big = rows * C.lora_wgrad_max_splits * 3 + 5
    s, per = C.lora_wgrad_splits(big)
    assert s <= C.lora_wgrad_max_splits and per % 64 == 0 and s * per >= big


@pytest.mark.parametrize("gdtype", [torch.float32, BF16])
@pytest.mark.parametrize("r", [1, 8, 24, 64])
@pytest.mark.parametrize("wide_major", [True, False])
def test_lora_wgrad(wide_major, r, gdtype):
    """G += alpha * W^T S onto a non-zero G (fp32 / bf16), both layouts, a strided W slice, more than one split;
    exact, and two runs bitwise equal."""
    wc = 72 if r == 24 else 768
    for N in WG_NS:
        Wfull = _x(N, wc + 16, seed=4)
        W = Wfull[:, 8:8 + wc]  # a column slice: row stride wc + 16
        S = R.dyadic((N, r), DEV, generator=R.gen(DEV, N + r + 9))
        G0 = R.dyadic((wc, r) if wide_major else (r, wc), DEV, generator=R.gen(DEV, r)).to(gdtype)
        prod = R.wgrad_ref(W, S)  # [wc, r]
        assert R.exact_headroom(W.t(), S.t(), extra=G0 if wide_major else G0.t()) * 2 < R.EXACT_LIMIT
        ref = (prod if wide_major else prod.t()) * 2.0 + G0.double()
        runs = []
        for _ in range(2):
            G = G0.clone()
            _C().lora_wgrad(W, S, 2.0, G, wide_major, True, 0.0, 0, 0)
            runs.append(G)
        R.assert_exact(runs[0], ref, msg=f"lora_wgrad N={N} r={r} wide_major={wide_major} {gdtype}")
        assert torch.equal(runs[0], runs[1])


@pytest.mark.parametrize("p", [0.5, 0.1])
def test_lora_wgrad_masked(p):
    """dA += dt^T (keep . x) / (1 - p): the regenerated mask on the wide operand.  p = 0.5 exact; p = 0.1: the sum is
    exact, alpha * sum and the add are two fp32 roundings."""
    r, K = 8, 520
    for N in WG_NS:
        x, dt = _x(N, K, seed=6), R.dyadic((N, r), DEV, generator=R.gen(DEV, N + 2))
        keep = _keep(777, p, N, K, 3)
        G0 = R.dyadic((r, K), DEV, generator=R.gen(DEV, 1)).float()
        alpha = 1.0 / (1.0 - p)
        G = G0.clone()
        _C().lora_wgrad(x, dt, alpha, G, False, True, p, 777, 3)
        xd = x * keep.to(BF16)
        prod = R.wgrad_ref(xd, dt).t()
        ref = prod * _f32(alpha) + G0.double()
        if p == 0.5:
            R.assert_exact(G, ref, msg=f"masked lora_wgrad N={N}")
        else:
            mass = (xd.double().abs().t() @ dt.double().abs()).t() * alpha + G0.double().abs()
            R.assert_elem_bound(G, ref, 2 * R.ACC_U * mass + R.TINY, msg=f"masked lora_wgrad N={N} p={p}")


def test_lora_wgrad_overwrite():
    G = torch.full((8, 64), 3.0, device=DEV)
    W, S = _x(257, 64, seed=8), R.dyadic((257, 8), DEV, generator=R.gen(DEV, 4))
    _C().lora_wgrad(W, S, 1.0, G, False, False, 0.0, 0, 0)
    R.assert_exact(G, R.wgrad_ref(W, S).t())


# ---------------------------------------------------------------------------------------------------------- rejects
def test_binding_rejects():
    C = _C()
    x = _x(64, 64)
    A = R.dyadic((8, 64), DEV)
    y = _x(64, 192, seed=1).clone()
    t = R.dyadic((64, 8), DEV)
    with pytest.raises(RuntimeError, match="lora_down: x must be a GPU tensor"):
        C.lora_down(x.cpu(), A.cpu(), 1.0, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="lora_down: .*multiples of 8"):
        C.lora_down(_x(64, 68), R.dyadic((8, 68), DEV), 1.0, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="lora_down: x must be 16-byte aligned"):
        C.lora_down(_x(64, 72)[:, 4:68], A, 1.0, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="lora_down: the rank must be 1 .. 64"):
        C.lora_down(x, R.dyadic((65, 64), DEV), 1.0, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="lora_up: the slice"):
        C.lora_up(t, R.dyadic((64, 8), DEV), False, 1.0, y, 4, 64, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="lora_up: the slice"):
        C.lora_up(t, R.dyadic((64, 8), DEV), False, 1.0, y, 136, 64, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="lora_up: M must be"):
        C.lora_up(t, R.dyadic((8, 64), DEV), False, 1.0, y, 0, 64, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="lora_up: y must be a GPU tensor"):
        C.lora_up(t, R.dyadic((64, 8), DEV), False, 1.0, y.cpu(), 0, 64, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="lora_wgrad: the rank must be 1 .. 64"):
        C.lora_wgrad(x, R.dyadic((64, 65), DEV), 1.0, torch.zeros(65, 64, device=DEV), False, True, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="lora_wgrad: G must be"):
        C.lora_wgrad(x, t, 1.0, torch.zeros(64, 8, device=DEV), False, True, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="lora_wgrad: W must be a GPU tensor"):
        C.lora_wgrad(x.cpu(), t.cpu(), 1.0, torch.zeros(8, 64), False, True, 0.0, 0, 0)
    assert torch.equal(y, _x(64, 192, seed=1))  # a rejected call wrote nothing


# ------------------------------------------------------------------------------------------------------ model level
def _cfg(name):
    c = resolve_config(name)
    return c.replace(num_layers=2, num_decoder_layers=2, vocab_size=4096, d_model=512, num_heads=8, d_kv=64, d_ff=1024)


def _batch(cfg, B=2, S=256, T=32):
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, cfg.vocab_size, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    am[1, -33:] = 0
    lab = torch.randint(3, cfg.vocab_size, (B, T), generator=g)
    return {k: v.cuda() for k, v in dict(input_ids=ids, attention_mask=am, labels=lab).items()}


def _adapted(cfg, targets, dropout, sd=None, ab=None):
    from distributed_llms_example_amd.models.lora import LoraConfig, apply_lora
    m = build_model(cfg)
    if sd is not None:
        m.load_state_dict(sd)
    apply_lora(m, LoraConfig(r=8, alpha=16, dropout=dropout, targets=targets))
    if ab is not None:
        m.load_state_dict(ab, strict=False)
    return m


def _random_b(m, seed=3):
    """lora_B away from its zero init (every gradient then carries signal), bf16-representable."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "lora_" in n:
                if "lora_B_" in n:
                    p.copy_(torch.randn(p.shape, generator=g) * 0.05)
                p.copy_(p.to(BF16).float())


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("targets", [("q", "v"), ("q", "k", "v", "o", "wi", "wo")], ids=["qv", "all"])
@pytest.mark.parametrize("name", ["t5-base", "bart-base"])
def test_native_adapters_match_reference(name, targets):
    """bf16 native path (csrc/lora.hip under lora=fused) vs the fp32 ``DLLM_REFERENCE_OPS=1`` composite on the same
    bf16-representable weights and dropout masks: loss within 1 % and every adapter gradient within the bf16 noise
    floor rule of tests/test_model_gpu.py (1.5x the torch-bf16 composite's error, floors 3e-2 / 1e-3)."""
    from distributed_llms_example_amd.ops import lora as lora_op
    from distributed_llms_example_amd.ops.rng import manual_seed
    cfg = _cfg(name)
    torch.manual_seed(0)
    m32 = _adapted(cfg, targets, 0.1)
    _random_b(m32)
    with torch.no_grad():
        for p in m32.parameters():
            p.copy_(p.to(BF16).float())
    sd = m32.state_dict()
    models = {}
    for key in ("ref32", "ref16", "native"):
        m = _adapted(cfg, targets, 0.1)
        m.load_state_dict(sd)
        models[key] = (m.cuda() if key == "ref32" else m.cuda().to(BF16)).train()
    b = _batch(cfg)
    loss = {}
    with _env(DLLM_REFERENCE_OPS="1"):
        for key in ("ref32", "ref16"):
            manual_seed(5)
            out = models[key](**b)
            out.loss.backward()
            loss[key] = out.loss.item()
    before = lora_op.fused_calls
    manual_seed(5)
    out = models["native"](**b)
    out.loss.backward()
    assert lora_op.fused_calls > before
    assert abs(out.loss.item() - loss["ref32"]) < 0.01 * loss["ref32"], (out.loss.item(), loss)

    def report(mt):
        rep = {}
        for (n, pt), (_, pr) in zip(mt.named_parameters(), models["ref32"].named_parameters()):
            if "lora_" not in n:
                assert pt.grad is None, n
                continue
            gt, gr = pt.grad.float().flatten(), pr.grad.float().flatten()
            assert gr.norm() > 0, n
            rep[n] = (((gt - gr).norm() / gr.norm()).item(),
                      torch.nn.functional.cosine_similarity(gt, gr, dim=0).item())
        return rep

    rep, floor = report(models["native"]), report(models["ref16"])
    assert len(rep) == 2 * sum(len(m._lora[0]) for m in models["native"].modules() if getattr(m, "_lora", None))
    bad = [(n, rel, floor[n]) for n, (rel, cos) in rep.items()
           if rel > max(3e-2, 1.5 * floor[n][0]) or 1 - cos > max(1e-3, 1.5 * (1 - floor[n][1]))]
    print(f"[lora parity {name} {targets}] worst rel {max(v[0] for v in rep.values()):.4f} "
          f"(torch-bf16 floor {max(v[0] for v in floor.values()):.4f})")
    assert not bad, bad[:5]


@pytest.mark.parametrize("name", ["t5-base", "bart-base"])
def test_route_spy(name, monkeypatch):
    """Under lora=fused every adapted linear's forward and backward reach the binding (csrc/lora.hip); under lora=lib
    none does — and both give the same loss."""
    from distributed_llms_example_amd.ops import routing
    from distributed_llms_example_amd.ops.rng import manual_seed
    C = _C()
    calls = {"lora_down": 0, "lora_up": 0, "lora_wgrad": 0}
    for fn in calls:
        real = getattr(C, fn)

        def spy(*a, _fn=fn, _real=real, **kw):
            calls[_fn] += 1
            return _real(*a, **kw)

        monkeypatch.setattr(C, fn, spy)
    cfg = _cfg(name)
    torch.manual_seed(0)
    m = _adapted(cfg, ("q", "v"), 0.1)
    _random_b(m)
    m = m.cuda().to(BF16).train()
    n_adapters = sum(len(x._lora[0]) for x in m.modules() if getattr(x, "_lora", None))
    b = _batch(cfg)
    losses = {}
    for route in ("fused", "lib"):
        monkeypatch.setenv("DLLM_ROUTE", routing.merged(lora=route))
        for k in calls:
            calls[k] = 0
        manual_seed(5)
        out = m(**b)
        out.loss.backward()
        losses[route] = out.loss.item()
        if route == "fused":
            # per adapter: down (forward) + down (dt); up (forward) + up (dx); two weight gradients.  The first
            # adapted layer of each stack has no input gradient (frozen embeddings): one lora_up less per adapter there
            assert calls["lora_down"] == 2 * n_adapters, calls
            assert calls["lora_wgrad"] == 2 * n_adapters, calls
            assert 2 * n_adapters - 4 <= calls["lora_up"] <= 2 * n_adapters, calls
        else:
            assert calls == {"lora_down": 0, "lora_up": 0, "lora_wgrad": 0}, calls
    assert abs(losses["fused"] - losses["lib"]) < 2e-3 * abs(losses["lib"]), losses


def test_graphed_adapter_step_matches_eager():
    """A HIP-graph step with adapters (train/graph.py) replays to the same losses and parameters as the eager steps:
    the op synchronises nothing and takes no data-dependent shape."""
    from distributed_llms_example_amd.ops import rng as rng_mod
    from distributed_llms_example_amd.ops.rng import manual_seed
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    from distributed_llms_example_amd.train.graph import GraphedStep
    env = init_distributed()
    cfg = _cfg("t5-base")
    torch.manual_seed(0)
    proto = _adapted(cfg, ("q", "v"), 0.1)
    _random_b(proto)
    sd = proto.state_dict()
    g = torch.Generator().manual_seed(3)
    data = [{"input_ids": torch.randint(3, cfg.vocab_size, (2, 256), generator=g).cuda(),
             "attention_mask": torch.ones(2, 256, dtype=torch.long).cuda(),
             "labels": torch.randint(3, cfg.vocab_size, (2, 32), generator=g).cuda()} for _ in range(5)]
    steps = 3

    def engine():
        m = _adapted(cfg, ("q", "v"), 0.1)
        m.load_state_dict(sd)
        manual_seed(11)
        e = TrainEngine(m, env, lr=1e-3, dtype=BF16)
        e.train()
        assert all("lora_" in s.name for s in e.flat.segments)
        return e

    try:
        eg = engine()
        gs = GraphedStep(eg, data[:1], warmup=2)
        lg = [float(gs.replay(data[2 + i:3 + i])) for i in range(steps)]
        pg = eg.flat.to_canonical(eg.flat.param_buf).float().clone()
        eg.disable_step_seeds()

        ee = engine()
        ee.enable_step_seeds()
        t = torch.zeros((), dtype=torch.float32, device="cuda")
        le = []
        for i in range(steps + 2):
            loss = float(ee.forward_backward(data[0] if i < 2 else data[i]))
            t.add_(1.0)
            ee.step(hyper=ee.optimizer.device_hyper(t, ee.optimizer.param_groups[0]["lr"]))
            if i >= 2:
                le.append(loss)
        pe = ee.flat.to_canonical(ee.flat.param_buf).float().clone()
        ee.disable_step_seeds()
    finally:
        st = rng_mod._active_step[0]
        if st is not None:
            st.disable()
        rng_mod.default_rng().site_mode = False
    assert lg == pytest.approx(le, rel=1e-3), (lg, le)
    assert ((pg - pe).norm() / pe.norm()).item() < 1e-3


@pytest.mark.parametrize("name", ["t5-base", "flan-t5-base", "bart-base"])
def test_frozen_ffn_stays_on_the_fused_kernels(name, monkeypatch):
    """Adapters on q, v only: the frozen FFNs (ReLU, gated GELU, GELU) keep their fused epilogue kernels — forward and
    input gradient, no weight gradient — and give the loss and adapter gradients of the unfused route, each measured
    against the fp32 reference on the same masks (the fused route within 1.5x of the unfused one's error, floor 3e-2)."""
    from distributed_llms_example_amd.ops import ffn as ffn_mod, routing
    from distributed_llms_example_amd.ops.rng import manual_seed
    cfg = _cfg(name)
    torch.manual_seed(0)
    m32 = _adapted(cfg, ("q", "v"), 0.1)
    _random_b(m32)
    with torch.no_grad():
        for p in m32.parameters():
            p.copy_(p.to(BF16).float())
    sd = m32.state_dict()
    m32 = m32.cuda().train()
    b = _batch(cfg, B=4, S=512, T=64)  # 2048 encoder rows: past ffn_min_rows, a multiple of 256

    def run(m):
        manual_seed(5)
        out = m(**b)
        out.loss.backward()
        return out.loss.item(), {n: p.grad.float().flatten() for n, p in m.named_parameters() if p.grad is not None}

    with _env(DLLM_REFERENCE_OPS="1"):
        l32, g32 = run(m32)
    res = {}
    for route in ("fused", "unfused"):
        m = _adapted(cfg, ("q", "v"), 0.1)
        m.load_state_dict(sd)
        m = m.cuda().to(BF16).train()
        monkeypatch.setenv("DLLM_ROUTE", routing.merged(ffn=route, gated_min_mf=0))
        before = ffn_mod.fused_calls + ffn_mod.gated_calls
        res[route] = run(m)
        ran = ffn_mod.fused_calls + ffn_mod.gated_calls - before
        assert (ran >= cfg.num_layers) if route == "fused" else ran == 0, (route, ran)
        assert all("lora_" in n for n in res[route][1])
    for route in res:
        assert abs(res[route][0] - l32) < 0.01 * l32, (route, res[route][0], l32)
    rel = {r: {n: ((g - g32[n]).norm() / g32[n].norm()).item() for n, g in res[r][1].items()} for r in res}
    bad = [(n, v, rel["unfused"][n]) for n, v in rel["fused"].items() if v > max(3e-2, 1.5 * rel["unfused"][n])]
    print(f"[frozen ffn {name}] worst rel fused {max(rel['fused'].values()):.4f} unfused "
          f"{max(rel['unfused'].values()):.4f}")
    assert not bad, bad[:5]
