"""csrc/adafactor.hip and FusedAdafactor on the GPU, against the fp64 recurrence of tests/adafactor_refs.py.

The kernel test runs ONE flat buffer holding every unit of ``SPECS`` for three consecutive steps with fresh gradients
and a clip coefficient other than 1 read from device memory.  The last row and the last column of every unit's gradient
are scaled x30: a missed row, a missed column or a slice boundary off by one then moves a statistic by more than 1e-2,
far from any rounding bound.

Bounds (each figure is printed before it is asserted; run with -s to collect them):

* ``R``, ``C``, ``V``: elementwise relative error <= (L + 8) * 2^-23, capped at 1e-4.  ``L`` is the kernel's longest
  sequential fp32 addition chain for the unit's shape, from the geometry constants the extension exports
  (``adafactor_geometry``): for ``C`` the AF_RB rows a lane adds up inside a tile, then ceil(row blocks / AF_FIN_SLICES)
  partials per slice, 2 shuffle steps and 3 additions over the 4 waves; for ``R`` 4 elements per lane, a 6-step wave
  tree, 3 additions over the 4 waves, then the column chunks in order; ``V`` has no sum.  Every term is positive, so
  nothing cancels; the 8 covers the roundings outside the sums (coef * g, the square, the mean's division, the blend).
* the update ``D = w_new - w_old`` of the master: ``|D - Dref| <= 1e-4 * (|Dref| + rms(Dref))``.  Rounding the master is
  2^-24 |w| against |D| ~ lr = 1e-2, and the statistics' error halves through the rsqrt: about 2e-5 together.
* bf16 parameters: exactly the round-to-nearest-even of the master.
"""
import math

import pytest
import torch

import adafactor_refs as A
from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops import routing
from distributed_llms_example_amd.ops.optim import FusedAdafactor
from distributed_llms_example_amd.parallel.flat import FlatParams

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, COEF, WD = 1e-2, 0.37, 0.1
EPS1, EPS2, CLIP, DECAY_RATE = 1e-30, 1e-3, 1.0, -0.8
UPDATE_BOUND = 1e-4


def _geom():
    rb, wc, cc, cap, slices, fcols = _ext.native().adafactor_geometry()
    return {"RB": rb, "WC": wc, "CC": cc, "CAP": cap, "SLICES": slices}


def _second_wave_rows():
    """Rows of the [rows, 64] unit whose tiles alone exceed one resident wave: a tile is AF_RB rows x AF_CC (>= 64)
    columns, a tile pass launches at most AF_GRID_CAP workgroups (256 CUs x 8 resident 256-thread workgroups), each
    striding over the tiles; with more than AF_GRID_CAP row blocks some workgroups take a second tile.  The 40 extra rows
    are no multiple of AF_RB, so the last row block is ragged."""
    g = _geom()
    return g["RB"] * g["CAP"] + 40


def _specs():
    return [((64, 64), 1, "min"), ((72, 200), 1, "cols%64"), ((32, 6), 1, "scalar"), ((32, 12), 1, "scalar12"),
            ((4100, 96), 1, "rowblocks"), ((96, 4100), 1, "wide"), ((3 * 64, 128), 3, "qkv"), ((2 * 96, 64), 2, "kv"),
            ((768,), 1, "1d"), ((100,), 1, "1d"), ((3 * 64,), 3, "1dqkv"), ((512, 64), 1, "zerorows"),
            ((128, 64), 1, "zerounit"), ((_second_wave_rows(), 64), 1, "wave2")]


def _chains(u, g):
    """Longest sequential fp32 addition chains (L of the module docstring) of unit ``u`` for R / C."""
    nrb = -(-u.rows // g["RB"])
    nchunk = -(-u.cols // g["CC"])
    return 4 + 6 + 3 + nchunk, min(u.rows, g["RB"]) + -(-nrb // g["SLICES"]) + 2 + 3


def _stat_bound(L):
    return min((L + 8) * 2.0 ** -23, 1e-4)


def _grads(units, n, step, scale):
    """Fresh fp32 gradients of one step on the CPU: N(0, scale^2), the last row and column of every unit x30, all-zero
    rows / units where the tag asks for them."""
    gen = torch.Generator().manual_seed(100 + step)
    g = torch.zeros(n)
    for u in units:
        x = torch.randn(u.shape, generator=gen) * scale
        if u.factored:
            x[-1, :] *= 30
            x[:, -1] *= 30
        else:
            x[-1] *= 30
        if "zerorows" in u.tag:
            keep = torch.zeros(u.rows, dtype=torch.bool)
            keep[[0, 7, 100, 333, 511]] = True
            x[~keep] = 0
        if "zerounit" in u.tag:
            x.zero_()
        g[u.off:u.off + u.numel] = x.reshape(-1)
    return g


class Kernel:
    """The buffers of one direct run of ``adafactor_step`` over ``units`` (bf16 parameters + fp32 master, or fp32)."""

    def __init__(self, units, n, w, bf16=True):
        C = _ext.native()
        self.units, self.n = units, n
        rv = c = 0
        rows = []
        self.rv_off, self.c_off = [], []
        for u in units:
            rows.append([u.off, u.rows, u.cols, rv, c if u.factored else -1, int(u.decay)])
            self.rv_off.append(rv)
            self.c_off.append(c if u.factored else -1)
            rv += ((u.rows if u.factored else u.cols) + 3) // 4 * 4
            if u.factored:
                c += (u.cols + 3) // 4 * 4
        self.host, self.n_tiles, colpart, rowpart = C.adafactor_plan(torch.tensor(rows, dtype=torch.int64))
        z = lambda k: torch.zeros(max(k, 4), dtype=torch.float32, device=DEV)
        self.table = self.host.to(DEV)
        self.rv, self.c = z(rv), z(c)
        self.scratch = [z(4 * len(units)), z(colpart), z(rowpart), z(2 * self.n_tiles)]
        self.master = w.to(DEV).float().clone() if bf16 else None
        self.param = w.to(DEV).to(torch.bfloat16 if bf16 else torch.float32).clone()
        self.coef = torch.tensor(COEF, dtype=torch.float32, device=DEV)

    def weights(self):
        return self.master if self.master is not None else self.param

    def clone_state(self):
        return [t.clone() if t is not None else None for t in (self.param, self.master, self.rv, self.c)]

    def set_state(self, st):
        for dst, src in zip((self.param, self.master, self.rv, self.c), st):
            if dst is not None:
                dst.copy_(src)

    def step(self, grad, rel, beta2t, wd=0.0, sp=False, hyper=None):
        _ext.native().adafactor_step(self.param, self.master, grad, self.rv, self.c, self.table, self.host,
                                     *self.scratch, self.coef, rel, beta2t, EPS1, EPS2, CLIP, wd, sp, hyper)

    def stat(self, i, kind):
        u = self.units[i]
        if kind == "C":
            return self.c[self.c_off[i]:self.c_off[i] + u.cols]
        return self.rv[self.rv_off[i]:self.rv_off[i] + (u.rows if kind == "R" else u.cols)]


def _check_step(tag, k, ref, deltas, w_before, geom, bad):
    """Statistics, update and bf16 parameters of every unit after one step; appends failures to ``bad``."""
    worst = {"R": (0.0, 1.0, ""), "C": (0.0, 1.0, ""), "V": (0.0, 1.0, ""), "D": (0.0, 1.0, "")}

    def note(kind, err, bound, name):
        if err / bound >= worst[kind][0] / worst[kind][1]:
            worst[kind] = (err, bound, name)
        if not err <= bound:
            bad.append(f"{tag} {name} {kind}: err {err:.3e} bound {bound:.3e}")

    w_after = k.weights().double().cpu()
    assert torch.isfinite(w_after).all(), f"{tag}: non-finite weights"
    for i, u in enumerate(k.units):
        if u.factored:
            LR_, LC_ = _chains(u, geom)
            note("R", A.rel_err(k.stat(i, "R"), ref.R[i]), _stat_bound(LR_), u.tag)
            note("C", A.rel_err(k.stat(i, "C"), ref.C[i]), _stat_bound(LC_), u.tag)
        else:
            note("V", A.rel_err(k.stat(i, "V"), ref.V[i]), _stat_bound(0), u.tag)
        d = (w_after[u.off:u.off + u.numel] - w_before[u.off:u.off + u.numel]).view(u.shape)
        dref = deltas[i]
        rms = float(dref.pow(2).mean().sqrt())
        tol = UPDATE_BOUND * (dref.abs() + rms)
        excess = (d - dref).abs() - tol
        j = int(excess.argmax())
        e, t = float((d - dref).abs().reshape(-1)[j]), float(tol.reshape(-1)[j])
        if t == 0.0:  # an all-zero unit without decay: the update is exactly zero
            if e != 0.0:
                bad.append(f"{tag} {u.tag} D: {e:.3e} where the reference update is 0")
        else:
            note("D", e, t, u.tag)
    for kind, (e, b, name) in worst.items():
        print(f"[fig] {tag} {kind}: worst err {e:.3e} bound {b:.3e} (ratio {e / b:.2f}) at {name}")
        if e > b / 2:
            print(f"[fig] {tag} {kind}: above half its bound")
    if k.master is not None:
        if not torch.equal(k.param, k.master.to(torch.bfloat16)):
            bad.append(f"{tag}: bf16 parameters are not the rounded master")


@pytest.fixture(scope="module")
def world():
    units, n = A.layout(_specs())
    gen = torch.Generator().manual_seed(1)
    w = (torch.rand(n, generator=gen) * 2 - 1) * 0.5
    # gradient scales that do not fall from step to step: the update bound's derivation takes |D| ~ lr, which holds
    # while the fresh gradient is not small against the history in R / C / V (a gradient 10x smaller than the last one
    # gives |D| ~ lr / 10, and the master's own rounding, 2^-24 |w|, then is no longer small against 1e-4 |D|)
    grads = [_grads(units, n, s, sc) for s, sc in ((1, 1e-2), (2, 2e-2), (3, 3e-2))]
    return units, n, w, grads


@pytest.mark.parametrize("mode", ["plain", "scale_parameter", "weight_decay", "fp32_params"])
def test_adafactor_step_direct(world, mode):
    """Three consecutive steps of every unit of ``SPECS`` in one flat buffer against the free-running fp64 recurrence.
    ``weight_decay`` decays every second unit; ``fp32_params`` updates fp32 parameters in place without a master."""
    units, n, w, grads = world
    sp, wd = mode == "scale_parameter", WD if mode == "weight_decay" else 0.0
    for i, u in enumerate(units):
        u.decay = mode == "weight_decay" and i % 2 == 0
    geom = _geom()
    k = Kernel(units, n, w, bf16=mode != "fp32_params")
    assert k.n_tiles > geom["CAP"], "the layout must not fit one resident wave of workgroups"
    ref = A.RefState(units, k.weights())
    bad = []
    for t, g in enumerate(grads, start=1):
        b2t = 1.0 - math.pow(t, DECAY_RATE)
        w_before = k.weights().double().cpu()
        k.step(g.to(DEV), LR, b2t, wd=wd, sp=sp)
        deltas = ref.step(g, COEF, LR, b2t, EPS1, EPS2, CLIP, wd, sp)
        _check_step(f"{mode} t={t}", k, ref, deltas, w_before, geom, bad)
    zi = next(i for i, u in enumerate(units) if "zerounit" in u.tag)
    if not units[zi].decay:
        u = units[zi]
        assert torch.equal(k.weights()[u.off:u.off + u.numel].cpu(),
                           (w if k.master is not None else w.float())[u.off:u.off + u.numel])
    assert not bad, "\n".join(bad)


def test_deterministic_and_hyper_tensor(world):
    """The same step twice from cloned state is equal bit for bit; a hyper tensor with the host's values reproduces the
    host-scalar call bit for bit; ``device_hyper`` (fp32 pow on the device) stays within the fp64 bounds."""
    units, n, w, grads = world
    for u in units:
        u.decay = False
    geom = _geom()
    k = Kernel(units, n, w)
    g1, g2 = grads[0].to(DEV), grads[1].to(DEV)
    k.step(g1, LR, 0.0, sp=True)
    start = k.clone_state()
    b2t = 1.0 - math.pow(2, DECAY_RATE)
    k.step(g2, LR, b2t, sp=True)
    first = k.clone_state()
    k.set_state(start)
    k.step(g2, LR, b2t, sp=True)
    for a, b in zip(first, k.clone_state()):
        assert torch.equal(a, b)
    k.set_state(start)
    k.step(g2, 123.0, 0.5, sp=True, hyper=torch.tensor([LR, b2t], dtype=torch.float32, device=DEV))
    for a, b in zip(first, k.clone_state()):
        assert torch.equal(a, b)
    # device_hyper: rel = lr, beta2t = 1 - t^-0.8 in fp32 on the device
    opt = FusedAdafactor.__new__(FusedAdafactor)
    opt.decay_rate, opt.relative_step, opt.warmup_init = DECAY_RATE, False, False
    dh = FusedAdafactor.device_hyper(opt, torch.full((), 2.0, device=DEV), LR)
    assert dh.shape == (2,) and dh.dtype == torch.float32
    assert abs(float(dh[1]) - b2t) < 4 * 2.0 ** -24 and float(dh[0]) == A.f32(LR)
    k.set_state(start)
    ref = A.RefState(units, k.weights())
    for i, u in enumerate(units):  # the reference continues from the kernel's state after step 1
        if u.factored:
            ref.R[i], ref.C[i] = k.stat(i, "R").double().cpu(), k.stat(i, "C").double().cpu()
        else:
            ref.V[i] = k.stat(i, "V").double().cpu()
    w_before = k.weights().double().cpu()
    k.step(g2, 123.0, 0.5, sp=True, hyper=dh)
    deltas = ref.step(grads[1], COEF, float(dh[0]), float(dh[1]), EPS1, EPS2, CLIP, 0.0, True)
    bad = []
    _check_step("device_hyper", k, ref, deltas, w_before, geom, bad)
    assert not bad, "\n".join(bad)


def test_large_offsets():
    """One [64, 64] unit at flat element offset 2^31 + 64: every index is 64-bit.  The buffers are ``torch.empty``; only
    the unit's region is initialised and read."""
    free, _ = torch.cuda.mem_get_info()
    if free < 40 * 2 ** 30:
        pytest.skip("needs 40 GB of free device memory")
    off = 2 ** 31 + 64
    n = off + 4096
    u = A.Unit(off, 64, 64, True, tag="far")
    gen = torch.Generator().manual_seed(3)
    w = torch.rand(4096, generator=gen) - 0.5
    g = torch.randn(4096, generator=gen) * 1e-2
    C = _ext.native()
    host, n_tiles, colpart, rowpart = C.adafactor_plan(torch.tensor([[off, 64, 64, 0, 0, 0]], dtype=torch.int64))
    z = lambda k: torch.zeros(max(k, 4), dtype=torch.float32, device=DEV)
    param = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    master = torch.empty(n, dtype=torch.float32, device=DEV)
    grad = torch.empty(n, dtype=torch.float32, device=DEV)
    master[off:] = w.to(DEV)
    param[off:] = w.to(DEV).to(torch.bfloat16)
    grad[off:] = g.to(DEV)
    guard = master[off - 64:off].clone()
    rv, c = z(64), z(64)
    coef = torch.tensor(COEF, dtype=torch.float32, device=DEV)
    C.adafactor_step(param, master, grad, rv, c, host.to(DEV), host, z(4), z(colpart), z(rowpart), z(2 * n_tiles), coef,
                     LR, 0.0, EPS1, EPS2, CLIP, 0.0, False, None)
    near = A.Unit(0, 64, 64, True)
    ref = A.RefState([near], w)
    w0 = w.double()
    (dref,) = ref.step(g, COEF, LR, 0.0)
    d = (master[off:].double().cpu() - w0).view(64, 64)
    rms = float(dref.pow(2).mean().sqrt())
    assert rms > 1e-3
    assert bool(((d - dref).abs() <= UPDATE_BOUND * (dref.abs() + rms)).all())
    assert torch.equal(param[off:], master[off:].to(torch.bfloat16))
    assert torch.equal(master[off - 64:off], guard)
    LR_, LC_ = _chains(near, _geom())
    assert A.rel_err(rv, ref.R[0]) < _stat_bound(LR_) and A.rel_err(c, ref.C[0]) < _stat_bound(LC_)


def test_binding_rejects_strided_and_misaligned():
    units, n = A.layout([((64, 64), 1, "a"), ((128,), 1, "b")])
    k = Kernel(units, n, torch.zeros(n))
    g = torch.zeros(n, device=DEV)
    k.step(g, LR, 0.0)  # aligned, contiguous buffers pass
    big = torch.zeros(2 * n + 8, device=DEV)
    ok_master = k.master
    with pytest.raises(RuntimeError, match="aligned"):
        k.master = big[1:n + 1]
        k.step(g, LR, 0.0)
    with pytest.raises(RuntimeError, match="contiguous"):
        k.master = big[:2 * n:2]
        k.step(g, LR, 0.0)
    k.master = ok_master
    with pytest.raises(RuntimeError, match="aligned"):
        k.step(big[1:n + 1], LR, 0.0)
    with pytest.raises(RuntimeError, match="contiguous"):
        k.step(big[:2 * n:2], LR, 0.0)
    with pytest.raises(RuntimeError, match="fp32"):
        k.step(g.to(torch.bfloat16), LR, 0.0)
    ok_rv = k.rv
    with pytest.raises(RuntimeError, match="aligned"):
        k.rv = torch.zeros(ok_rv.numel() + 4, device=DEV)[1:ok_rv.numel() + 1]
        k.step(g, LR, 0.0)
    with pytest.raises(RuntimeError, match="outside its buffer"):
        k.rv = torch.zeros(ok_rv.numel() - 4, device=DEV)
        k.step(g, LR, 0.0)
    k.rv = ok_rv
    with pytest.raises(RuntimeError, match="outside the flat buffer"):
        bad = k.host.clone()
        bad[1, 0] = n  # the second unit starts at the end of the buffer
        k.host = bad
        k.step(g, LR, 0.0)


# ------------------------------------------------------------------------------------------------ FusedAdafactor
def _small_t5():
    from distributed_llms_example_amd.models import build_model, resolve_config
    c = resolve_config("t5-base").replace(num_layers=2, num_decoder_layers=2, vocab_size=4096, d_model=512,
                                            num_heads=8, d_kv=64, d_ff=1024, dropout_rate=0.0, attention_dropout=0.0)
    torch.manual_seed(0)
    return build_model(c).cuda().to(torch.bfloat16)


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


def _opt(model, **kw):
    from distributed_llms_example_amd.models.hf_io import hf_param_names
    flat = FlatParams(model, grad_dtype=torch.float32)
    cfg = model.config
    return FusedAdafactor(flat, parts=lambda n: len(hf_param_names(cfg, n)), **kw)


class _Spy:
    """The extension with its calls counted."""

    def __init__(self, C):
        self._C, self.calls = C, {}

    def __getattr__(self, name):
        f = getattr(self._C, name)
        if not callable(f):
            return f

        def wrapped(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            return f(*a, **k)
        return wrapped


def test_model_level_and_routing(monkeypatch):
    """FusedAdafactor on a 2-layer T5 (bf16 parameters, fp32 gradients), kernels against ``_reference_step`` on identical
    gradients for 3 steps: master rel-L2 < 1e-6 (the bound of test_adamw_bf16_params_fp32_grads), parameters < 5e-3.
    The composite route runs no native call; the default route a constant number per step."""
    import copy
    m1 = _small_t5()
    m2 = copy.deepcopy(m1)
    kw = dict(lr=1e-3, relative_step=False, scale_parameter=True, weight_decay=0.01,
              no_decay=lambda n: "layer_norm" in n)
    o1, o2 = _opt(m1, **kw), _opt(m2, **kw)
    assert any(u["part"] > 0 for u in o1.units)
    # a relayout before the first step, as the native reducer does after the first backward: the table follows it
    gen = torch.Generator().manual_seed(2)
    o1.flat.relayout(torch.randperm(len(o1.flat.segments), generator=gen).tolist())
    assert routing.get("adafactor") == "fused"
    route_default = routing.merged(adafactor="fused")
    spy = _Spy(_ext.native())
    monkeypatch.setattr(_ext, "native", lambda: spy)
    counts = []
    for step in range(3):
        gen = torch.Generator().manual_seed(10 + step)
        for (n, p), (_, q) in zip(sorted(m1.named_parameters()), sorted(m2.named_parameters())):
            g = (torch.randn(p.shape, generator=gen) * 1e-3).to(DEV)  # tiny values: bf16 would lose them
            p._dllm_gbuf.copy_(g)
            q._dllm_gbuf.copy_(g)
        spy.calls = {}
        n1 = o1.step(max_grad_norm=1.0)
        counts.append(dict(spy.calls))
        monkeypatch.setenv("DLLM_ROUTE", routing.merged(adafactor="composite"))
        spy.calls = {}
        n2 = o2.step(max_grad_norm=1.0)
        assert spy.calls == {}, spy.calls
        monkeypatch.setenv("DLLM_ROUTE", route_default)
        assert float(n1) == pytest.approx(float(n2), rel=1e-5)
        for (n, p), (_, q) in zip(sorted(m1.named_parameters()), sorted(m2.named_parameters())):
            assert _rel(p, q) < 5e-3, n
        e = _rel(o1.flat.to_canonical(o1.master), o2.master)
        print(f"[fig] model step {step + 1}: master rel-L2 {e:.3e} bound 1.0e-06")
        assert e < 1e-6
    assert counts[1] == counts[2] == {"sq_norm": 1, "adafactor_step": 1}, counts
    assert counts[0] == {"sq_norm": 1, "adafactor_plan": 1, "adafactor_step": 1}, counts


def test_graph_capture():
    """``opt.step(hyper=opt.device_hyper(t, lr))`` captured in one graph; three replays with ``t`` advanced on the
    device equal three eager steps (host scalars) within the kernel bounds: the only difference is beta2t computed in
    fp32 on the device."""
    import copy
    m1 = _small_t5()
    m2 = copy.deepcopy(m1)
    kw = dict(lr=LR, relative_step=False, scale_parameter=False)
    o1, o2 = _opt(m1, **kw), _opt(m2, **kw)

    def fill(step):
        gen = torch.Generator(device=DEV).manual_seed(50 + step)
        g = torch.randn(o1.flat.numel, generator=gen, device=DEV) * 1e-2
        o1.flat.grad_buf.copy_(g)
        o2.flat.grad_buf.copy_(g)

    fill(0)  # one eager step each: the unit table is built outside the capture
    o1.step(max_grad_norm=1.0)
    o2.step(max_grad_norm=1.0)
    assert torch.equal(o1.master, o2.master)
    t = torch.full((), 1.0, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    fill(1)
    with torch.cuda.graph(graph, stream=side):
        t.add_(1.0)
        o1.step(max_grad_norm=1.0, hyper=o1.device_hyper(t, LR))
    t.fill_(1.0)
    for step in range(1, 4):
        fill(step)
        before1, before2 = o1.master.clone(), o2.master.clone()
        graph.replay()
        o2.step(max_grad_norm=1.0)
        d, dref = (o1.master - before1).double(), (o2.master - before2).double()
        seg = o1.flat.segments
        worst = 0.0
        for s in seg:
            a, b = d[s.offset:s.offset + s.numel], dref[s.offset:s.offset + s.numel]
            tol = UPDATE_BOUND * (b.abs() + float(b.pow(2).mean().sqrt()))
            worst = max(worst, float(((a - b).abs() / tol).max()))
        print(f"[fig] graph replay {step}: worst update error / bound {worst:.3f}")
        assert worst <= 1.0
        assert torch.equal(o1.flat.param_buf, o1.master.to(torch.bfloat16))
    assert float(t) == 4.0
