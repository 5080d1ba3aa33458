"""Packed training steps on the GPU: the native path (segment-masked kernels) against the torch reference path on the
same packed batch, by the protocols of tests/test_model_gpu.py; a graphed packed step against the eager one; and a spy
on the bindings — every attention call of a packed step runs csrc/attn_hd.hip or csrc/attn_f32.hip with segments."""
import os

import numpy as np
import pytest
import torch

from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.data.collator import DataCollatorForSeq2Seq
from distributed_llms_example_amd.data.packing import pack_examples
from distributed_llms_example_amd.models import build_model, resolve_config
from distributed_llms_example_amd.ops import attention as A

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_leaked_step_seeds():
    """Step-seed mode is process-wide (ops/rng.py StepSeed): switched off after every test, as tests/test_graph_gpu.py
    does, so later dropout tests in the same process run in the default mode."""
    from distributed_llms_example_amd.ops import rng as rng_mod
    yield
    st = rng_mod._active_step[0]
    if st is not None:
        st.disable()
    rng_mod.default_rng().site_mode = False


def _cfg(name):
    """Small but kernel-shaped (head dim 64), as tests/test_model_gpu.py."""
    return resolve_config(name).replace(num_layers=2, num_decoder_layers=2, vocab_size=4096, d_model=512, num_heads=8,
                                        d_kv=64, d_ff=1024)


def _packed_batches(cfg, n, rows=4, S=256, T=64, seed=0):
    """``n`` packed batches of ``rows`` rows: sources of 20 .. 150 and targets of 1 .. 30 tokens, so boundaries fall
    mid-block and rows end in a padded tail."""
    rng = np.random.default_rng(seed)
    ex = [(rng.integers(3, cfg.vocab_size, size=int(s)), rng.integers(3, cfg.vocab_size, size=int(t)))
          for s, t in zip(rng.integers(20, 151, 40 * n), rng.integers(1, 31, 40 * n))]
    pk = pack_examples(ex, S, T, cfg.pad_token_id, cfg.decoder_start_token_id, seed=seed, shift_mode=cfg.shift_mode)
    assert len(pk) >= n * rows and pk.examples_per_row > 1.5
    # first-fit-decreasing fills its first rows with the longest sources: take rows spread over the whole packing
    idx = np.linspace(0, len(pk) - 1, n * rows).astype(int)
    assert (pk.arrays["segment_ids"][idx, -1] == -1).any()
    coll = DataCollatorForSeq2Seq.for_model(cfg)
    return [{k: v.cuda() for k, v in coll([pk[int(i)] for i in idx[b::n]]).items()} for b in range(n)]


def _grad_report(m_test, m_ref):
    rep = []
    for (n, pt), (_, pr) in zip(m_test.named_parameters(), m_ref.named_parameters()):
        if pr.grad is None or pr.grad.norm() == 0:
            continue
        gt, gr = pt.grad.float().flatten(), pr.grad.float().flatten()
        rep.append((((gt - gr).norm() / gr.norm()).item(),
                    torch.nn.functional.cosine_similarity(gt, gr, dim=0).item(), n))
    return rep


@pytest.mark.parametrize("name", ["t5-base", "bart-base"])
def test_packed_native_bf16_matches_fp32_reference(name):
    """tests/test_model_gpu.py test_native_bf16_matches_fp32_reference on a packed batch: loss within 1 %, every
    parameter's gradient within 1.5x of what the plain-torch composite run in bf16 costs on that parameter (floors
    3e-2 relative, 1e-3 cosine deficit)."""
    from distributed_llms_example_amd.ops.rng import manual_seed
    cfg = _cfg(name)
    torch.manual_seed(0)
    m32 = build_model(cfg).cuda()
    with torch.no_grad():
        for p in m32.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    m32.train()
    m16, t16 = (build_model(cfg).cuda() for _ in range(2))
    for m in (m16, t16):
        m.load_state_dict(m32.state_dict())
    m16, t16 = m16.to(torch.bfloat16).train(), t16.to(torch.bfloat16).train()
    b = _packed_batches(cfg, 1)[0]
    os.environ["DLLM_REFERENCE_OPS"] = "1"
    try:
        manual_seed(5)
        ref = m32(**b)
        ref.loss.backward()
        manual_seed(5)
        t16(**b).loss.backward()
    finally:
        os.environ.pop("DLLM_REFERENCE_OPS")
    manual_seed(5)  # same dropout masks on every path
    out = m16(**b)
    out.loss.backward()
    assert abs(out.loss.item() - ref.loss.item()) < 0.01 * ref.loss.item(), (out.loss.item(), ref.loss.item())
    rep = _grad_report(m16, m32)
    floor = {n: (rel, cos) for rel, cos, n in _grad_report(t16, m32)}
    bad = [(n, rel, floor[n][0], cos, floor[n][1]) for rel, cos, n in rep
           if rel > max(3e-2, 1.5 * floor[n][0]) or 1 - cos > max(1e-3, 1.5 * (1 - floor[n][1]))]
    worst = max(rep)
    print(f"[packed parity {name}] loss {out.loss.item():.4f} / {ref.loss.item():.4f}; worst rel {worst} "
          f"(torch-bf16 floor {floor[worst[2]]})")
    assert len(rep) > 20 and not bad, bad[:5]


@pytest.mark.parametrize("name", ["t5-base", "bart-base"])
def test_packed_fp32_training_matches_reference(name):
    """tests/test_model_gpu.py test_fp32_training_on_gpu_matches_reference on a packed batch: one fp32 engine step on
    the fp32 kernels against the pure-torch reference step."""
    from distributed_llms_example_amd.ops.rng import manual_seed
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    env = init_distributed()
    cfg = _cfg(name)
    torch.manual_seed(0)
    sd = build_model(cfg).state_dict()
    b = _packed_batches(cfg, 1)[0]
    res = []
    for ref in (True, False):
        if ref:
            os.environ["DLLM_REFERENCE_OPS"] = "1"
        try:
            m = build_model(cfg)
            m.load_state_dict(sd)
            eng = TrainEngine(m, env, lr=1e-3, dtype=torch.float32)
            eng.train()
            manual_seed(5)
            loss = eng.forward_backward(b)
            g = eng.flat.grad_buf.clone()
            eng.step()
            res.append((float(loss), g, eng.flat.param_buf.clone()))
        finally:
            os.environ.pop("DLLM_REFERENCE_OPS", None)
    (l0, g0, p0), (l1, g1, p1) = res
    assert g1.dtype == torch.float32 and p1.dtype == torch.float32
    assert abs(l0 - l1) < 1e-4 * abs(l0), (l0, l1)
    assert ((g1 - g0).norm() / g0.norm()).item() < 1e-3
    assert ((p1 - p0).norm() / p0.norm()).item() < 1e-5


# ------------------------------------------------------------------------------------------------------------ spy
_NAMES = ("attn_fwd", "attn_bwd", "attn_hd_fwd", "attn_hd_bwd", "attn_f32_fwd", "attn_f32_bwd")


class _Spy:
    """The native module with the attention bindings' calls recorded as (name, segments given)."""

    def __init__(self, calls, real):
        self.calls, self.real = calls, real

    def __getattr__(self, n):
        real = getattr(self.real, n)
        if n not in _NAMES:
            return real

        def f(*a, **kw):
            pos = 9 if n.endswith("fwd") else 16
            seg = n not in ("attn_fwd", "attn_bwd") and len(a) == pos + 5 and all(t is not None for t in a[pos + 1:])
            self.calls.append((n, seg))
            return real(*a, **kw)
        return f


@pytest.mark.parametrize("name,dtype", [("t5-base", torch.bfloat16), ("bart-base", torch.bfloat16),
                                        ("t5-base", torch.float32)])
def test_every_attention_call_of_a_packed_step_has_segments(name, dtype, monkeypatch):
    """2 + 2 layers: 2 encoder self-attentions, 2 decoder self-attentions and 2 cross-attentions, forward and backward,
    all on csrc/attn_hd.hip (bf16) or csrc/attn_f32.hip (fp32) with segments — none on csrc/attn.hip, and none on the
    composite (which would warn: the warning set stays as it was)."""
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    calls = []
    monkeypatch.setattr(A._ext, "native", lambda spy=_Spy(calls, _ext.native()): spy)
    warned = set(A._warned)
    cfg = _cfg(name)
    torch.manual_seed(0)
    eng = TrainEngine(build_model(cfg), init_distributed(), lr=1e-3, dtype=dtype)
    eng.train()
    loss = eng.forward_backward(_packed_batches(cfg, 1)[0])
    eng.step()
    assert torch.isfinite(loss)
    fam = "attn_hd" if dtype == torch.bfloat16 else "attn_f32"
    assert sorted(calls) == sorted([(fam + "_fwd", True)] * 6 + [(fam + "_bwd", True)] * 6), calls
    assert A._warned == warned


# ---------------------------------------------------------------------------------------------------------- graph
def _engine(cfg):
    from distributed_llms_example_amd.ops.rng import manual_seed
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    torch.manual_seed(0)
    m = build_model(cfg)
    manual_seed(11)
    eng = TrainEngine(m, init_distributed(), lr=1e-3, dtype=torch.bfloat16, bucket_mb=8.0)
    eng.train()
    return eng


@pytest.mark.parametrize("name", ["t5-base", "bart-base"])
def test_graphed_packed_steps_match_eager(name):
    """tests/test_graph_gpu.py test_graphed_steps_match_eager on packed batches: the segment and position ids are
    tensors of fixed shape, copied into the graph's static inputs like every other batch key."""
    from distributed_llms_example_amd.train.graph import GraphedStep
    cfg = _cfg(name)
    steps = 3
    data = _packed_batches(cfg, steps + 2)
    assert not torch.equal(data[2]["segment_ids"], data[3]["segment_ids"])  # replays see other ids than the capture
    eng_g = _engine(cfg)
    gs = GraphedStep(eng_g, data[:1], warmup=2)  # 2 warm-up steps on data[0]
    losses_g = [float(gs.replay(data[2 + i:3 + i])) for i in range(steps)]
    pg = eng_g.flat.to_canonical(eng_g.flat.param_buf).float().clone()
    eng_g.disable_step_seeds()

    eng_e = _engine(cfg)
    eng_e.enable_step_seeds()
    t = torch.zeros((), dtype=torch.float32, device="cuda")
    losses_e = []
    for i in range(steps + 2):
        loss = float(eng_e.forward_backward(data[0] if i < 2 else data[i]))
        t.add_(1.0)
        eng_e.step(hyper=eng_e.optimizer.device_hyper(t, eng_e.optimizer.param_groups[0]["lr"]))
        if i >= 2:
            losses_e.append(loss)
    pe = eng_e.flat.to_canonical(eng_e.flat.param_buf).float().clone()
    eng_e.disable_step_seeds()
    assert losses_g == pytest.approx(losses_e, rel=1e-3), (losses_g, losses_e)
    assert ((pg - pe).norm() / pe.norm()).item() < 1e-3
