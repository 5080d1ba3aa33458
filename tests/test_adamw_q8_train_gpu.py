"""``TrainEngine(optim="adamw_8bit")`` on a 2-layer T5 on the GPU: the captured step against the eager one, the torch
composite against csrc/adamw_q8.hip, and the loss against fp32 AdamW."""
import math

import pytest
import torch

import rowwise_refs as R
from distributed_llms_example_amd.models import build_model, resolve_config
from distributed_llms_example_amd.ops import routing
from distributed_llms_example_amd.ops.optim import FusedAdamW8bit
from distributed_llms_example_amd.ops.rng import manual_seed
from distributed_llms_example_amd.parallel.env import init_distributed
from distributed_llms_example_amd.train.engine import TrainEngine
from distributed_llms_example_amd.train.graph import GraphedStep
from test_adamw_q8_gpu import _deq64, _nearest_gap

pytestmark = pytest.mark.gpu
CFG = dict(num_layers=2, num_decoder_layers=2, vocab_size=4096, d_model=512, num_heads=8, d_kv=64, d_ff=1024,
           dropout_rate=0.0, attention_dropout=0.0)
STATE = ("code_m", "code_v", "absmax_m", "absmax_v", "side_m", "side_v", "master")

# Relative loss gap adamw_8bit vs adamw after LOSS_STEPS steps, same seed and batches, measured once on an MI355X
# (profiles/adamw_q8_step.txt).  Asserted at twice that: both runs are deterministic, so the gap repeats; the factor 2
# leaves room for another compiler's contraction of the fp32 recurrence moving individual codes, no more.
LOSS_STEPS = 20
LOSS_GAP_MEASURED = 1.747e-2


@pytest.fixture
def _no_leaked_step_seeds():
    from distributed_llms_example_amd.ops import rng as rng_mod
    yield
    st = rng_mod._active_step[0]
    if st is not None:
        st.disable()
    rng_mod.default_rng().site_mode = False


def _batches(n, B=4, S=64, T=32):
    g = torch.Generator().manual_seed(3)
    return [{"input_ids": torch.randint(3, 4096, (B, S), generator=g).cuda(),
             "attention_mask": torch.ones(B, S, dtype=torch.long).cuda(),
             "labels": torch.randint(3, 4096, (B, T), generator=g).cuda()} for _ in range(n)]


def _engine(optim="adamw_8bit", **kw):
    torch.manual_seed(0)
    m = build_model(resolve_config("t5-base").replace(**CFG))
    manual_seed(11)
    eng = TrainEngine(m, init_distributed(), lr=1e-3, dtype=torch.bfloat16, optim=optim, weight_decay=0.01, **kw)
    eng.train()
    return eng


def test_graphed_step_equals_eager_bit_for_bit(_no_leaked_step_seeds):
    data = _batches(1)
    eg = _engine()
    opt = eg.optimizer
    assert isinstance(opt, FusedAdamW8bit) and (opt.slots >= 0).any() and (opt.slots < 0).any()
    assert "shared.weight" in opt.fp32_slots  # the embedding (and the tied LM head) keeps fp32 moments
    gs = GraphedStep(eg, data, warmup=1)
    for _ in range(2):
        gs.replay(data)
    eg.disable_step_seeds()
    ee = _engine()
    ee.enable_step_seeds()
    t = torch.zeros((), dtype=torch.float32, device="cuda")
    for _ in range(3):
        ee.forward_backward(data[0], grad_accum=1, sync=True)
        t.add_(1.0)
        ee.step(hyper=ee.optimizer.device_hyper(t, ee.optimizer.param_groups[0]["lr"]))
    ee.disable_step_seeds()
    sg, se = eg.optimizer.state_dict(), ee.optimizer.state_dict()
    for k in STATE:
        assert torch.equal(sg[k], se[k]), k
    assert torch.equal(eg.flat.to_canonical(eg.flat.param_buf), ee.flat.to_canonical(ee.flat.param_buf))
    assert len(torch.unique(sg["code_m"])) > 64


def test_composite_agrees_with_kernel(monkeypatch):
    """One step from a zero state without a clip, so the exact new moments are (1 - b1) g and (1 - b2) g^2 of the
    gradient buffer: kernel and composite each meet the bounds of tests/test_adamw_q8_gpu.py against them, and their
    masters agree within its parameter bound."""
    from distributed_llms_example_amd.ops import optim as optim_mod
    monkeypatch.setattr(optim_mod, "_warned_q8_composite", [False])
    data = _batches(1)
    engs, grads = [], []
    for route in ("fused", "composite"):
        monkeypatch.setenv("DLLM_ROUTE", routing.merged(adamw_q8=route))
        eng = _engine(max_grad_norm=None)
        eng.forward_backward(data[0], grad_accum=1, sync=True)
        g = eng.flat.grad_buf.double().view(-1, 64)
        grads.append(g)
        if route == "composite":
            with pytest.warns(UserWarning, match="composite"):
                eng.step()
        else:
            eng.step()
        opt = eng.optimizer
        # the kernel takes the betas as fp32 and forms 1 - beta exactly; the composite passes doubles to torch
        b1, b2 = opt.betas if route == "composite" else (float(torch.tensor(b, dtype=torch.float32)) for b in opt.betas)
        q = opt.slots < 0
        for signed, codes, absmax, e in ((True, opt.code_m, opt.absmax_m, (1.0 - b1) * g),
                                         (False, opt.code_v, opt.absmax_v, (1.0 - b2) * g * g)):
            e, a = e[q], absmax[q]
            want = e.abs().amax(-1)
            assert ((a.double() - want).abs() <= 2.0 ** -21 * want).all(), route
            d = _deq64(codes[q], a, signed)
            over = (d - e).abs() - _nearest_gap(e, a, signed) - 2.0 ** -20 * torch.maximum(e.abs(), d.abs())
            assert not (over > 0).any(), (route, signed, int((over > 0).sum()))
        engs.append(eng)
    k, c = (e.optimizer.master for e in engs)
    assert torch.equal(*grads)
    print(f"[fig] composite vs kernel master: rel-L2 {R.rel_l2(k, c):.3e} elem {R.elem_err(k, c):.3e}")
    assert R.elem_err(k, c) < 1e-5


def test_loss_tracks_fp32_adamw():
    data, final = _batches(4), {}
    for optim in ("adamw", "adamw_8bit"):
        eng = _engine(optim)
        for i in range(LOSS_STEPS):
            loss = eng.forward_backward(data[i % 4], grad_accum=1, sync=True)
            eng.step()
        final[optim] = float(loss)
    l32, l8 = final["adamw"], final["adamw_8bit"]
    print(f"[fig] loss after {LOSS_STEPS} steps: adamw {l32:.6f} adamw_8bit {l8:.6f} gap {abs(l8 - l32) / l32:.3e}")
    assert l32 < math.log(4096)  # below the loss of a uniform prediction: the run trains
    assert abs(l8 - l32) / l32 <= 2 * LOSS_GAP_MEASURED
