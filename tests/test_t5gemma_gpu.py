"""T5Gemma on the GPU.  Both tiny presets have head dim 16: their attention takes the composite (asserted), everything
else the kernels.  A ``t5gemma-tiny`` variant at head dim 64 (hidden 256) runs bf16 on the HIP kernels against the fp32
torch reference path on the same weights — the method and model-level bounds of tests/test_longt5_gpu.py — with a spy
on the routes: soft-capped ``attn_hd_*`` everywhere (windowed on the encoder's sliding layers), never ``attn_fwd``,
``rope_fwd`` once per self-attention, the capped CE.  A graphed step equals the eager one, and ``generate`` on the GPU
gives the tokens of the CPU reference path."""
import os

import pytest
import torch

from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.models import PRESETS, build_model

pytestmark = pytest.mark.gpu
_WATCH = ("attn_fwd", "attn_hd_fwd", "attn_f32_fwd", "rope_fwd", "ce_fwd", "ce_chunk_fwd", "lmhead_ce_fwd", "norm_fwd")


def _cfg(**kw):
    """t5gemma-tiny at head dim 64: hidden 256, 4 heads, encoder window 4 (sliding, full), vocabulary 4096."""
    c = PRESETS["t5gemma-tiny"].replace(d_model=256, d_kv=64, d_ff=512, vocab_size=4096, query_pre_attn_scalar=64,
                                        attn_logit_softcapping=5.0, final_logit_softcapping=3.0)
    return c.replace(**kw)


def _reinit(m, embed=4.0, proj=3.0):
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "layernorm" in n or n.endswith(".norm.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
            elif "embed_tokens" in n:
                p.mul_(embed)
            else:
                p.mul_(proj)
            p.copy_(p.to(torch.bfloat16).float())  # exactly representable in bf16: the comparison measures compute
    return m


def _batch(cfg, B=4, S=150, T=16):
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, cfg.vocab_size, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    lab = torch.randint(3, cfg.vocab_size, (B, T), generator=g)
    am[1, 2 * S // 3:] = 0
    ids[1, 2 * S // 3:] = cfg.pad_token_id
    lab[-1, -5:] = -100
    return {k: v.cuda() for k, v in dict(input_ids=ids, attention_mask=am, labels=lab).items()}


def _spy(monkeypatch):
    """Records (binding, Sq or rows, window argument, softcap keyword) of the watched forwards, on every module that
    holds the native handle."""
    calls = []
    real = _ext.native()

    class Spy:
        def __getattr__(self, n):
            f = getattr(real, n)
            if n not in _WATCH:
                return f

            def g(*a, **kw):
                w = a[9] if n in ("attn_hd_fwd", "attn_f32_fwd") and len(a) > 9 else None
                calls.append((n, a[0].shape[1] if n.startswith("attn") else None, w, kw.get("softcap")))
                return f(*a, **kw)
            return g

    monkeypatch.setattr(_ext, "native", lambda: Spy())
    return calls


def _grad_report(m_test, m_ref):
    rep = []
    for (n, pt), (_, pr) in zip(m_test.named_parameters(), m_ref.named_parameters()):
        if pr.grad is None or pr.grad.norm() == 0:
            continue
        gt, gr = pt.grad.float().flatten(), pr.grad.float().flatten()
        rep.append((((gt - gr).norm() / gr.norm()).item(),
                    torch.nn.functional.cosine_similarity(gt, gr, dim=0).item(), n))
    return rep


@pytest.mark.parametrize("name", ["t5gemma-tiny", "t5gemma-tiny-gqa"])
def test_tiny_presets_take_the_composite_for_attention(name, monkeypatch):
    """Head dim 16: no attention kernel (one warning, the composite); RoPE, norms and the capped CE run their kernels,
    and the loss is the fp32 reference path's."""
    cfg = PRESETS[name]
    torch.manual_seed(0)
    m32 = _reinit(build_model(cfg)).cuda().eval()
    m16 = build_model(cfg).cuda()
    m16.load_state_dict(m32.state_dict())
    m16 = m16.to(torch.bfloat16).eval()
    b = _batch(cfg, B=2, S=23, T=9)
    os.environ["DLLM_REFERENCE_OPS"] = "1"
    try:
        ref = m32(**b)
    finally:
        os.environ.pop("DLLM_REFERENCE_OPS")
    calls = _spy(monkeypatch)
    out = m16(**b)
    names = [c[0] for c in calls]
    assert not [n for n in names if n.startswith("attn")], names
    assert names.count("rope_fwd") == cfg.num_layers + cfg.num_decoder_layers
    assert [c for c in calls if c[0] == "ce_fwd"] == [("ce_fwd", None, None, cfg.final_logit_softcapping)], calls
    assert abs(out.loss.item() - ref.loss.item()) < 0.02 * ref.loss.item(), (out.loss.item(), ref.loss.item())


@pytest.mark.parametrize("kv_heads", [4, 2])
def test_t5gemma_matches_fp32_reference(kv_heads, monkeypatch):
    """kv_heads = 2: grouped K/V heads on the kernels — q and k rotated as one slot of H + H_kv heads, strided q / k
    views and the repeated K / V into csrc/attn_hd.hip."""
    cfg = _cfg(num_kv_heads=kv_heads)
    torch.manual_seed(0)
    m32 = _reinit(build_model(cfg)).cuda().train()
    m16 = build_model(cfg).cuda()
    m16.load_state_dict(m32.state_dict())
    m16 = m16.to(torch.bfloat16).train()
    t16 = build_model(cfg).cuda()
    t16.load_state_dict(m32.state_dict())
    t16 = t16.to(torch.bfloat16).train()
    b = _batch(cfg)
    from distributed_llms_example_amd.ops.rng import manual_seed
    os.environ["DLLM_REFERENCE_OPS"] = "1"
    try:
        manual_seed(5)
        ref = m32(**b)
        ref.loss.backward()
        manual_seed(5)
        tb = t16(**b)
        tb.loss.backward()
    finally:
        os.environ.pop("DLLM_REFERENCE_OPS")
    calls = _spy(monkeypatch)
    manual_seed(5)
    out = m16(**b)
    calls = list(calls)  # the forward's: the backward runs rope_fwd once more per self-attention (sign -1)
    out.loss.backward()
    cap = cfg.attn_logit_softcapping
    attn = [c for c in calls if c[0].startswith("attn")]
    # encoder: sliding (window 4) then full; decoder: per layer causal self-attention (the window holds the 16 targets)
    # and cross-attention — every one capped, on attn_hd (csrc/attn.hip has no cap)
    assert attn == [("attn_hd_fwd", 150, 4, cap), ("attn_hd_fwd", 150, -1, cap)] + [("attn_hd_fwd", 16, -1, cap)] * 4, attn
    names = [c[0] for c in calls]
    assert "attn_fwd" not in names
    assert names.count("rope_fwd") == cfg.num_layers + cfg.num_decoder_layers  # once per self-attention
    assert [c for c in calls if c[0] == "ce_fwd"] == [("ce_fwd", None, None, cfg.final_logit_softcapping)], calls
    assert abs(out.loss.item() - ref.loss.item()) < 0.01 * ref.loss.item(), (out.loss.item(), ref.loss.item())
    rep = _grad_report(m16, m32)
    floor = {n: (rel, cos) for rel, cos, n in _grad_report(t16, m32)}
    names = {n for _, _, n in rep}
    assert "model.encoder.embed_tokens.weight" in names and "model.decoder.embed_tokens.weight" in names
    bad = []
    for rel, cos, n in rep:
        frel, fcos = floor[n]
        if rel > max(3e-2, 1.5 * frel) or 1 - cos > max(1e-3, 1.5 * (1 - fcos)):
            bad.append((n, rel, frel, cos, fcos))
    worst = max(rep)
    print(f"[t5gemma parity] worst rel {worst} (torch-bf16 floor {floor[worst[2]]}); "
          f"worst torch-bf16 rel {max(v[0] for v in floor.values()):.4f}")
    assert not bad, bad[:5]
    assert torch.isfinite(out.encoder_last_hidden_state.float()).all()


@pytest.fixture
def _no_leaked_step_seeds():
    """Step-seed mode is process-wide (ops/rng.py StepSeed): switched off afterwards, as in tests/test_graph_gpu.py."""
    from distributed_llms_example_amd.ops import rng as rng_mod
    yield
    st = rng_mod._active_step[0]
    if st is not None:
        st.disable()
    rng_mod.default_rng().site_mode = False


def test_t5gemma_graphed_step_equals_eager(_no_leaked_step_seeds):
    """Two warm-up steps and two replays of the captured step against the same four steps run eagerly (the method of
    tests/test_graph_gpu.py test_graphed_steps_match_eager), with dropout on so that the seeds are part of it."""
    from distributed_llms_example_amd.ops.rng import manual_seed
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    from distributed_llms_example_amd.train.graph import GraphedStep
    env = init_distributed()
    cfg = _cfg(dropout_rate=0.1, attention_dropout=0.1)
    torch.manual_seed(0)
    sd = _reinit(build_model(cfg)).state_dict()
    data = [_batch(cfg)]

    def engine():
        m = build_model(cfg)
        m.load_state_dict(sd)
        manual_seed(11)
        eng = TrainEngine(m, env, lr=1e-3, dtype=torch.bfloat16)
        eng.train()
        return eng

    eng_g = engine()
    gs = GraphedStep(eng_g, data, warmup=2)
    losses_g = [float(gs.replay(data)) for _ in range(2)]
    pg = eng_g.flat.to_canonical(eng_g.flat.param_buf).float().clone()
    eng_g.disable_step_seeds()

    eng_e = engine()
    eng_e.enable_step_seeds()
    t = torch.zeros((), dtype=torch.float32, device="cuda")
    losses_e = []
    for i in range(4):
        loss = float(eng_e.forward_backward(data[0], grad_accum=1, sync=True))
        t.add_(1.0)
        eng_e.step(hyper=eng_e.optimizer.device_hyper(t, eng_e.optimizer.param_groups[0]["lr"]))
        if i >= 2:
            losses_e.append(loss)
    pe = eng_e.flat.to_canonical(eng_e.flat.param_buf).float().clone()
    eng_e.disable_step_seeds()
    assert losses_g == pytest.approx(losses_e, rel=1e-3), (losses_g, losses_e)
    assert ((pg - pe).norm() / pe.norm()).item() < 1e-3


@pytest.mark.parametrize("kv_heads", [4, 2])
def test_t5gemma_generate_on_gpu_matches_the_cpu_reference(kv_heads, monkeypatch):
    """kv_heads = 2: the K/V store holds the 2 K/V heads and the model repeats them for the 4 query heads."""
    cfg = _cfg(num_kv_heads=kv_heads)
    torch.manual_seed(0)
    m = _reinit(build_model(cfg), embed=1.0).eval()  # smaller embeddings: the tied head does not just repeat its input
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab_size, (3, 150), generator=g)
    am = torch.ones_like(ids)
    am[2, 100:] = 0
    ids[2, 100:] = cfg.pad_token_id
    kw = dict(max_length=10, min_length=0, no_repeat_ngram_size=0, length_penalty=1.0, early_stopping=False)
    gpu = build_model(cfg)
    gpu.load_state_dict(m.state_dict())
    gpu = gpu.cuda().eval()  # fp32 on the GPU: csrc/attn_f32.hip with the cap, csrc/rope.hip in fp32
    for beams in (1, 3):
        want = m.generate(ids, attention_mask=am, num_beams=beams, **kw)
        calls = _spy(monkeypatch)
        got = gpu.generate(ids.cuda(), attention_mask=am.cuda(), num_beams=beams, **kw)
        assert torch.equal(got.cpu(), want), (beams, got, want)
        attn = [c for c in calls if c[0].startswith("attn")]
        assert attn and all(c[0] == "attn_f32_fwd" and c[3] == cfg.attn_logit_softcapping for c in attn), attn[:4]
        assert attn[0][2] == 4 and attn[1][2] == -1  # the encoder's sliding, then full layer
    assert want[:, 1:].unique().numel() > 3


def test_t5gemma_bf16_generate_with_grouped_heads_runs_the_decode_kernels(monkeypatch):
    """bf16, 2 K/V heads, 3 beams: the K/V store of H_kv heads through csrc/beam.hip ``kv_reorder`` and ``beam_topk``,
    capped attention on csrc/attn_hd.hip at every step; the output is well-formed (token parity is the fp32 test's)."""
    cfg = _cfg(num_kv_heads=2)
    torch.manual_seed(0)
    m = _reinit(build_model(cfg), embed=1.0).cuda().to(torch.bfloat16).eval()
    ids = torch.randint(3, cfg.vocab_size, (3, 150), device="cuda")
    real = _ext.native()
    seen = set()

    class Spy:
        def __getattr__(self, n):
            seen.add(n)
            return getattr(real, n)

    monkeypatch.setattr(_ext, "native", lambda: Spy())
    out = m.generate(ids, attention_mask=torch.ones_like(ids), max_length=10, num_beams=3)
    assert out.shape[0] == 3 and out.shape[1] <= 10 and (out[:, 0] == cfg.bos_token_id).all()
    assert {"attn_hd_fwd", "rope_fwd", "kv_reorder", "beam_topk"} <= seen, sorted(seen)
    assert "attn_fwd" not in seen


def test_adafactor_kernels_with_grouped_heads():
    """csrc/adafactor.hip on the unit table of a grouped-K/V model (the fused qkv_proj's three units differ in rows)
    against the torch composite on identical gradients, three steps: the bounds of tests/test_adafactor_gpu.py
    test_model_level_and_routing (master rel-L2 < 1e-6, bf16 parameters < 5e-3)."""
    import copy
    from distributed_llms_example_amd.models.hf_io import hf_param_parts
    from distributed_llms_example_amd.ops import routing
    from distributed_llms_example_amd.ops.optim import FusedAdafactor
    from distributed_llms_example_amd.parallel.flat import FlatParams
    cfg = _cfg(num_kv_heads=2)
    torch.manual_seed(0)
    m1 = build_model(cfg).cuda().to(torch.bfloat16)
    m2 = copy.deepcopy(m1)

    def opt(m):
        return FusedAdafactor(FlatParams(m, grad_dtype=torch.float32), parts=lambda n: hf_param_parts(cfg, n), lr=1e-3,
                              relative_step=False, scale_parameter=True, weight_decay=0.01,
                              no_decay=lambda n: "norm" in n)

    o1, o2 = opt(m1), opt(m2)
    assert sorted({u["rows"] for u in o1.units if u["name"].endswith("self_attn.qkv_proj.weight")}) == [128, 256]

    def rel(a, b):
        a, b = a.detach().double(), b.detach().double()
        return float((a - b).norm() / b.norm())

    default = os.environ.get("DLLM_ROUTE")
    try:
        for step in range(3):
            gen = torch.Generator().manual_seed(10 + step)
            for (n, p), (_, q) in zip(sorted(m1.named_parameters()), sorted(m2.named_parameters())):
                g = (torch.randn(p.shape, generator=gen) * 1e-3).cuda()
                p._dllm_gbuf.copy_(g)
                q._dllm_gbuf.copy_(g)
            os.environ["DLLM_ROUTE"] = routing.merged(adafactor="fused")
            n1 = o1.step(max_grad_norm=1.0)
            os.environ["DLLM_ROUTE"] = routing.merged(adafactor="composite")
            n2 = o2.step(max_grad_norm=1.0)
            assert float(n1) == pytest.approx(float(n2), rel=1e-5)
            for (n, p), (_, q) in zip(sorted(m1.named_parameters()), sorted(m2.named_parameters())):
                assert rel(p, q) < 5e-3, n
            e = rel(o1.flat.to_canonical(o1.master), o2.flat.to_canonical(o2.master))
            print(f"[fig] t5gemma gqa adafactor step {step + 1}: master rel-L2 {e:.3e} bound 1.0e-06")
            assert e < 1e-6
    finally:
        if default is None:
            os.environ.pop("DLLM_ROUTE", None)
        else:
            os.environ["DLLM_ROUTE"] = default
