"""BigBird-Pegasus on the GPU: the bf16 HIP-kernel path (encoder self-attention on csrc/attn_hd.hip following the block
lists of models/bigbird.py, decoder on csrc/attn.hip) against the fp32 torch reference path on the same weights and
dropout masks — the method, bounds and floors of tests/test_longt5_gpu.py; the fp32 engine (encoder on
csrc/attn_f32.hip); generation; and a 4096-token input whose step stays below one [H, S, S] score tensor."""
import os

import pytest
import torch

from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.models import build_model, resolve_config
from distributed_llms_example_amd.ops import attention as A

pytestmark = pytest.mark.gpu
_FWD = ("attn_fwd", "attn_hd_fwd", "attn_f32_fwd")


@pytest.fixture(autouse=True)
def _no_leaked_step_seeds():
    """As tests/test_graph_gpu.py: step-seed mode is process-wide and is switched off after every test."""
    from distributed_llms_example_amd.ops import rng as rng_mod
    yield
    st = rng_mod._active_step[0]
    if st is not None:
        st.disable()
    rng_mod.default_rng().site_mode = False


def _cfg(**kw):
    """Head dim 64, d_model 256, 4 heads, 2 + 2 layers, block 64, 3 random blocks (the presets' own)."""
    c = resolve_config("bigbird-pegasus-large-arxiv").replace(num_layers=2, num_decoder_layers=2, vocab_size=4096,
                                                              d_model=256, num_heads=4, d_kv=64, d_ff=512)
    assert c.model_type == "bigbird_pegasus" and (c.block_size, c.num_random_blocks, c.use_bias) == (64, 3, False)
    return c.replace(**kw)


def _batch(cfg, B=2, S=832, T=16, keep1=700):
    """13 blocks of 64; row 1 keeps ``keep1`` source tokens."""
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, cfg.vocab_size, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    lab = torch.randint(3, cfg.vocab_size, (B, T), generator=g)
    if B > 1:
        am[1, keep1:] = 0
        lab[1, -5:] = -100
    return {k: v.cuda() for k, v in dict(input_ids=ids, attention_mask=am, labels=lab).items()}


def _spy(monkeypatch):
    """Records (binding, Sq, block lists given) of every attention forward."""
    calls = []
    real = _ext.native()

    class Spy:
        def __getattr__(self, n):
            f = getattr(real, n)
            if n not in _FWD:
                return f

            def g(*a, **kw):
                q = a[0] if a else kw["q"]
                lists = all(kw.get(t) is not None for t in ("kl_ptr", "kl_idx", "ql_ptr", "ql_idx"))
                calls.append((n, q.shape[1], lists))
                return f(*a, **kw)
            return g

    monkeypatch.setattr(A._ext, "native", lambda: Spy())
    return calls


def _grad_report(m_test, m_ref):
    rep = []
    for (n, pt), (_, pr) in zip(m_test.named_parameters(), m_ref.named_parameters()):
        if pr.grad is None or pr.grad.norm() == 0:
            continue
        gt, gr = pt.grad.float().flatten(), pr.grad.float().flatten()
        rel = ((gt - gr).norm() / gr.norm()).item()
        cos = torch.nn.functional.cosine_similarity(gt, gr, dim=0).item()
        rep.append((rel, cos, n))
    return rep


def test_bigbird_matches_fp32_reference(monkeypatch):
    cfg = _cfg()
    torch.manual_seed(0)
    m32 = build_model(cfg).cuda()
    with torch.no_grad():  # weights exactly representable in bf16: the comparison measures compute, not weight rounding
        for p in m32.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    m32.train()
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
    manual_seed(5)  # same dropout masks on every path
    out = m16(**b)
    out.loss.backward()
    # exactly one list-carrying attn_hd launch per encoder layer; decoder self- and cross-attention on the tuned kernels
    assert calls == [("attn_hd_fwd", 832, True)] * 2 + [("attn_fwd", 16, False)] * 4, calls
    assert abs(out.loss.item() - ref.loss.item()) < 0.01 * ref.loss.item(), (out.loss.item(), ref.loss.item())
    rep = _grad_report(m16, m32)
    floor = {n: (rel, cos) for rel, cos, n in _grad_report(t16, m32)}
    names = {n for _, _, n in rep}
    for layer in range(2):
        assert f"model.encoder.layers.{layer}.self_attn.qkv_proj.weight" in names
    bad = []
    for rel, cos, n in rep:
        frel, fcos = floor[n]
        if rel > max(3e-2, 1.5 * frel) or 1 - cos > max(1e-3, 1.5 * (1 - fcos)):
            bad.append((n, rel, frel, cos, fcos))
    worst = max(rep)
    print(f"[bigbird parity] worst rel {worst} (torch-bf16 floor {floor[worst[2]]}); "
          f"worst torch-bf16 rel {max(v[0] for v in floor.values()):.4f}")
    assert not bad, bad[:5]
    assert torch.isfinite(out.encoder_last_hidden_state.float()).all()


def test_bigbird_fp32_training_matches_reference(monkeypatch):
    """fp32 end to end: one engine step against the pure-torch reference step; the encoder's attention runs
    csrc/attn_f32.hip with the block lists."""
    from distributed_llms_example_amd.ops.rng import manual_seed
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    env = init_distributed()
    cfg = _cfg()
    torch.manual_seed(0)
    sd = build_model(cfg).state_dict()
    b = _batch(cfg)
    res = []
    calls = None
    for ref in (True, False):
        if ref:
            os.environ["DLLM_REFERENCE_OPS"] = "1"
        else:
            calls = _spy(monkeypatch)
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
    assert calls == [("attn_f32_fwd", 832, True)] * 2 + [("attn_f32_fwd", 16, False)] * 4, calls
    (l0, g0, p0), (l1, g1, p1) = res
    assert g1.dtype == torch.float32 and p1.dtype == torch.float32
    assert abs(l0 - l1) < 1e-4 * abs(l0), (l0, l1)
    assert ((g1 - g0).norm() / g0.norm()).item() < 1e-3
    assert ((p1 - p0).norm() / p0.norm()).item() < 1e-5


def test_bigbird_generate_on_gpu(monkeypatch):
    """Eval mode: the encoder's lists are the ones with block 0 repeated."""
    cfg = _cfg()
    m = build_model(cfg).cuda().to(torch.bfloat16).eval()
    ids = torch.randint(3, cfg.vocab_size, (3, 832), device="cuda")
    calls = _spy(monkeypatch)
    out = m.generate(ids, attention_mask=torch.ones_like(ids), max_length=12, num_beams=2)
    assert out.shape[0] == 3 and out.shape[1] <= 12
    assert calls[:2] == [("attn_hd_fwd", 832, True)] * 2, calls[:4]
    assert all(c[0] == "attn_fwd" and not c[2] for c in calls[2:]), sorted(set(calls[2:]))
    del calls[:]
    short = m.generate(ids[:, :448], max_length=8, num_beams=1)  # 448 <= (5 + 2 * 3) * 64: the full-attention rule
    assert short.shape[0] == 3
    assert all(c[0] == "attn_fwd" and not c[2] for c in calls), sorted(set(calls))


def test_4096_token_step_stays_below_one_score_tensor(monkeypatch):
    """4096 source tokens (the padded length at which transformers uses the old plan, repeats included), B = 1: exactly
    one list-carrying attn_hd_fwd per encoder layer, and the peak memory of the step — forward and backward, every
    activation and gradient, above the baseline of the resident model and batch — stays below ONE bf16 [H, S, S] score
    tensor (4 x 4096^2 x 2 B = 128 MiB), which any O(S^2) path would have to hold (the composite holds several, in
    fp32).  At this length that is a tight bound: the step's own O(S) tensors measured 121 MiB, and with the 12 MiB of
    bf16 weights counted in, 133 MiB."""
    S = 4096
    cfg = _cfg()
    assert cfg.max_position_embeddings >= S
    torch.manual_seed(0)
    import gc
    m = build_model(cfg).cuda().to(torch.bfloat16).train()
    b = _batch(cfg, B=1, S=S, T=16)
    b["attention_mask"][0, -500:] = 0
    calls = _spy(monkeypatch)
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = m(**b)
    out.loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert [c for c in calls if c[0] == "attn_hd_fwd"] == [("attn_hd_fwd", S, True)] * cfg.num_layers, calls
    assert [c for c in calls if c[0] != "attn_hd_fwd"] == [("attn_fwd", 16, False)] * 4, calls
    print(f"[bigbird 4096] peak {peak / 2**20:.1f} MiB above {base / 2**20:.1f} MiB")
    assert peak < cfg.num_heads * S * S * 2, peak
    assert torch.isfinite(out.loss).item()
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad.float()).all(), n
