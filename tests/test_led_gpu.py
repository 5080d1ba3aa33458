"""LED on the GPU, after tests/test_longt5_gpu.py: the bf16 HIP-kernel path (encoder self-attention on csrc/attn_hd.hip
with a window and global keys, the global rows and the decoder on csrc/attn.hip) against the fp32 torch reference path
on the same weights and dropout masks; the fp32 engine (csrc/attn_f32.hip); generation; a graphed training step
against the eager one; and a 12K-token encoder input in one windowed launch per layer."""
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
    """Head dim 64, d_model 256, 4 heads, 2 + 2 layers, window 256 (128 keys on either side), attention dropout on."""
    c = resolve_config("led-base-16384").replace(num_layers=2, num_decoder_layers=2, vocab_size=4096, d_model=256,
                                                 num_heads=4, d_kv=64, d_ff=512, attention_window=[256, 256],
                                                 attention_dropout=0.1)
    assert c.model_type == "led" and c.max_encoder_position_embeddings == 16384
    return c.replace(**kw)


def _batch(cfg, B=4, S=300, T=16, seed=0, extra=200):
    """Row 1 keeps 140 source tokens.  Token 0 of every row is global, and token ``extra`` of row 2 as well; the batch
    names them both ways, as data/collator.py does."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, cfg.vocab_size, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    lab = torch.randint(3, cfg.vocab_size, (B, T), generator=g)
    gi = torch.full((B, 2), -1, dtype=torch.long)
    gi[:, 0] = 0
    if B > 2:
        am[1, 140:] = 0
        lab[2, -5:] = -100
        gi[2, 1] = extra
    gm = torch.zeros(B, S, dtype=torch.long)
    gm[:, 0] = 1
    if B > 2:
        gm[2, extra] = 1
    out = dict(input_ids=ids, attention_mask=am, labels=lab, global_attention_mask=gm, global_index=gi)
    return {k: v.cuda() for k, v in out.items()}


def _spy(monkeypatch):
    """Records (binding, Sq, window argument, global flags given) of every attention forward."""
    calls = []
    real = _ext.native()

    class Spy:
        def __getattr__(self, n):
            f = getattr(real, n)
            if n not in _FWD:
                return f

            def g(*a, **kw):
                q = a[0] if a else kw["q"]
                glob = kw.get("k_glob") is not None and kw.get("k_gblk") is not None
                calls.append((n, q.shape[1], a[9] if n != "attn_fwd" and len(a) > 9 else None, glob))
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


def test_led_matches_fp32_reference(monkeypatch):
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
    # per encoder layer one windowed attn_hd launch with the flags, then its global rows (2 per batch row) on the tuned
    # kernels; decoder self- and cross-attention on the tuned kernels, no window
    assert calls == [("attn_hd_fwd", 300, 128, True), ("attn_fwd", 2, None, False)] * 2 + \
        [("attn_fwd", 16, None, False)] * 4, calls
    assert abs(out.loss.item() - ref.loss.item()) < 0.01 * ref.loss.item(), (out.loss.item(), ref.loss.item())
    rep = _grad_report(m16, m32)
    floor = {n: (rel, cos) for rel, cos, n in _grad_report(t16, m32)}
    names = {n for _, _, n in rep}
    for part in ("q_global.weight", "kv_global.weight", "qkv_proj.weight"):
        assert f"model.encoder.layers.0.self_attn.{part}" in names
    bad = []
    for rel, cos, n in rep:
        frel, fcos = floor[n]
        if rel > max(3e-2, 1.5 * frel) or 1 - cos > max(1e-3, 1.5 * (1 - fcos)):
            bad.append((n, rel, frel, cos, fcos))
    worst = max(rep)
    print(f"[led parity] worst rel {worst} (torch-bf16 floor {floor[worst[2]]}); "
          f"worst torch-bf16 rel {max(v[0] for v in floor.values()):.4f}")
    assert not bad, bad[:5]
    assert torch.isfinite(out.encoder_last_hidden_state.float()).all()


def test_led_fp32_training_matches_reference(monkeypatch):
    """fp32 end to end: one engine step against the pure-torch reference step; the encoder's attention runs
    csrc/attn_f32.hip with the window and the global keys."""
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
    assert calls == [("attn_f32_fwd", 300, 128, True), ("attn_f32_fwd", 2, -1, False)] * 2 + \
        [("attn_f32_fwd", 16, -1, False)] * 4, calls
    (l0, g0, p0), (l1, g1, p1) = res
    assert g1.dtype == torch.float32 and p1.dtype == torch.float32
    assert abs(l0 - l1) < 1e-4 * abs(l0), (l0, l1)
    assert ((g1 - g0).norm() / g0.norm()).item() < 1e-3
    assert ((p1 - p0).norm() / p0.norm()).item() < 1e-5


def test_led_generate_on_gpu(monkeypatch):
    cfg = _cfg()
    m = build_model(cfg).cuda().to(torch.bfloat16).eval()
    ids = torch.randint(3, cfg.vocab_size, (3, 300), device="cuda")
    gm = torch.zeros_like(ids)
    gm[:, 0] = 1
    calls = _spy(monkeypatch)
    out = m.generate(ids, attention_mask=torch.ones_like(ids), global_attention_mask=gm, max_length=12, num_beams=2)
    assert out.shape[0] == 3 and out.shape[1] <= 12
    assert calls[:4] == [("attn_hd_fwd", 300, 128, True), ("attn_fwd", 1, None, False)] * 2, calls[:6]
    assert all(c[0] == "attn_fwd" and c[2] is None for c in calls[4:]), sorted(set(calls[4:]))
    out_i = m.generate(ids, attention_mask=torch.ones_like(ids), global_index=torch.zeros(3, 1, dtype=torch.long,
                                                                                          device="cuda"),
                       max_length=12, num_beams=2)
    assert torch.equal(out, out_i)
    out1 = m.generate(ids, max_length=12, num_beams=1)  # no global token: the plain windowed encoder
    assert out1.shape[0] == 3


def test_graphed_step_matches_eager():
    """train/graph.py carries global_attention_mask / global_index like any batch tensor: steps replayed from the HIP
    graph on batches whose global tokens differ from the captured ones equal the same steps run eagerly."""
    from distributed_llms_example_amd.ops.rng import manual_seed
    from distributed_llms_example_amd.parallel.env import init_distributed
    from distributed_llms_example_amd.train.engine import TrainEngine
    from distributed_llms_example_amd.train.graph import GraphedStep
    env = init_distributed()
    cfg = _cfg()
    steps = 3
    data = [_batch(cfg, seed=i, extra=50 + 60 * i) for i in range(steps + 2)]

    def setup():
        torch.manual_seed(0)
        m = build_model(cfg)
        manual_seed(11)
        eng = TrainEngine(m, env, lr=1e-3, dtype=torch.bfloat16, bucket_mb=8.0)
        eng.train()
        return eng

    eng_g = setup()
    gs = GraphedStep(eng_g, data[:1], warmup=2)
    assert gs.use_graph
    assert {"global_attention_mask", "global_index"} <= set(gs.static[0])
    losses_g = [float(gs.replay(data[2 + i:3 + i])) for i in range(steps)]
    pg = eng_g.flat.to_canonical(eng_g.flat.param_buf).float().clone()
    eng_g.disable_step_seeds()

    eng_e = setup()
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


def test_long_encoder_input_is_one_windowed_launch_per_layer(monkeypatch):
    """12288 source tokens (above attn_chunk_min, where the plain T5 encoder goes to 4K-token chunks): exactly one
    windowed attn_hd_fwd per encoder layer at Sq = 12288 with the global flags, and the peak memory of model + batch +
    step stays below ONE bf16 [H, S, S] score tensor (4 x 12288^2 x 2 B = 1.2 GB) — which any O(S^2) path would have
    to hold.  The peak is counted above what earlier tests of the process still hold."""
    from distributed_llms_example_amd.ops import routing
    S = 12288
    assert S > routing.get("attn_chunk_min")
    cfg = _cfg()
    torch.manual_seed(0)
    import gc
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    m = build_model(cfg).cuda().to(torch.bfloat16).train()
    b = _batch(cfg, B=1, S=S, T=16)
    b["attention_mask"][0, -1000:] = 0
    calls = _spy(monkeypatch)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    out = m(**b)
    out.loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    enc = [c for c in calls if c[2] not in (None, -1)]
    assert enc == [("attn_hd_fwd", S, 128, True)] * cfg.num_layers, calls
    assert not [c for c in calls if c[0] == "attn_hd_fwd" and c not in enc], calls
    assert calls.count(("attn_fwd", 2, None, False)) == cfg.num_layers  # the global rows, against all 12288 keys
    print(f"[led 12K] peak {peak / 2**20:.1f} MiB above {base / 2**20:.1f} MiB")
    assert peak < cfg.num_heads * S * S * 2, peak
    assert torch.isfinite(out.loss).item()
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad.float()).all(), n
