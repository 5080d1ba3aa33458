"""Whole models at head dims other than 64 on the GPU: the bf16 HIP-kernel path (attention on csrc/attn_hd.hip) against
the fp32 torch reference path on the same weights and dropout masks — the method of
tests/test_model_gpu.py::test_native_bf16_matches_fp32_reference, restated: the plain-torch composite run in bf16 sets
each parameter's noise floor, and the native path must stay within 1.5x of its relative error (floor 3e-2) and of its
cosine deficit (floor 1e-3)."""
import os

import pytest
import torch

from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.models import build_model, resolve_config
from distributed_llms_example_amd.ops import attention as A

pytestmark = pytest.mark.gpu


def _cfg(name):
    c = resolve_config(name)
    if c.model_type == "t5":  # head dim 128, as t5-3b / t5-11b
        return c.replace(num_layers=2, num_decoder_layers=2, vocab_size=4096, d_model=512, num_heads=4, d_kv=128,
                         d_ff=1024)
    # head dim 40, as the preset itself (1280 / 32); 200 source tokens need more than its 128 learned positions
    return c.replace(num_layers=2, num_decoder_layers=2, vocab_size=4096, d_model=320, num_heads=8, d_kv=40, d_ff=1280,
                     max_position_embeddings=256)


def _batch(cfg, B=4, S=200, T=40):
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, cfg.vocab_size, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    am[1, -33:] = 0
    lab = torch.randint(3, cfg.vocab_size, (B, T), generator=g)
    lab[2, -5:] = -100
    return {k: v.cuda() for k, v in dict(input_ids=ids, attention_mask=am, labels=lab).items()}


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


@pytest.mark.parametrize("name,head_dim", [("t5-base", 128), ("blenderbot-400m-distill", 40)])
def test_attn_hd_model_matches_fp32_reference(name, head_dim, monkeypatch):
    cfg = _cfg(name)
    assert cfg.d_kv == head_dim
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
    calls = []
    real = _ext.native()

    class Spy:
        def __getattr__(self, n):
            if n in ("attn_fwd", "attn_hd_fwd"):
                calls.append(n)
            return getattr(real, n)

    monkeypatch.setattr(A._ext, "native", lambda: Spy())
    manual_seed(5)  # same dropout masks on every path
    out = m16(**b)
    out.loss.backward()
    assert "attn_hd_fwd" in calls and "attn_fwd" not in calls, sorted(set(calls))
    assert abs(out.loss.item() - ref.loss.item()) < 0.01 * ref.loss.item(), (out.loss.item(), ref.loss.item())
    rep = _grad_report(m16, m32)
    floor = {n: (rel, cos) for rel, cos, n in _grad_report(t16, m32)}
    bad = []
    for rel, cos, n in rep:
        frel, fcos = floor[n]
        if rel > max(3e-2, 1.5 * frel) or 1 - cos > max(1e-3, 1.5 * (1 - fcos)):
            bad.append((n, rel, frel, cos, fcos))
    worst = max(rep)
    print(f"[attn_hd parity {name} D={head_dim}] worst rel {worst} (torch-bf16 floor {floor[worst[2]]}); "
          f"worst torch-bf16 rel {max(v[0] for v in floor.values()):.4f}")
    assert not bad, bad[:5]
