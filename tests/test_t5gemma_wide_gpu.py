"""T5Gemma at head dim 256 with 2 K/V heads for 4 query heads — the shape class of the 2b-2b / 9b-9b checkpoints — on
csrc/attn_wide.hip: bf16 on the kernels against the fp32 torch reference path on the same weights, with the method and
bounds of tests/test_t5gemma_gpu.py test_t5gemma_matches_fp32_reference (whose two helpers are copied here)."""
import logging
import os

import pytest
import torch

from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.models import PRESETS, build_model
from distributed_llms_example_amd.ops.rng import manual_seed

pytestmark = pytest.mark.gpu


def _cfg():
    return PRESETS["t5gemma-tiny"].replace(d_model=256, d_kv=256, d_ff=512, vocab_size=4096, num_heads=4, num_kv_heads=2,
                                           query_pre_attn_scalar=256, attn_logit_softcapping=5.0,
                                           final_logit_softcapping=3.0)


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


def _grad_report(m_test, m_ref):
    rep = []
    for (n, pt), (_, pr) in zip(m_test.named_parameters(), m_ref.named_parameters()):
        if pr.grad is None or pr.grad.norm() == 0:
            continue
        gt, gr = pt.grad.float().flatten(), pr.grad.float().flatten()
        rep.append((((gt - gr).norm() / gr.norm()).item(),
                    torch.nn.functional.cosine_similarity(gt, gr, dim=0).item(), n))
    return rep


def _spy(monkeypatch):
    calls, real = [], _ext.native()

    class Spy:
        def __getattr__(self, n):
            f = getattr(real, n)
            if not (n.startswith("attn") and n.endswith("fwd")):
                return f

            def g(*a, **kw):
                calls.append((n, a[0].shape[1], a[9] if len(a) > 9 else None, kw.get("softcap"), a[1].shape[2]))
                return f(*a, **kw)
            return g

    monkeypatch.setattr(_ext, "native", lambda: Spy())
    return calls


def test_t5gemma_head_dim_256_grouped_matches_fp32_reference(monkeypatch, caplog):
    cfg = _cfg()
    torch.manual_seed(0)
    m32 = _reinit(build_model(cfg)).cuda().train()
    m16, t16 = (build_model(cfg).cuda() for _ in range(2))
    for m in (m16, t16):
        m.load_state_dict(m32.state_dict())
    m16, t16 = m16.to(torch.bfloat16).train(), t16.to(torch.bfloat16).train()
    g = torch.Generator().manual_seed(0)
    ids, lab = (torch.randint(3, cfg.vocab_size, (4, n), generator=g) for n in (150, 16))
    am = torch.ones(4, 150, dtype=torch.long)
    am[1, 100:], ids[1, 100:], lab[-1, -5:] = 0, cfg.pad_token_id, -100
    b = {k: v.cuda() for k, v in dict(input_ids=ids, attention_mask=am, labels=lab).items()}
    os.environ["DLLM_REFERENCE_OPS"] = "1"
    try:
        manual_seed(5)
        ref = m32(**b)
        ref.loss.backward()
        manual_seed(5)
        t16(**b).loss.backward()
    finally:
        os.environ.pop("DLLM_REFERENCE_OPS")
    calls = _spy(monkeypatch)
    manual_seed(5)
    with caplog.at_level(logging.WARNING):
        out = m16(**b)
        out.loss.backward()
    assert "running the composite" not in caplog.text
    w = ("attn_wide_fwd", 150, -1, cfg.attn_logit_softcapping, 2)  # encoder: sliding (window 4), full; decoder: 2 x 2
    assert calls == [w[:2] + (4,) + w[3:], w] + [w[:1] + (16,) + w[2:]] * 4, calls
    assert abs(out.loss.item() - ref.loss.item()) < 0.01 * ref.loss.item(), (out.loss.item(), ref.loss.item())
    rep = _grad_report(m16, m32)
    floor = {n: (rel, cos) for rel, cos, n in _grad_report(t16, m32)}
    bad = [(n, rel, floor[n][0], cos, floor[n][1]) for rel, cos, n in rep
           if rel > max(3e-2, 1.5 * floor[n][0]) or 1 - cos > max(1e-3, 1.5 * (1 - floor[n][1]))]
    print(f"[t5gemma wide parity] worst rel {max(rep)}; worst torch-bf16 rel {max(v[0] for v in floor.values()):.4f}")
    assert not bad, bad[:5]
    del calls[:]
    m16.eval()
    seq = m16.generate(b["input_ids"][:3], attention_mask=b["attention_mask"][:3], max_length=10, num_beams=3)
    assert seq.shape[0] == 3 and seq.shape[1] <= 10 and (seq[:, 0] == cfg.bos_token_id).all()
    assert {c[0] for c in calls} == {"attn_wide_fwd"} and all(c[4] == 2 for c in calls), calls
    assert len(calls) >= 2 + 2 * cfg.num_decoder_layers * (seq.shape[1] - 1), (len(calls), seq.shape)
