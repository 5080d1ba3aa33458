"""Cached generation on csrc/attn_decode.hip at model level: which bindings the decode steps call (a spy), and the
hidden state of a teacher-forced cached step against the fp32 reference model, route on against route off."""
import copy

import pytest
import torch

from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.models import PRESETS, build_model, resolve_config
from distributed_llms_example_amd.models import generation as gen
from distributed_llms_example_amd.ops import routing

pytestmark = pytest.mark.gpu
SRC = 50


def _config(name):
    if name != "t5gemma-gqa":
        return resolve_config(name)
    # t5gemma-tiny at head dim 64 with 2 K/V heads for 4 query heads (tests/test_t5gemma_gpu.py)
    return PRESETS["t5gemma-tiny"].replace(d_model=256, d_kv=64, d_ff=512, vocab_size=4096, query_pre_attn_scalar=64,
                                           attn_logit_softcapping=5.0, final_logit_softcapping=3.0, num_kv_heads=2)


def _spy(monkeypatch):
    """(binding, Sq) of every attention binding call, on every module that holds the native handle."""
    calls, real = [], _ext.native()

    class Spy:
        def __getattr__(self, n):
            f = getattr(real, n)
            if not (n.startswith("attn") and (n.endswith("_fwd") or n == "attn_decode")):
                return f

            def g(*a, **kw):
                calls.append((n, a[0].shape[1]))
                return f(*a, **kw)
            return g

    monkeypatch.setattr(_ext, "native", lambda: Spy())
    return calls


def _cached_step(m, ids, am, prefix, nb):
    """Last hidden state after feeding ``prefix`` [B * nb, T] one token at a time through the KV cache, the nb rows of
    a batch entry sharing its encoder K/V as in beam search."""
    cfg = m.config
    with torch.no_grad():
        enc = m.encode(ids, am)
        cross = m.project_cross_kv(enc)
        H, D = gen._head_geom(m)
        store = gen.KVStore(cfg.num_decoder_layers, prefix.shape[0], 8, H, D, enc.dtype, ids.device, nb)
        for cur in range(1, prefix.shape[1] + 1):
            h = m.decode(prefix[:, cur - 1:cur], enc, am, caches=store.layers, q_offset=cur - 1, cross_kv=cross)
    return h[:, -1].double()


@pytest.mark.parametrize("name", ["t5-base", "bart-base", "t5gemma-gqa"])
def test_decode_steps_run_attn_decode_and_keep_the_accuracy(name, monkeypatch):
    """Measured (MI355X, profiles/attn_decode.txt), rel-L2 of the last hidden state against the fp32 reference model,
    route on / off: see the profile's "accuracy" table."""
    cfg = _config(name)
    torch.manual_seed(0)
    ref = build_model(cfg).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.to(torch.bfloat16).float())  # exactly representable in bf16: the comparison measures compute
    ref = ref.cuda()
    m = copy.deepcopy(ref).to(torch.bfloat16)
    g = torch.Generator().manual_seed(1)
    B, nb = 3, 2
    ids = torch.randint(3, cfg.vocab_size, (B, SRC), generator=g).cuda()
    am = torch.ones_like(ids)
    am[1, 30:] = 0
    am[2, 41:] = 0
    ids[am == 0] = cfg.pad_token_id

    # ---- the spy: greedy and 2 beams
    per_step = 2 * cfg.num_decoder_layers
    for beams in (1, nb):
        calls = _spy(monkeypatch)
        out = m.generate(ids, attention_mask=am, max_length=8, num_beams=beams)
        monkeypatch.undo()
        enc_on = [c for c in calls if c[0] != "attn_decode"]
        dec_on = [c for c in calls if c[0] == "attn_decode"]
        assert all(sq == SRC for _, sq in enc_on), enc_on  # no training forward at Sq <= nb: the encoder's calls only
        assert dec_on and len(dec_on) % per_step == 0 and {sq for _, sq in dec_on} <= {1, beams}, dec_on[:8]
        assert sum(sq == beams for _, sq in dec_on) >= len(dec_on) // 2  # the shared cross-attention: Sq = nb
        calls = _spy(monkeypatch)
        monkeypatch.setenv("DLLM_ROUTE", routing.merged(attn_decode=0))
        off = m.generate(ids, attention_mask=am, max_length=8, num_beams=beams)
        monkeypatch.undo()
        assert not any(c[0] == "attn_decode" for c in calls)
        assert [c for c in calls if c[1] == SRC] == enc_on  # the encoder's calls are unchanged
        assert out.shape[0] == off.shape[0] == B

    # ---- accuracy of one teacher-forced cached step against the fp32 reference model
    prefix = torch.randint(3, cfg.vocab_size, (B * nb, 4), generator=g).cuda()
    prefix[:, 0] = cfg.decoder_start_token_id
    monkeypatch.setenv("DLLM_REFERENCE_OPS", "1")
    want = _cached_step(ref, ids, am, prefix, nb)
    monkeypatch.delenv("DLLM_REFERENCE_OPS")
    err = {}
    for route in (1, 0):
        monkeypatch.setenv("DLLM_ROUTE", routing.merged(attn_decode=route))
        got = _cached_step(m, ids, am, prefix, nb)
        err[route] = float((got - want).norm() / want.norm())
    print(f"[attn_decode model {name}] err_on {err[1]:.3e} err_off {err[0]:.3e}")
    assert err[1] <= 2 * err[0], err
