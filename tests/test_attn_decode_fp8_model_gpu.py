"""generate()'s FP8 cross-attention K/V at model level: the teacher-forced cached step of
tests/test_attn_decode_model_gpu.py with the projected encoder K/V quantised as ``cross_kv_dtype="fp8"`` does, against
the fp32 reference model; and generate() itself with the option."""
import copy

import pytest
import torch

from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.models import build_model, resolve_config
from distributed_llms_example_amd.models import generation as gen

pytestmark = pytest.mark.gpu
SRC = 50
# rel-L2 of the last hidden state against the fp32 reference model, FP8 arm: 2 x the value measured on the first run
# (seed-to-seed spread, and what tests/test_attn_decode_model_gpu.py allows itself): 1.051e-2 and 1.183e-2
BOUND = {"t5-base": 2.102e-2, "bart-base": 2.366e-2}


def _cached_step(m, ids, am, prefix, nb, fp8):
    cfg = m.config
    with torch.no_grad():
        enc = m.encode(ids, am)
        cross = m.project_cross_kv(enc)
        if fp8:
            cross = gen._quantize_cross(cross)
        H, D = gen._head_geom(m)
        store = gen.KVStore(cfg.num_decoder_layers, prefix.shape[0], 8, H, D, enc.dtype, ids.device, nb)
        for cur in range(1, prefix.shape[1] + 1):
            h = m.decode(prefix[:, cur - 1:cur], enc, am, caches=store.layers, q_offset=cur - 1, cross_kv=cross)
    return h[:, -1].double()


@pytest.mark.parametrize("name", ["t5-base", "bart-base"])
def test_fp8_cross_kv_cached_step_and_generate(name, monkeypatch):
    """Measured (MI355X, profiles/attn_decode_fp8.txt), rel-L2 of the last hidden state against the fp32 reference
    model, FP8 cross K/V / bf16 cross K/V: t5-base 1.051e-2 / 9.255e-3, bart-base 1.183e-2 / 1.074e-2."""
    cfg = resolve_config(name)
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
    prefix = torch.randint(3, cfg.vocab_size, (B * nb, 4), generator=g).cuda()
    prefix[:, 0] = cfg.decoder_start_token_id

    # the decoder receives float8_e4m3fn K/V, and the FP8 instantiation serves them
    real, seen = _ext.native(), []

    class Spy:
        def __getattr__(self, n):
            f = getattr(real, n)
            if n != "attn_decode":
                return f
            return lambda *a, **kw: (seen.append(a[1].dtype), f(*a, **kw))[1]

    monkeypatch.setattr(_ext, "native", lambda: Spy())
    got = _cached_step(m, ids, am, prefix, nb, True)
    monkeypatch.undo()
    assert seen.count(torch.float8_e4m3fn) == 4 * cfg.num_decoder_layers and torch.bfloat16 in seen, seen[:8]
    out = m.generate(ids, attention_mask=am, max_length=8, num_beams=nb, cross_kv_dtype="fp8")
    assert out.shape[0] == B and 1 < out.shape[1] <= 8
    with pytest.raises(ValueError, match="cross_kv_dtype"):
        m.generate(ids, attention_mask=am, max_length=8, cross_kv_dtype="int3")
    base = _cached_step(m, ids, am, prefix, nb, False)
    monkeypatch.setenv("DLLM_REFERENCE_OPS", "1")
    want = _cached_step(ref, ids, am, prefix, nb, False)
    monkeypatch.delenv("DLLM_REFERENCE_OPS")
    err, err_bf16 = (float((x - want).norm() / want.norm()) for x in (got, base))
    print(f"[attn_decode fp8 model {name}] err_fp8 {err:.3e} err_bf16 {err_bf16:.3e}")
    assert err < BOUND[name], (err, err_bf16)
