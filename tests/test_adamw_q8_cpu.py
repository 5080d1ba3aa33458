"""ops/q8.py and FusedAdamW8bit's composite on the CPU: code books, quantiser, relayout, checkpoint, state bytes."""
import copy

import numpy as np
import pytest
import torch

from distributed_llms_example_amd.models import build_model
from distributed_llms_example_amd.ops import q8
from distributed_llms_example_amd.ops.optim import FusedAdamW, FusedAdamW8bit, embedding_parameters
from distributed_llms_example_amd.parallel.flat import FlatParams
from distributed_llms_example_amd.train.checkpoint import load_checkpoint, save_checkpoint


@pytest.mark.parametrize("signed", [True, False])
def test_code_books_and_quantiser(signed):
    t = q8.SIGNED if signed else q8.UNSIGNED
    assert t.dtype == np.float32 and t.size == 256 and np.all(np.diff(t) > 0) and np.all(np.diff(q8.midpoints(t)) > 0)
    assert t[-1] == 1.0 and 0.0 in t
    if signed:
        assert abs(t[0] + 0.99297) < 1e-5 and -1.0 not in t and t[127] == 0.0
    else:
        assert t[0] == 0.0
    t = torch.from_numpy(t)
    # every entry times a scale returns its own code: 4 blocks of 64 entries, each block carrying 1.0 so absmax = scale
    scale = 3.7e-3
    x = t.clone().reshape(4, 64)
    x[:, 0] = 1.0
    codes, absmax = q8.quantize((x * scale).reshape(-1), signed)
    want = torch.arange(256).reshape(4, 64)
    want[:, 0] = 255
    assert torch.equal(codes.long(), want) and torch.all(absmax == np.float32(scale))
    assert torch.equal(q8.dequantize(codes, absmax, signed).reshape(4, 64), t[want] * absmax[:, None])
    # a value exactly on a midpoint gets the lower code (absmax = 1: the division is exact)
    mid = torch.from_numpy(q8.midpoints(t.numpy()))
    x = torch.cat([mid, torch.ones(1)]).reshape(4, 64)
    x[:, 0] = 1.0
    want = torch.cat([torch.arange(255), torch.tensor([255])]).reshape(4, 64)
    want[:, 0] = 255
    assert torch.equal(q8.quantize(x.reshape(-1), signed)[0].long(), want)
    # a zero block gets the code of 0.0 and a zero scale
    codes, absmax = q8.quantize(torch.zeros(64), signed)
    assert torch.all(t[codes.long()] == 0.0) and absmax.item() == 0.0


class _Net(torch.nn.Module):
    """An embedding (fp32 by ownership), two quantised matrices (one ends in a partial block), small biases (fp32)."""

    def __init__(self):
        super().__init__()
        self.emb = torch.nn.Embedding(50, 96)
        self.a = torch.nn.Linear(96, 96)
        self.b = torch.nn.Linear(96, 67)


def _set_grads(flat, seed):
    for s, p in zip(flat.segments, flat.params):
        g = torch.Generator().manual_seed(1000 * seed + sum(map(ord, s.name)))
        p._dllm_gbuf.copy_(torch.randn(p.shape, generator=g) * 10.0 ** torch.randint(-4, 0, p.shape, generator=g))


def _opt(net, **kw):
    flat = FlatParams(net)
    return flat, FusedAdamW8bit(flat, lr=1e-2, weight_decay=0.1, no_decay=lambda n: n.endswith("bias"),
                                keep_fp32=embedding_parameters(net).__contains__, **kw)


def _canonical_state(o):
    sd = o.state_dict()
    return [sd[k] for k in ("code_m", "code_v", "absmax_m", "absmax_v", "side_m", "side_v", "master")] + \
           [o.flat.to_canonical(o.flat.param_buf)]


def test_relayout_moves_whole_blocks():
    torch.manual_seed(0)
    n1 = _Net()
    n2 = copy.deepcopy(n1)
    (f1, o1), (f2, o2) = _opt(n1, master_weights=True), _opt(n2, master_weights=True)
    assert set(o1.fp32_slots) == {"emb.weight", "a.bias", "b.bias"} and (o1.slots < 0).any()
    for step in range(3):
        if step == 2:
            f2.relayout([3, 0, 4, 2, 1])
            assert [s.name for s in f2.segments] != f2.canonical
        for f, o in ((f1, o1), (f2, o2)):
            _set_grads(f, step)
            o.step()  # no global-norm clip: its reduction order follows the layout
    assert len(torch.unique(o1.code_m)) > 64  # codes of several decades occur
    for a, b in zip(_canonical_state(o1), _canonical_state(o2)):
        assert torch.equal(a, b)
    for (n, a), (_, b) in zip(sorted(n1.named_parameters()), sorted(n2.named_parameters())):
        assert torch.equal(a, b), n
    # state_bytes: master 4n, codes 2n, scales 8n / 64, slots 4n / 64, the side store, the mask
    n, side = f1.numel, sum((p.numel() + 63) // 64 * 64 for p in (n1.emb.weight, n1.a.bias, n1.b.bias))
    assert o1.wd_mask is not None and o1.side_m.numel() == side
    assert o1.state_bytes() == 4 * n + 2 * n + 8 * n // 64 + 4 * n // 64 + 8 * side + n


def test_checkpoint_round_trip_is_exact(tmp_path):
    torch.manual_seed(0)
    m1 = build_model("t5-tiny")
    m2 = copy.deepcopy(m1)
    (f1, o1), (f2, o2) = _opt(m1), _opt(m2)
    assert (o1.slots >= 0).any() and (o1.slots < 0).any()
    for step in range(2):
        _set_grads(f1, step)
        o1.step(max_grad_norm=1.0)
    save_checkpoint(str(tmp_path), m1, o1)
    m2.load_state_dict(m1.state_dict())
    load_checkpoint(str(tmp_path), None, o2)
    assert o2.step_count == 2
    for f, o in ((f1, o1), (f2, o2)):
        _set_grads(f, 7)
        o.step(max_grad_norm=1.0)
    for a, b in zip(_canonical_state(o1)[:-2], _canonical_state(o2)[:-2]):
        assert torch.equal(a, b)
    assert torch.equal(f1.param_buf, f2.param_buf)
    adamw = FusedAdamW(FlatParams(build_model("t5-tiny")), lr=1e-2)
    with pytest.raises(ValueError, match="adamw_8bit"):
        load_checkpoint(str(tmp_path), None, adamw)
    with pytest.raises(ValueError, match="adamw"):
        o2.load_state_dict(adamw.state_dict())
