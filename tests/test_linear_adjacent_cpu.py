"""ops/linear.py ``_adjacent``: several tensors as ONE view only when they are slices of one storage.

Parameters of a model outside FlatParams each own a storage; the allocator may place two of them back to back (two
2 KiB biases, for instance).  Equal addresses alone once made ``_adjacent`` build a view of the first tensor that
reached past its storage, and ``stacked_linear`` raised from ``as_strided``."""
import numpy as np
import torch

from distributed_llms_example_amd.ops.linear import Linear, _adjacent, stacked_linear


def _back_to_back(rows, cols):
    """Two tensors at adjacent addresses, each with a storage of its own."""
    a = np.arange(2 * rows * cols, dtype=np.float32)
    t0, t1 = torch.from_numpy(a[:rows * cols]).view(rows, cols), torch.from_numpy(a[rows * cols:]).view(rows, cols)
    assert t1.data_ptr() == t0.data_ptr() + t0.numel() * 4
    assert t0.untyped_storage().data_ptr() != t1.untyped_storage().data_ptr()
    return t0, t1


def test_adjacent_needs_one_storage():
    t0, t1 = _back_to_back(4, 8)
    assert _adjacent([t0, t1]) is None
    b0, b1 = _back_to_back(1, 8)
    assert _adjacent([b0.view(8), b1.view(8)]) is None


def test_adjacent_views_of_one_buffer():
    buf = torch.arange(3 * 4 * 8, dtype=torch.float32)
    parts = [buf[i * 32:(i + 1) * 32].view(4, 8) for i in range(3)]
    v = _adjacent(parts)
    assert v is not None and v.shape == (12, 8) and v.data_ptr() == buf.data_ptr()
    assert torch.equal(v, buf.view(12, 8))
    assert _adjacent([parts[0], parts[2]]) is None  # a gap
    assert _adjacent([parts[1], parts[0]]) is None  # out of order
    assert _adjacent([parts[0], parts[1].double()]) is None


def test_stacked_linear_on_back_to_back_parameters():
    """The whole path: layers whose weights and biases sit next to each other without sharing a storage."""
    w0, w1 = _back_to_back(6, 8)
    b0, b1 = _back_to_back(1, 6)
    mods = []
    for w, b in ((w0, b0), (w1, b1)):
        m = Linear(8, 6)
        m.weight.data, m.bias.data = w.mul_(1e-2), b.view(6).mul_(1e-2)  # in place: the storages stay where they are
        mods.append(m)
    assert mods[1].weight.data_ptr() == mods[0].weight.data_ptr() + mods[0].weight.numel() * 4
    x = torch.randn(2, 5, 8, requires_grad=True)
    outs = stacked_linear(x, mods, (2, 5, 6))
    for m, o in zip(mods, outs):
        torch.testing.assert_close(o, m(x))
    with torch.no_grad():
        outs = stacked_linear(x, mods, (2, 5, 6))
    for m, o in zip(mods, outs):
        torch.testing.assert_close(o, torch.nn.functional.linear(x, m.weight, m.bias))
