"""The one-pass cross-attention backward (csrc/attn.hip attn_bwd_dkdv_sq_kernel, DQ arm: dQ folded into the short-query
dK/dV kernel, no dQ kernel launch) against the fp64 reference of tests/attn_refs.py, with the per-row error measure,
the zero checks and the bounds of tests/test_attn_rows_gpu.py (4 x the bf16 model's error on the same inputs), imported
from there.

Per shape (D = 64, B = 2, H = 2; Sq 1 / 64 / 65 / 128: one stage, a full stage, one row into the second, two full
stages; Sk 256 / 320 / 1024: 2 blocks, 3 with a ragged last one, 8), with and without key padding (each batch row has
one fully padded and one partly padded 128-key block) and dropout (keep planes from the forward):

* dq, dk, dv (and o) of the one-pass arm per row against the reference;
* dk and dv bit-equal between the one-pass arm and the split arm (``attn_sq_onepass=0``: dQ kernel + MB = 4 kernel) —
  the one-pass arm leaves the dK / dV arithmetic and its delta / lse row terms as they were;
* with csq / csk / csv: outputs unchanged bit for bit, every partial row written, column sums against the reference;
* K / V as column slices of a stacked [B * Sk, L * 2 * H * D] projection output and dK / dV written into the matching
  slices of its gradient buffer (the hand-off the models use): bit-equal to the contiguous call, other columns
  untouched.

``attn_dkdv_sq_force=1`` takes the short-query path at this small B x H; which arm a call takes cannot be observed from
Python, ``_onepass`` mirrors the launcher's rule and the unforced test sizes B x H from the device's CU count.
"""
import pytest
import torch

import attn_refs as R
import test_attn_rows_gpu as T
from distributed_llms_example_amd.ops import routing

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUTS = T.OUTS


def _onepass(c, force, route=1):
    """Mirrors csrc/attn.hip dllm_attn_bwd: ``sq_shape = lut == nullptr && !causal && Sq <= 2 * K2_QT && n_kblocks >=
    2`` and ``onepass = sq_shape && attn_sq_onepass != 0 && (force || H * B >= 6 * cus)`` (column sums all or none)."""
    return (not c.bias and not c.causal and c.Sq <= 128 and T._cdiv(c.Sk, 128) >= 2 and route != 0
            and (force or c.B * c.H >= 6 * T._cus()))


def _route(monkeypatch, force, onepass):
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(attn_dkdv_sq_force=1 if force else 0,
                                                    attn_sq_onepass=1 if onepass else 0))


def _padding(B, Sk):
    """uint8 [B, Sk]: batch row 0 keeps a prefix that ends inside the second-to-last 128-key block (that block partly,
    the last one fully padded); the other rows lose the whole first block and the last 19 keys."""
    n = T._cdiv(Sk, 128)
    m = torch.ones(B, Sk, dtype=torch.uint8)
    m[0, 128 * (n - 2) + 72:] = 0
    m[1:, :128] = 0
    m[1:, Sk - 19:] = 0
    return m


_built = {}


def _case(Sq, Sk, pad, p, B=2, H=2):
    """(case, inputs on the GPU, fp64 reference, the bf16 model's figures): built once per shape and left unchanged."""
    key = (Sq, Sk, pad, p, B, H)
    if key not in _built:
        c = R.case(Sq, Sk, B=B, H=H, kpm="blocks" if pad else None, p=p)
        c.kpm = None  # make_case draws no mask; the padding of this file is put in below
        r = R.make_case(c)
        c.kpm = "blocks" if pad else None
        if pad:
            r.kpm = _padding(B, Sk)
        r = R.to_device(r, DEV)
        ref, fig = R.ref_and_figures(r)
        _built[key] = (c, r, ref, fig)
    return _built[key]


def _rows(F, got, ref, fig):
    for n in OUTS:
        F.add(n, R.row_err(getattr(got, n), getattr(ref, n)), R.MODEL_FACTOR * fig[n], fig[n])
    T._check_zeros(F, ref, got)


SHAPES = [(sq, sk) for sq in (1, 64, 65, 128) for sk in (256, 320, 1024)]


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop"])
@pytest.mark.parametrize("pad", [False, True], ids=["nopad", "pad"])
@pytest.mark.parametrize("Sq,Sk", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_onepass_rows_and_split_arm(Sq, Sk, pad, p, monkeypatch):
    """dq / dk / dv of the one-pass arm per row against the fp64 reference; dk / dv bit-equal with the split arm."""
    c, r, ref, fig = _case(Sq, Sk, pad, p)
    F = T.Figures(f"onepass {R.case_id(c)}")
    _route(monkeypatch, True, True)
    assert _onepass(c, True)
    one = T._kernel(r)
    _rows(F, one, ref, fig)
    _route(monkeypatch, True, False)
    assert not _onepass(c, True, route=0) and T._sq_mb(c, True) == 4
    split = T._kernel(r)
    F.tag = f"split {R.case_id(c)}"
    _rows(F, split, ref, fig)
    for n in ("dk", "dv"):
        F.check(f"{n} bit-equal between the one-pass and the split arm",
                torch.equal(getattr(one, n), getattr(split, n)))
    F.done()


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop"])
@pytest.mark.parametrize("pad", [False, True], ids=["nopad", "pad"])
@pytest.mark.parametrize("Sq,Sk", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_onepass_column_sums(Sq, Sk, pad, p, monkeypatch):
    """csq / csk / csv set (BART's q / k / v projection bias gradients): the outputs do not change, every partial row is
    written, the sums meet the reference's within the model's bound."""
    c, r, ref, fig = _case(Sq, Sk, pad, p)
    F = T.Figures(f"onepass-cs {R.case_id(c)}")
    _route(monkeypatch, True, True)
    HD, nk = c.H * 64, c.B * T._cdiv(Sk, 128)
    csq = torch.full((c.B, HD), float("nan"), device=DEV)
    pkv = torch.full((nk, 2 * HD), float("nan"), device=DEV)  # dK | dV halves of one buffer, as ops/attention.py passes
    plain = T._kernel(r)
    got = T._kernel(r, cs=(csq, pkv[:, :HD], pkv[:, HD:]))
    for n in OUTS:
        F.check(f"{n} bit-equal with and without the column sums", torch.equal(getattr(got, n), getattr(plain, n)))
    for n, part in (("cs_dq", csq), ("cs_dk", pkv[:, :HD]), ("cs_dv", pkv[:, HD:])):
        F.check(f"{n}: every partial row written", bool(torch.isfinite(part).all()))
        F.add(n, R.mass_err(part.double().sum(0), getattr(ref, n), getattr(ref, n + "_mass")), R.MODEL_FACTOR * fig[n],
              fig[n])
    F.done()


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop"])
@pytest.mark.parametrize("pad", [False, True], ids=["nopad", "pad"])
@pytest.mark.parametrize("Sq,Sk", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_onepass_stacked_kv(Sq, Sk, pad, p, monkeypatch):
    """K / V of layer 1 of 3 as column slices of a stacked [B * Sk, L * 2 * H * D] tensor, dK / dV into the matching
    slices of a gradient buffer of that shape: the same bits as the contiguous call, nothing else written."""
    c, r, ref, fig = _case(Sq, Sk, pad, p)
    _route(monkeypatch, True, True)
    L, lay, HD = 3, 1, c.H * 64
    big = torch.randn(c.B * Sk, L * 2 * HD, device=DEV).to(torch.bfloat16)
    view = lambda t, j: t.view(c.B, Sk, L, 2, c.H, 64)[:, :, lay, j]
    view(big, 0).copy_(r.k)
    view(big, 1).copy_(r.v)
    gbig = torch.full_like(big, 7.0)
    plain = T._kernel(r)
    got = T._kernel(r, outs=(None, view(gbig, 0), view(gbig, 1)), kv=(view(big, 0), view(big, 1)))
    F = T.Figures(f"onepass-stacked {R.case_id(c)}")
    for n in OUTS:
        F.check(f"{n} bit-equal with the contiguous call", torch.equal(getattr(got, n), getattr(plain, n)))
    F.check("dk / dv landed in the stacked gradient's slices",
            torch.equal(view(gbig, 0), plain.dk) and torch.equal(view(gbig, 1), plain.dv))
    other = torch.ones(L * 2 * HD, dtype=torch.bool, device=DEV)
    other[lay * 2 * HD:(lay + 1) * 2 * HD] = False
    F.check("the other layers' columns untouched", bool((gbig[:, other] == 7.0).all()))
    _rows(F, got, ref, fig)
    F.done()


def test_onepass_unforced(monkeypatch):
    """The production route, no override: B x H = 6 x CUs (the smallest launch that takes the one-pass arm), 100 x 320
    with padding and dropout, against the reference; one batch row less stays on the split arm."""
    _route(monkeypatch, False, True)
    H = 16
    B = T._cdiv(6 * T._cus(), H)
    c, r, ref, fig = _case(100, 320, True, 0.1, B=B, H=H)
    assert _onepass(c, False)
    assert not _onepass(R.case(100, 320, B=B - 1, H=H), False)
    F = T.Figures(f"onepass-unforced {R.case_id(c)}")
    _rows(F, T._kernel(r), ref, fig)
    F.done()
    del _built[(100, 320, True, 0.1, B, H)]  # the large reference is not kept
