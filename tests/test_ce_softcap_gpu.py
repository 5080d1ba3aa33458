"""The cross-entropy kernels with a soft cap (csrc/ce.hip ``ce_fwd`` / ``ce_bwd`` / ``ce_chunk_fwd`` / ``ce_chunk_bwd``
with ``softcap``) and the capped ``cross_entropy`` / ``lm_head_loss`` on the GPU: the method and bounds of
tests/test_loss_kernels_gpu.py, with the cap added to an fp64 reference written here (tests/loss_refs.py is not edited).

Reference: ``x' = c tanh(x / c)`` in fp64 of the logits as stored, then ``loss_refs.ce_ref`` on ``x'``; the gradient is
``d' (1 - tanh^2)``.  Bounds: loss and lse per row ``loss_refs.LOSS_BOUND``; gradient elements ``BF16_REL |ref| +
abs_term`` (bf16 store) or ``abs_term`` (fp32 store) with ``abs_term`` from the fp32 error model of ``_capped_abs_term``.
Logits are scaled so that half of them lie beyond the cap (asserted), labels walk ``loss_refs.edge_labels`` (ignored and
out-of-range rows among them), label smoothing is 0 and 0.1."""
import pytest
import torch

import loss_refs as L
import rowwise_refs as R
from distributed_llms_example_amd import _ext
from distributed_llms_example_amd.ops import cross_entropy as CE
from distributed_llms_example_amd.ops import lm_head as LM
from distributed_llms_example_amd.ops import routing

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF16, "fp32": F32}
IGN = L.IGNORE
GS = 0.375  # the gradient scale g: exact in fp32
CAP = 30.0  # Gemma 2's final_logit_softcapping
TANH_ULPS = 8.0  # allowance for the device library's tanhf (documented to 2 ulp = 4 u), in units of U32, as EXP_ULPS


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _scale():
    return torch.full((1,), GS, device=DEV, dtype=F32)


def _half_saturated(N, V, gen, c=CAP):
    """fp32 [N, V] ~ N(0, (c / 0.6745)^2): half of the logits beyond the cap; a few peak columns boosted."""
    x = (c / 0.6745) * torch.randn(N, V, device=DEV, generator=gen)
    x[:, L.peak_columns(V)] += 0.5 * c
    return x


def _capped_ref(x, labels, eps, V, g, c=CAP):
    """(loss_rows, lse, dlogits, x', 1 - tanh^2) in fp64 of the logits as given."""
    t = torch.tanh(x.double() / c)
    xc = c * t
    loss, lse, d = L.ce_ref(xc, labels, None, eps, IGN, V, g)
    return loss, lse, d * (1.0 - t * t), xc, 1.0 - t * t


def _capped_abs_term(x, labels, eps, V, g, c=CAP):
    """Per-element fp32 evaluation error of ``g (exp(x' - lse) - eps / V - (1 - eps) [v == y]) (1 - t^2)`` with
    ``t = tanh(x / c)``, ``x' = c t``, u = 2^-24, on top of loss_refs.ce_abs_term's model E' for the bracket given an
    exact x':

      x' in fp32:   x / c (as x * fl(1 / c)) carries 2 u |x / c|, which tanh turns into 2 u |x / c| (1 - t^2); tanhf
                    itself TANH_ULPS u |t|; the product with c one more u |t|:  dx' = c u (2 |x / c| (1 - t^2) +
                    (TANH_ULPS + 1) |t|), which exp turns into  |g| p dx'
      1 - t^2:      t^2 carries (2 TANH_ULPS + 1) u t^2, the subtraction u:  dd = (2 TANH_ULPS + 2) u
      the product:  E' (1 - t^2) + |bracket| dd + one rounding u |ref|

    all under the same COMP_MARGIN = 4 as the model it extends."""
    xd = x.double()
    t = torch.tanh(xd / c)
    xc, dt = c * t, 1.0 - t * t
    base = L.ce_abs_term(xc, labels, None, eps, IGN, V, g)  # holds COMP_MARGIN already
    lse = torch.logsumexp(xc, dim=1).view(-1, 1)
    p = torch.exp(xc - lse)
    _, _, d = L.ce_ref(xc, labels, None, eps, IGN, V, g)
    dx = c * L.U32 * (2.0 * (xd / c).abs() * dt + (TANH_ULPS + 1.0) * t.abs())
    extra = abs(float(g)) * p * dx * dt + d.abs() * (2.0 * TANH_ULPS + 2.0) * L.U32 + L.U32 * (d * dt).abs()
    valid = L.valid_rows(labels, IGN, V).view(-1, 1)
    return torch.where(valid, base * dt + L.COMP_MARGIN * extra, torch.full_like(base, 5e-324))


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("N,V", [(300, 512), (70, 50265)])
def test_ce_fwd_bwd_capped(N, V, dt):
    C, dtype = _ext.native(), DT[dt]
    F = L.Figures(f"capped ce [{N}, {V}] {dt}")
    gen = _gen(V + N)
    x = _half_saturated(N, V, gen).to(dtype)
    frac = (x.float().abs() > CAP).float().mean().item()
    assert 0.4 < frac < 0.6, frac
    labels = L.edge_labels(N, V, DEV, gen)
    for eps in (0.0, 0.1):
        case = f"eps={eps}"
        loss_r, lse_r, d_r, _, _ = _capped_ref(x, labels, eps, V, GS)
        abs_term = _capped_abs_term(x, labels, eps, V, GS)
        loss, lse = C.ce_fwd(x, labels, None, eps, IGN, softcap=CAP)
        F.fold("lse per row", L.row_metric(lse, lse_r), L.LOSS_BOUND, case)
        F.fold("loss per row", L.row_metric(loss, loss_r), L.LOSS_BOUND, case)
        inv = ~L.valid_rows(labels, IGN, V)
        F.check(f"[{case}] rows with an ignored / out-of-range label: loss exactly 0", not loss[inv].any())
        lse32 = lse_r.float()
        out = C.ce_bwd(_scale(), x, labels, lse32, None, eps, IGN, False, softcap=CAP)
        worst, where = L.grad_worst(out, d_r, L.grad_bound(d_r, abs_term, dtype))
        F.fold("dlogits out of place", worst, 1.0, f"{case} {where['row']},{where['col']}")
        xi = x.clone()
        res = C.ce_bwd(_scale(), xi, labels, lse32, None, eps, IGN, True, softcap=CAP)
        F.check(f"[{case}] in place: same storage", res.data_ptr() == xi.data_ptr())
        worst, where = L.grad_worst(xi, d_r, L.grad_bound(d_r, abs_term, dtype))
        F.fold("dlogits in place", worst, 1.0, f"{case} {where['row']},{where['col']}")
        F.check(f"[{case}] ignored rows: gradient exactly 0", not xi[inv].any())
        # the cap is what is tested: the uncapped loss of these logits is far away
        plain, plain_lse = C.ce_fwd(x, labels, None, eps, IGN)
        F.check(f"[{case}] the cap bites", (plain - loss)[~inv].abs().mean().item() > 1.0)
        # without a cap: bit for bit the call without the argument
        p0, l0 = C.ce_fwd(x, labels, None, eps, IGN, softcap=0.0)
        F.check(f"[{case}] softcap=0 is the uncapped call", torch.equal(p0, plain) and torch.equal(l0, plain_lse))
    F.done()


def test_cross_entropy_op_capped():
    """The autograd op: loss and in-place gradient against the fp64 reference; ``softcap=None`` is the call without it."""
    N, V = 300, 512
    gen = _gen(5)
    x = _half_saturated(N, V, gen).to(BF16)
    labels = L.edge_labels(N, V, DEV, gen).clamp(-100, V - 1)
    labels[labels < 0] = IGN
    count = int((labels != IGN).sum())
    F = L.Figures("cross_entropy softcap")
    for eps in (0.0, 0.1):
        loss_r, _, d_r, _, _ = _capped_ref(x, labels, eps, V, 1.0 / count)
        xg = x.clone().requires_grad_(True)
        loss = CE.cross_entropy(xg, labels, label_smoothing=eps, softcap=CAP)
        loss.backward()
        ref = loss_r.sum().item() / count
        F.add(f"loss eps={eps}", abs(loss.item() - ref) / max(1.0, abs(ref)), L.LOSS_BOUND)
        abs_term = _capped_abs_term(x, labels, eps, V, 1.0 / count)
        worst, where = L.grad_worst(xg.grad, d_r, L.grad_bound(d_r, abs_term, BF16))
        F.add(f"dlogits eps={eps}", worst, 1.0)
        a = CE.cross_entropy(x, labels, label_smoothing=eps, softcap=None)
        b = CE.cross_entropy(x, labels, label_smoothing=eps)
        F.check("softcap=None is the call without it", torch.equal(a, b), quiet=False)
    F.done()


class _Spy:
    """The native module with the called bindings recorded as (name, softcap keyword or None)."""

    def __init__(self, calls, real):
        self.calls, self.real = calls, real

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not callable(fn):
            return fn

        def wrapped(*a, **k):
            self.calls.append((name, k.get("softcap")))
            return fn(*a, **k)
        return wrapped


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_lm_head_loss_capped_is_chunked(eps, monkeypatch):
    """V = 1003, N = 130 in 256-column chunks (four, the last ragged) with ``lmhead`` = fused: a capped call must not
    take the GEMM epilogues (they have no cap) but the vocabulary chunks, every one with the cap; loss, dh per row and
    dW per row of [V, d] against fp64 of the same bf16 operands.  The same call without a cap takes the epilogues."""
    N, d, V, c = 130, 128, 1003, 3.0
    F = L.Figures(f"lm_head_loss softcap eps={eps}")
    gen = _gen(41)
    h = torch.randn(N, d, device=DEV, generator=gen).to(BF16)
    w = (torch.randn(V, d, device=DEV, generator=gen) * (c / 0.6745) * d ** -0.5).to(BF16)  # logits ~ N(0, (c / .67)^2)
    labels = L.edge_labels(N, V, DEV, gen)
    labels[3], labels[5] = IGN, IGN
    labels[9:13] = torch.tensor([762, 763, 767, 768], device=DEV)
    count = int((labels != IGN).sum().item())
    h64, w64 = h.double(), w.double()
    logits = h64 @ w64.t()
    frac = (logits.abs() > c).double().mean().item()
    assert 0.4 < frac < 0.6, frac
    loss_r, _, dl, _, _ = _capped_ref(logits, labels, eps, V, 1.0 / count, c)
    dh_r, dw_r = dl @ w64, dl.t() @ h64
    monkeypatch.setenv("DLLM_ROUTE", routing.merged(lmhead_chunk_mb=0.07, lmhead="fused"))
    assert LM._chunk_cols(N, V) == 256
    chunks = LM._chunks(V, 256)
    calls = []
    spy = _Spy(calls, _ext.native())
    monkeypatch.setattr(LM._ext, "native", lambda: spy)
    hg, wg = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    loss = LM.lm_head_loss(hg, wg, labels, label_smoothing=eps, ignore_index=IGN, softcap=c)
    loss.backward()
    names = [n for n, _ in calls]
    assert names.count("ce_chunk_fwd") == len(chunks) and names.count("ce_chunk_bwd") == len(chunks), calls
    assert "lmhead_ce_fwd" not in names and "lmhead_ce_bwd_slice" not in names, calls
    assert all(cap == c for n, cap in calls if n.startswith("ce_chunk")), calls
    ref = loss_r.sum().item() / count
    F.add("loss", abs(loss.item() - ref), 2e-3 * max(1.0, abs(ref)))
    F.add("dh per row", R.row_err(hg.grad, dh_r), R.ROW_BOUND[BF16])
    F.add("dW per row of [V, d]", R.row_err(wg.grad, dw_r), R.ROW_BOUND[BF16])
    del calls[:]
    plain = LM.lm_head_loss(h, w, labels, label_smoothing=eps, ignore_index=IGN)
    assert [n for n, _ in calls] == ["lmhead_ce_fwd"], calls
    F.check("the cap bites", abs(plain.item() - loss.item()) > 0.1, quiet=False)
    F.done()
