"""Fused multi-head attention for encoder-decoder models (flash-style, HIP/MFMA on gfx950).

One op covers every attention variant the reference's models run (SURVEY.md §2.3 "SDPA attention"):

* T5 self-attention: no 1/sqrt(d) scale (transformers modeling_t5.py:196-197) and an additive
  relative-position bias built from a (num_buckets, H) table (modeling_t5.py:217-279).  HF
  materialises the bias as a float ``[1, H, Sq, Sk]`` mask, which also knocks SDPA off its flash path
  (integrations/sdpa_attention.py:39-76).  Here the bias is a per-head LUT indexed by the relative
  distance ``j - i`` (``[H, Sq + Sk - 1]``, O(S) memory) that the kernel reads from LDS; its
  backward returns the gradient of that LUT (diagonal sums of dS), which autograd scatters back
  into the bucket table.
* T5 / BART decoder: causal (+ bias); cross-attention: key-padding mask only.
* BART: scale ``d**-0.5`` (modeling_bart.py:169), key-padding mask.
* Attention-probability dropout (T5 applies ``dropout_rate`` to the probabilities,
  modeling_t5.py:360) with the counter-based mask of ops/rng.py, regenerated in backward.

Layout: q ``[B, Sq, H, D]``, k/v ``[B, Sk, H, D]`` — the natural output of the fused QKV GEMM
viewed without any transpose copy (only the last dim must be contiguous).  Output ``[B, Sq, H, D]``.

Kernels: csrc/attn.hip (bf16, head dim 64: forward; backward = dQ kernel + dK/dV kernel, no atomics except the bias
LUT), csrc/attn_hd.hip (bf16, every other head dim 32 .. 128 that is a multiple of 8: the same op templated on the
padded head dim) and csrc/attn_f32.hip (fp32 at head dim 64, the reference's own precision: the same op on the
f32-input matrix cores).  All are O(S) memory.  ``_route`` picks one; what none serves takes the O(Sq·Sk) composite.

Sliding window (LongT5-local encoder self-attention): ``window=w`` keeps key ``j`` for query ``i`` only when
``|j - i| <= w`` (``Sq == Sk``, not causal).  csrc/attn_hd.hip (bf16, head dim 64 included) and csrc/attn_f32.hip skip
the key blocks outside the band, O(S·w) work; csrc/attn.hip has no window.  The composite masks a full score matrix.

Segments (sequence packing, data/packing.py): ``q_segments`` ``[B, Sq]`` and ``k_segments`` ``[B, Sk]`` integer ids,
both or neither; key ``j`` is visible to query ``i`` only when ``k_segments[b, j] >= 0`` and the two ids are equal (a
negative id is padding; a query row with one sees no key: output row 0).  Pass ids (cheap, ``[B, S]``) or, to build the
per-64-block tables once per batch instead of once per call, a :class:`Segments` from :func:`segments`.
csrc/attn_hd.hip (bf16, head dim 64 included) and csrc/attn_f32.hip skip the blocks of other segments; csrc/attn.hip has
no segments.  They compose with causal, the key-padding mask, the bias and dropout, not with ``window``.

Global keys (Longformer / LED encoder self-attention): with ``window=w`` and ``global_keys`` ``[B, Sk]`` (nonzero =
global) key ``j`` is visible to query ``i`` when it is valid and ``|j - i| <= w`` or it is global; a global key inside
the window counts once. Pass the flags or, to build the kernels' block list once per batch instead of once per call, a
:class:`GlobalKeys` from :func:`global_keys`. The same two kernel files walk the band plus the 64-key blocks that hold
a global key, O(S·(w + 64·such blocks)); they compose with the key-padding mask, the bias and dropout, need a
``window`` and do not go with ``causal`` or segments; bf16 at head dim 32 takes the composite (csrc/attn_hd.hip). (The
rows AT the global positions attend to everything through projections of their own: the model runs them as a second,
ordinary call — models/bart.py.)

Block lists (block-sparse attention, BigBird-Pegasus encoder self-attention): ``block_lists`` is a :class:`BlockLists`
from :func:`block_lists`: per head (or one for all heads) and per query block the key blocks that block attends to.
Key ``j`` counts for query ``i`` once per occurrence of block ``j // block`` in the list of block ``i // block``: a
block listed ``n`` times counts ``n`` times, which as a dense mask is ``+ log n`` on the scores and ``-inf`` on what no
list names (``_reference``).  Repeats are the contract, not an accident: BigBird's own plans have them (models/
bigbird.py).  The same two kernel files follow the lists at 64-block granularity — a pattern whose block size is a
multiple of 64 is expanded, any other block size takes the composite on the GPU — and never load an unlisted block.
Lists compose with the key-padding mask, the bias and dropout, not with ``causal``, ``window``, segments or global
keys; bf16 at head dim 32 takes the composite.

Soft cap (Gemma 2 / T5Gemma ``attn_logit_softcapping``): with ``softcap=c`` (``c > 0``) the score of (query, key) is
``c * tanh(scale * q.k / c)``, formed before every mask.  csrc/attn_hd.hip (bf16, head dim 64 included: csrc/attn.hip
has no cap) and csrc/attn_f32.hip carry it in instantiations of their own; it composes with the key-padding mask,
``causal``, ``window`` and dropout.  With a bias LUT, segments, global keys or block lists, and bf16 at head dim 32,
a capped call takes the composite.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import _ext
from ..utils.logging import get_logger
from . import routing
from . import streams
from .gemm import colsum_record
from .rng import attention_keep_mask

# --------------------------------------------------------------------------- T5 relative bias


def relative_position_bucket(relative_position: torch.Tensor, bidirectional: bool = True, num_buckets: int = 32,
                             max_distance: int = 128) -> torch.Tensor:
    """Bit-exact re-statement of T5Attention._relative_position_bucket (modeling_t5.py:217-262)."""
    relative_buckets = 0
    if bidirectional:
        num_buckets //= 2
        relative_buckets += (relative_position > 0).to(torch.long) * num_buckets
        relative_position = torch.abs(relative_position)
    else:
        relative_position = -torch.min(relative_position, torch.zeros_like(relative_position))
    max_exact = num_buckets // 2
    is_small = relative_position < max_exact
    rp_large = max_exact + (torch.log(relative_position.float() / max_exact) / math.log(max_distance / max_exact)
                            * (num_buckets - max_exact)).to(torch.long)
    rp_large = torch.min(rp_large, torch.full_like(rp_large, num_buckets - 1))
    relative_buckets += torch.where(is_small, relative_position, rp_large)
    return relative_buckets


_bucket_cache: dict = {}


def relative_bias_lut(table: torch.Tensor, q_len: int, k_len: int, bidirectional: bool, num_buckets: int,
                      max_distance: int, q_offset: int = 0) -> torch.Tensor:
    """Per-head bias indexed by relative distance: ``lut[h, (j - i) + (q_len - 1)]`` for local query
    row ``i`` (absolute position ``i + q_offset``) and key ``j``.  Differentiable w.r.t. ``table``
    (shape ``[num_buckets, H]``).  Returns fp32 ``[H, q_len + k_len - 1]``."""
    key = (q_len, k_len, bidirectional, num_buckets, max_distance, q_offset, table.device)
    hit = _bucket_cache.get(key)
    if hit is None:
        rel = torch.arange(-(q_len - 1), k_len, dtype=torch.long) - q_offset
        idx = relative_position_bucket(rel, bidirectional, num_buckets, max_distance)
        hit = (idx.to(table.device), saturated_ranges(idx))
        if len(_bucket_cache) > 256:
            _bucket_cache.clear()
        _bucket_cache[key] = hit
    idx, sat = hit
    lut = table.float().index_select(0, idx).t().contiguous()
    # the kernels may treat tiles inside these constant-bucket ranges as scalar-bias tiles (csrc/attn_params.h):
    # valid because this LUT's gradient only reaches the table through index_select (per bucket)
    lut._dllm_sat = sat
    return lut


def saturated_ranges(idx: torch.Tensor) -> tuple[int, int]:
    """(sat_lo, sat_hi) for a bucket index row over the LUT: entries [0, sat_lo] share idx[0]'s bucket and
    [sat_hi, L) share idx[-1]'s (T5 buckets saturate at +-max_distance)."""
    L = idx.numel()
    same_lo = (idx == idx[0]).long().cumprod(0).sum().item()
    same_hi = (idx.flip(0) == idx[-1]).long().cumprod(0).sum().item()
    if same_lo == L:  # one bucket everywhere (far-apart context-parallel shards): all of it is the low range
        return L - 1, L
    return int(same_lo) - 1, int(L - same_hi)


# --------------------------------------------------------------------------- reference


class Segments:
    """Segment ids of one side of a packed batch as the kernels take them: ``ids`` int32 ``[B, S]`` contiguous and
    ``blk`` int32 ``[B, ceil(S / 64), 2]``, the (min, max) of the non-negative ids of each 64-block — ``(INT_MAX, -1)``
    for a block without one (csrc/attn_params.h).  Built once per batch by :func:`segments`."""

    __slots__ = ("ids", "blk")

    def __init__(self, ids: torch.Tensor, blk: torch.Tensor):
        self.ids, self.blk = ids, blk


_INT_MAX = 2**31 - 1


def segments(ids) -> "Segments | None":
    """:class:`Segments` of integer ids ``[B, S]`` (None and a ``Segments`` pass through)."""
    if ids is None or isinstance(ids, Segments):
        return ids
    if ids.dim() != 2 or ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"attention: segment ids must be int32 or int64 [B, S], got {ids.dtype} {tuple(ids.shape)}")
    ids = ids.to(torch.int32).contiguous()
    B, S = ids.shape
    x = torch.nn.functional.pad(ids, (0, -S % 64), value=-1).view(B, -1, 64)
    lo = torch.where(x >= 0, x, torch.full_like(x, _INT_MAX)).amin(-1)
    hi = x.clamp_min(-1).amax(-1)
    return Segments(ids, torch.stack((lo, hi), -1).contiguous())


class GlobalKeys:
    """Global-key flags of a batch as the kernels take them: ``flags`` uint8 ``[B, Sk]`` contiguous (1 = global) and
    ``blk`` int32 ``[B, 1 + ceil(Sk / 64)]``: per batch row the number of 64-key blocks that hold a global key, then
    their indices in ascending order (the rest of the row is not read; csrc/attn_params.h).  Built once per batch by
    :func:`global_keys`, without a host sync."""

    __slots__ = ("flags", "blk")

    def __init__(self, flags: torch.Tensor, blk: torch.Tensor):
        self.flags, self.blk = flags, blk


def global_keys(flags) -> "GlobalKeys | None":
    """:class:`GlobalKeys` of flags ``[B, Sk]`` (bool or integer, nonzero = global; None and a ``GlobalKeys`` pass
    through)."""
    if flags is None or isinstance(flags, GlobalKeys):
        return flags
    if flags.dim() != 2 or flags.dtype.is_floating_point or flags.dtype.is_complex:
        raise ValueError(f"attention: global_keys must be bool or integer [B, Sk], got {flags.dtype} "
                         f"{tuple(flags.shape)}")
    on = flags != 0
    B, S = on.shape
    hit = torch.nn.functional.pad(on, (0, -S % 64)).view(B, -1, 64).any(-1)  # [B, blocks]
    order = torch.argsort((~hit).to(torch.uint8), dim=1, stable=True)  # the flagged blocks first, ascending
    blk = torch.cat((hit.sum(1, keepdim=True), order), 1).to(torch.int32).contiguous()
    return GlobalKeys(on.to(torch.uint8).contiguous(), blk)


def _check_global(gk, B, Sk, window, causal, q_seg) -> None:
    """Global keys need a window and go with neither causal nor segments; flags are [B, Sk]."""
    if gk is None:
        return
    if q_seg is not None:
        raise ValueError("attention: global_keys with segments are unsupported")
    if causal:
        raise ValueError("attention: global_keys with causal are unsupported")
    if window is None:
        raise ValueError("attention: global_keys need a window")
    if tuple(gk.flags.shape) != (B, Sk):
        raise ValueError(f"attention: global_keys must be [B, Sk] = [{B}, {Sk}], got {tuple(gk.flags.shape)}")


class BlockLists:
    """A block-sparse pattern as the kernels and the composite take it.  ``ptr`` int64 ``[heads, nq + 1]`` and ``idx``
    int64 ``[nnz]`` (numpy, host): the key blocks of query block ``x`` of head ``h`` are ``idx[ptr[h, x] : ptr[h, x +
    1]]``, in list order, repeats kept; ``heads`` is the call's head count or 1 (one pattern for all heads); ``block``
    the block size in positions; ``nq`` / ``nk`` the numbers of query / key blocks.  :meth:`tables` gives the int32
    device tables of csrc/attn_params.h at 64-block granularity (``kl_ptr``, ``kl_idx`` and their transpose ``ql_ptr``,
    ``ql_idx``), built once per device and shape and kept; :meth:`log_mult` the dense definition.  Built by
    :func:`block_lists`."""

    __slots__ = ("ptr", "idx", "heads", "block", "nq", "nk", "_tables")

    def __init__(self, ptr, idx, block: int, nk: int):
        self.ptr, self.idx, self.block, self.nk = ptr, idx, int(block), int(nk)
        self.heads, self.nq = ptr.shape[0], ptr.shape[1] - 1
        self._tables: dict = {}

    def counts(self) -> np.ndarray:
        """The multiplicity matrix ``[heads, nq, nk]``: how often key block ``j`` stands in the list of query block
        ``x``.  Entries outside ``[0, nk)`` are passed over, as the kernels do."""
        m = np.zeros((self.heads, self.nq, self.nk), dtype=np.int64)
        for h in range(self.heads):
            rows = np.repeat(np.arange(self.nq), np.diff(self.ptr[h]))
            cols = self.idx[self.ptr[h, 0]:self.ptr[h, -1]]
            ok = (cols >= 0) & (cols < self.nk)
            np.add.at(m[h], (rows[ok], cols[ok]), 1)
        return m

    def log_mult(self, Sq: int, Sk: int, device) -> tuple:
        """``(bias, hidden)`` of the dense definition, both ``[heads, Sq, Sk]``: ``log`` of the multiplicity of (query,
        key) where it is listed (fp32, 0 elsewhere) and where it is not (bool)."""
        m = torch.from_numpy(self.counts()).to(device)
        m = m.repeat_interleave(self.block, 1)[:, :Sq].repeat_interleave(self.block, 2)[:, :, :Sk]
        return torch.log(m.clamp_min(1).to(torch.float32)), m == 0

    def tables(self, device, Sq: int, Sk: int) -> dict:
        """The keyword arguments of attn_hd_* / attn_f32_* (csrc/bind_attn.cpp) for a ``[Sq, Sk]`` call on ``device``:
        the lists in 64-blocks (each block of a pattern with ``block`` = 64 m stands for m x m of them, in order;
        64-blocks past the ends of the sequences are dropped) and their transpose, multiplicities kept.  Built and
        uploaded on first use, so a step that is captured and replayed builds nothing."""
        if self.block % 64:
            raise ValueError(f"attention: the kernels follow lists of 64-blocks; block size {self.block} is no multiple")
        nq, nk = (Sq + 63) // 64, (Sk + 63) // 64
        key = (str(device), nq, nk)
        hit = self._tables.get(key)
        if hit is not None:
            return hit
        m = self.block // 64
        kp, ki, qp, qi = [], [], [], []
        off = 0
        for h in range(self.heads):
            cnt = np.diff(self.ptr[h])
            rows = np.repeat(np.arange(self.nq), cnt)  # the query block of every entry, list order kept
            cols = self.idx[self.ptr[h, 0]:self.ptr[h, -1]]
            ok = (cols >= 0) & (cols < self.nk)
            rows, cols = rows[ok], cols[ok]
            if m > 1:  # (x, j) -> (m x + a, m j + c): per 64-row block a, the entries in list order, each m wide
                a, c = np.arange(m), np.arange(m)
                r64 = (rows[None, :, None] * m + a[:, None, None] + 0 * c[None, None, :])
                c64 = (cols[None, :, None] * m + 0 * a[:, None, None] + c[None, None, :])
                rows, cols = r64.reshape(-1), c64.reshape(-1)
                order = np.argsort(rows, kind="stable")
                rows, cols = rows[order], cols[order]
            ok = (rows < nq) & (cols < nk)
            rows, cols = rows[ok], cols[ok]
            kp.append(off + np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=nq)))))
            ki.append(cols)
            order = np.argsort(cols, kind="stable")  # the transpose: per key block its query blocks, ascending
            qp.append(off + np.concatenate(([0], np.cumsum(np.bincount(cols, minlength=nk)))))
            qi.append(rows[order])
            off += len(cols)
        if off >= 2**31:
            raise ValueError("attention: block lists too long")

        def dev(parts, shape):
            return torch.from_numpy(np.concatenate(parts).astype(np.int32)).view(*shape).to(device)

        hit = {"kl_ptr": dev(kp, (self.heads, nq + 1)), "kl_idx": dev(ki, (-1,)),
               "ql_ptr": dev(qp, (self.heads, nk + 1)), "ql_idx": dev(qi, (-1,))}
        self._tables[key] = hit
        return hit


def block_lists(kl, *, block: int = 64, num_key_blocks: int | None = None, device=None, seq_len=None) -> "BlockLists | None":
    """:class:`BlockLists` of ``kl`` (None and a ``BlockLists`` pass through): per head a sequence with, per query
    block, the sequence of key-block indices it attends to (Python lists or numpy arrays; lists may differ in length,
    repeat an index, or be empty) — or the lists of a single head, shared by all.  ``block``: the block size in
    positions; ``num_key_blocks``: the number of key blocks (default: that of query blocks, self-attention).  With
    ``device`` and ``seq_len`` (``S`` or ``(Sq, Sk)``) the kernels' tables are built there at once."""
    if kl is None or isinstance(kl, BlockLists):
        return kl
    if block < 1:
        raise ValueError(f"attention: block_lists block size must be >= 1, got {block}")
    heads = list(kl)
    if not heads:
        raise ValueError("attention: block_lists got no lists")

    def is_list_of_ints(x):
        return len(x) == 0 or np.ndim(x[0]) == 0

    if is_list_of_ints(heads[0]) or (isinstance(kl, np.ndarray) and kl.ndim == 2):  # one head's lists
        heads = [heads]
    nq = len(heads[0])
    ptr = np.zeros((len(heads), nq + 1), dtype=np.int64)
    idx = []
    off = 0
    for h, lists in enumerate(heads):
        if len(lists) != nq:
            raise ValueError(f"attention: block_lists head {h} has {len(lists)} query blocks, head 0 has {nq}")
        ptr[h, 0] = off
        for x, lst in enumerate(lists):
            a = np.asarray(lst)
            if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
                raise ValueError(f"attention: block_lists head {h} query block {x}: expected a 1-D list of integer "
                                 f"block indices, got {a.dtype} {a.shape}")
            idx.append(a.astype(np.int64))
            off += a.size
            ptr[h, x + 1] = off
    bl = BlockLists(ptr, np.concatenate(idx) if idx else np.zeros(0, np.int64), block,
                    nq if num_key_blocks is None else num_key_blocks)
    if device is not None and seq_len is not None and block % 64 == 0:
        sq, sk = (seq_len, seq_len) if np.ndim(seq_len) == 0 else seq_len
        bl.tables(device, int(sq), int(sk))
    return bl


def _check_lists(bl, H, Sq, Sk, window, causal, q_seg, gk) -> None:
    """Block lists go with neither causal, a window, segments nor global keys, and fit the call's heads and lengths."""
    if bl is None:
        return
    if causal:
        raise ValueError("attention: block_lists with causal are unsupported")
    if window is not None:
        raise ValueError("attention: block_lists with a window are unsupported")
    if q_seg is not None:
        raise ValueError("attention: block_lists with segments are unsupported")
    if gk is not None:
        raise ValueError("attention: block_lists with global_keys are unsupported")
    if bl.heads not in (1, H):
        raise ValueError(f"attention: block_lists are for {bl.heads} heads, the call has {H} (1 or {H} expected)")
    nq, nk = -(-Sq // bl.block), -(-Sk // bl.block)
    if (bl.nq, bl.nk) != (nq, nk):
        raise ValueError(f"attention: block_lists are for {bl.nq} x {bl.nk} blocks of {bl.block}, the call has "
                         f"{nq} x {nk} (Sq = {Sq}, Sk = {Sk})")


def _check_segments(q_seg, k_seg, B, Sq, Sk, window) -> None:
    """Segments come for both sides or neither, as ids [B, Sq] / [B, Sk], and not with a window."""
    if q_seg is None and k_seg is None:
        return
    if q_seg is None or k_seg is None:
        raise ValueError("attention: q_segments and k_segments are given together or not at all")
    if window is not None:
        raise ValueError("attention: segments with a window are unsupported")
    for name, sg, S in (("q_segments", q_seg, Sq), ("k_segments", k_seg, Sk)):
        if tuple(sg.ids.shape) != (B, S):
            raise ValueError(f"attention: {name} must be [B, S] = [{B}, {S}], got {tuple(sg.ids.shape)}")


def _check_softcap(softcap) -> float | None:
    """A soft cap is a finite positive number, or None (no cap)."""
    if softcap is None:
        return None
    c = float(softcap)
    if not (c > 0.0 and math.isfinite(c)):
        raise ValueError(f"attention: softcap must be a finite number > 0 or None, got {softcap}")
    return c


def _reference(q, k, v, scale, causal, kpm, lut, p, seed, window=None, q_seg=None, k_seg=None, gk=None, bl=None,
               softcap=None):
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    gk = global_keys(gk)
    _check_global(gk, B, Sk, window, causal, q_seg)
    qf = q.float().permute(0, 2, 1, 3)
    kf = k.float().permute(0, 2, 1, 3)
    vf = v.float().permute(0, 2, 1, 3)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    softcap = _check_softcap(softcap)
    if softcap is not None:  # before the bias and every mask
        s = softcap * torch.tanh(s / softcap)
    if lut is not None:
        rel = torch.arange(Sk, device=q.device)[None, :] - torch.arange(Sq, device=q.device)[:, None] + (Sq - 1)
        s = s + lut.float()[:, rel].unsqueeze(0)
    neg = torch.finfo(torch.float32).min
    if kpm is not None:
        s = s.masked_fill(~kpm.bool()[:, None, None, :], neg)
    if causal:
        off = Sk - Sq
        cm = torch.arange(Sk, device=q.device)[None, :] > (torch.arange(Sq, device=q.device)[:, None] + off)
        s = s.masked_fill(cm, neg)
    if window is not None:
        _check_window(window, Sq, Sk, causal)
        dist = torch.arange(Sk, device=q.device)[None, :] - torch.arange(Sq, device=q.device)[:, None]
        off = (dist.abs() > window)[None, None]
        if gk is not None:  # a global key is visible off the band too
            off = off & (gk.flags.to(q.device) == 0)[:, None, None, :]
        s = s.masked_fill(off, neg)
    q_seg, k_seg = segments(q_seg), segments(k_seg)
    _check_segments(q_seg, k_seg, B, Sq, Sk, window)
    if q_seg is not None:
        qs, ks = q_seg.ids.to(q.device), k_seg.ids.to(q.device)
        hid = (ks[:, None, :] < 0) | (qs[:, :, None] != ks[:, None, :])
        s = s.masked_fill(hid[:, None], neg)
    bl = block_lists(bl)
    _check_lists(bl, H, Sq, Sk, window, causal, q_seg, gk)
    if bl is not None:  # the dense definition: + log(multiplicity) where listed, hidden where not
        lm, hid = bl.log_mult(Sq, Sk, q.device)
        s = s.masked_fill(hid[None], neg) + lm[None]
    pr = torch.softmax(s, dim=-1)
    if bl is not None:  # an empty list, or only padding listed: rows without a visible key, output 0
        see = ~hid[None] if kpm is None else ~hid[None] & kpm.bool()[:, None, None, :]
        pr = pr * see.any(-1, keepdim=True).to(pr.dtype)
    if q_seg is not None:  # the kernels' contract for a row without a visible key (here: a padding row): output 0
        pr = pr * (qs >= 0)[:, None, :, None].to(pr.dtype)
    if p > 0.0:
        keep = attention_keep_mask(seed, p, B, H, Sq, Sk, q.device)
        pr = pr * keep.to(pr.dtype) * (1.0 / (1.0 - p))
    o = torch.matmul(pr, vf)
    return o.permute(0, 2, 1, 3).to(q.dtype)


def _check_window(window, Sq, Sk, causal) -> None:
    """A window is a band around the diagonal of a square, non-causal problem (csrc/attn_params.h)."""
    if window < 0:
        raise ValueError(f"attention: window must be >= 0 or None, got {window}")
    if Sq != Sk:
        raise ValueError(f"attention: window needs Sq == Sk, got {Sq} and {Sk}")
    if causal:
        raise ValueError("attention: window with causal is unsupported")


# --------------------------------------------------------------------------- native


def _split(mode, a, b, c):
    if mode == "qkv":  # a = [B,S,3,H,D]
        return a[:, :, 0], a[:, :, 1], a[:, :, 2]
    if mode == "q_kv":  # a = q, b = [B,Sk,2,H,D]
        return a, b[:, :, 0], b[:, :, 1]
    return a, b, c


def _tuned(q, window=None, seg=None, bl=None, softcap=None) -> bool:
    """csrc/attn.hip serves the call (bf16, head dim 64, no window, no segments, no block lists, no soft cap); else
    csrc/attn_f32.hip (fp32) or csrc/attn_hd.hip (bf16)."""
    return (q.dtype != torch.float32 and q.shape[-1] == 64 and window is None and seg is None and bl is None
            and softcap is None)


def _cap_args(softcap) -> dict:
    """The soft-cap keyword argument of attn_hd_* / attn_f32_* (csrc/bind_attn.cpp), or nothing."""
    return {} if softcap is None else {"softcap": float(softcap)}


def _seg_args(q_seg, k_seg) -> tuple:
    """The trailing segment arguments of attn_hd_* / attn_f32_* (csrc/bind_attn.cpp): ids and block tables, or nothing."""
    return () if q_seg is None else (q_seg.ids, k_seg.ids, q_seg.blk, k_seg.blk)


def _glob_args(gk) -> dict:
    """The global-key keyword arguments of attn_hd_* / attn_f32_* (csrc/bind_attn.cpp): flags and block list, or nothing."""
    return {} if gk is None else {"k_glob": gk.flags, "k_gblk": gk.blk}


def _list_args(bl, q, k) -> dict:
    """The block-list keyword arguments of attn_hd_* / attn_f32_* (csrc/bind_attn.cpp): the four tables, or nothing."""
    return {} if bl is None else bl.tables(q.device, q.shape[1], k.shape[1])


class _AttnFn(torch.autograd.Function):
    """Inputs are packed the way the projections produce them (``qkv`` = one [B,S,3,H,D] tensor for
    self-attention, ``q`` + ``kv`` [B,Sk,2,H,D] for cross-attention) so backward writes ONE packed
    gradient buffer through strided views instead of three zero-padded slice gradients."""

    @staticmethod
    def forward(ctx, mode, a, b, c, lut, kpm, scale, causal, p, seed, window=None, q_seg=None, k_seg=None, gk=None,
                bl=None, softcap=None):
        C = _ext.native()
        q, k, v = _split(mode, a, b, c)
        args = (q, k, v, kpm, lut, float(scale), bool(causal), float(p), int(seed))
        sat_lo = sat_hi = -1
        dmask = None
        if _tuned(q, window, q_seg, bl, softcap):
            # saturated bias tiles add a scalar instead of reading the LUT (forward -2 %)
            sat = getattr(lut, "_dllm_sat", None) if lut is not None else None
            sat_lo, sat_hi = sat if sat is not None else (-1, -1)
            o, lse, dmask = C.attn_fwd(*args, sat_lo, sat_hi)
        else:
            o, lse = (C.attn_f32_fwd if q.dtype == torch.float32 else C.attn_hd_fwd)(
                *args, -1 if window is None else int(window), *_seg_args(q_seg, k_seg), **_glob_args(gk),
                **_list_args(bl, q, k), **_cap_args(softcap))
        ctx.save_for_backward(a, b, c, o, lse, lut, kpm, dmask)
        ctx.cfg = (mode, scale, causal, p, seed, lut is not None and lut.requires_grad, sat_lo, sat_hi, window)
        ctx.seg = (q_seg, k_seg)  # plain int tensors, no graph: kept as they are
        ctx.gk = gk
        ctx.bl = bl
        ctx.softcap = softcap
        # packed inputs straight from a biased projection (ops/linear.py marks its output): the backward kernels also
        # sum dQ / dK / dV over tokens for that projection's bias gradient (colsum_record).  csrc/attn.hip only (the
        # partials hard-code H * 64) and bias-LUT-free calls only (its column-sum variants exist for those); everything
        # else takes the separate reduction, as with BIAS_COLSUM = False
        cs_ok = BIAS_COLSUM and lut is None and _tuned(q, window, q_seg, bl, softcap)
        ctx.cs = (cs_ok and mode != "sep" and _bias_out(a), cs_ok and mode == "q_kv" and _bias_out(b))
        # ops/linear.py stacked_linear: the packed kv is a slice of a multi-layer projection and its
        # gradient has a home in the stacked gradient buffer — write dK/dV there directly
        ctx.grad_into = getattr(b, "_dllm_grad_into", None) if mode == "q_kv" else None
        return o

    @staticmethod
    def backward(ctx, do):
        C = _ext.native()
        a, b, c, o, lse, lut, kpm, dmask = ctx.saved_tensors
        mode, scale, causal, p, seed, need_dlut, sat_lo, sat_hi, window = ctx.cfg
        q, k, v = _split(mode, a, b, c)
        da = db = dc = None
        if mode == "qkv":
            da = torch.empty_like(a)
            dq, dk, dv = da[:, :, 0], da[:, :, 1], da[:, :, 2]
        elif mode == "q_kv":
            da = torch.empty_like(a)
            gi = ctx.grad_into
            db = gi if gi is not None and gi.shape == b.shape else torch.empty_like(b)
            ctx.grad_into = None
            dq, dk, dv = da, db[:, :, 0], db[:, :, 1]
        else:
            dq = dk = dv = None
        part = pq = pkv = None
        csq = csk = csv = None
        if ctx.cs[0] or ctx.cs[1]:
            B, Sq, H = q.shape[0], q.shape[1], q.shape[2]
            HD, nq, nk = H * 64, B * ((Sq + 127) // 128), B * ((k.shape[1] + 127) // 128)
            f32 = dict(device=q.device, dtype=torch.float32)
            if mode == "qkv":  # one [blocks, 3 H D] buffer: the q | k | v thirds of the fused bias
                part = torch.empty(nq, 3 * HD, **f32)
                csq, csk, csv = part[:, :HD], part[:, HD:2 * HD], part[:, 2 * HD:]
            else:
                if ctx.cs[0]:
                    pq = csq = torch.empty(nq, HD, **f32)
                if ctx.cs[1]:
                    pkv = torch.empty(nk, 2 * HD, **f32)
                    csk, csv = pkv[:, :HD], pkv[:, HD:]
        args = (do.contiguous(), q, k, v, o, lse, kpm, lut, float(scale), bool(causal), float(p), int(seed),
                bool(need_dlut), dq, dk, dv)
        if _tuned(q, window, ctx.seg[0], ctx.bl, ctx.softcap):
            rq, rk, rv, dlut = C.attn_bwd(*args, dmask, sat_lo, sat_hi, csq, csk, csv)
        else:
            rq, rk, rv, dlut = (C.attn_f32_bwd if q.dtype == torch.float32 else C.attn_hd_bwd)(
                *args, -1 if window is None else int(window), *_seg_args(*ctx.seg), **_glob_args(ctx.gk),
                **_list_args(ctx.bl, q, k), **_cap_args(ctx.softcap))
        if part is not None:  # per-block partials, reduced by the consumer into the bias gradient (ops/gemm.py)
            colsum_record(da, part)
        if pq is not None:
            colsum_record(da, pq)
        if pkv is not None:
            colsum_record(db, pkv)
        if mode == "sep":
            da, db, dc = rq, rk, rv
        streams.pair_join()  # side-stream weight gradients paired with these VALU-bound kernels (ops/streams.py)
        return (None, da, db, dc, (dlut if need_dlut else None), None, None, None, None, None, None, None, None, None,
                None, None)


# False: the projections' bias gradients from a separate column reduction of dQKV (tests flip the module attribute)
BIAS_COLSUM = True


def _bias_out(t) -> bool:
    """t (or the tensor it is a full view of) is a biased projection's output (ops/linear.py ``_dllm_bias_out``)."""
    if t is None:
        return False
    if getattr(t, "_dllm_bias_out", False):
        return True
    src = t._base
    return (src is not None and getattr(src, "_dllm_bias_out", False) and src.data_ptr() == t.data_ptr()
            and src.numel() == t.numel())


def _prep_kpm(kpm):
    if kpm is not None and kpm.dtype != torch.uint8:
        kpm = kpm.to(torch.uint8)
    return kpm.contiguous() if kpm is not None else None


_warned: set = set()


def _warn_composite(reason: str, t) -> None:
    """One warning per process and reason when a GPU tensor takes the composite: it is the test oracle, not a kernel."""
    if reason in _warned:
        return
    _warned.add(reason)
    get_logger().warning(
        "attention: no HIP kernel for %s (head dim %d, %s); running the composite, which materialises fp32 "
        "[B, H, Sq, Sk] scores, masks and probabilities: O(Sq*Sk) memory and time.  The kernels take bf16 at head dims "
        "32 .. 128 that are multiples of 8 with 16-byte aligned rows, and fp32 at head dim 64, with or without a "
        "sliding window.",
        reason, t.shape[-1], str(t.dtype).replace("torch.", ""))


def _aligned(t) -> bool:
    """Row starts of a [..., D] view on 16 bytes (bf16): last dim contiguous, every other stride % 8, base aligned."""
    return t.stride(-1) == 1 and all(s % 8 == 0 for s in t.stride()[:-1]) and t.data_ptr() % 16 == 0


def _route(t, *rest, window=None, seg=False, glob=False, lists=None, softcap=None, lut=False):
    """Which kernel family serves a call whose q (or packed qkv) is ``t`` — by ops/routing.py ``attention_route``:

    * ``"attn.hip"``: bf16, head dim 64, no ``window`` (csrc/attn.hip, the tuned kernels);
    * ``"attn_hd.hip"``: bf16, any other head dim 32 .. 128 with ``D % 8 == 0`` and 16-byte aligned rows in ``t`` and
      ``rest`` (csrc/attn_hd.hip; blenderbot-400m has 40, t5-3b / t5-11b / nllb-3.3B 128, blenderbot-3B 80; ``attn_hd``
      = 0 sends them to the composite, A/B), and with a ``window`` or segments (``seg``) head dim 64 too;
    * ``"attn_f32.hip"``: fp32 at head dim 64 — the reference's own precision (ref/train-torchrun.py:115-128 sets
      neither bf16 nor fp16; Accelerate's default mixed_precision is 'no') — on the f32-input MFMA (``attn_f32`` = 0
      sends it to the composite, A/B);
    * ``None``: the composite ``_reference``, the exact-math oracle the kernels are tested against: CPU tensors,
      ``DLLM_REFERENCE_OPS=1``, head dims below 32, above 128 or not a multiple of 8, fp32 at head dims other than 64,
      other dtypes.  On a GPU tensor that is logged once per reason.

    ``softcap``: a capped bf16 call at head dim 64 runs csrc/attn_hd.hip (csrc/attn.hip has no cap); the kernels have
    no cap together with a bias LUT (``lut``), segments, global keys or block lists, nor at bf16 head dim 32: those
    take the composite."""
    if not _ext.use_native(t):
        return None
    D = t.shape[-1]
    bf16 = t.dtype == torch.bfloat16
    if not bf16 and t.dtype != torch.float32:
        _warn_composite("this dtype", t)
        return None
    if softcap is not None:
        other = ("a bias LUT" if lut else "segments" if seg else "global keys" if glob else
                 "block lists" if lists is not None else None)
        if other is not None:
            _warn_composite(f"a soft cap with {other}", t)
            return None
        if bf16 and D == 32:  # csrc/attn_hd.hip keeps its head dim 32 kernels the code they are
            _warn_composite("a soft cap at head dim 32", t)
            return None
    if glob and bf16 and D == 32:  # csrc/attn_hd.hip serves no global keys at head dim 32 (its header says why)
        _warn_composite("global keys at head dim 32", t)
        return None
    if lists is not None:
        if not routing.get("attn_lists"):  # A/B: list calls on the composite
            return None
        if lists.block % 64:  # the kernels follow lists of 64-blocks
            _warn_composite(f"block lists at block size {lists.block} (no multiple of 64)", t)
            return None
        if bf16 and D == 32:  # csrc/attn_hd.hip serves no block lists at head dim 32 (its header says why)
            _warn_composite("block lists at head dim 32", t)
            return None
    r = routing.attention_route(D, bf16, window, segments=seg, lists=lists is not None, softcap=softcap is not None)
    if r == "attn_hd.hip" and not all(_aligned(x) for x in (t,) + rest if x is not None):
        _warn_composite("unaligned rows", t)
        return None
    if r == "composite":
        served = (D == 64 and window is None and not seg and lists is None or bf16 and 32 <= D <= 128 and D % 8 == 0
                  or not bf16 and D == 64)
        if not served:  # (else: switched off by DLLM_ROUTE)
            _warn_composite("this head dim" if bf16 else "fp32 at this head dim", t)
        return None
    return r


def _native(t, *rest, window=None, seg=False, glob=False, lists=None, softcap=None, lut=False) -> bool:
    return _route(t, *rest, window=window, seg=seg, glob=glob, lists=lists, softcap=softcap, lut=lut) is not None


def _on(sg, t):
    """``sg`` with its tensors on ``t``'s device (a no-op for what :func:`segments` built there)."""
    if isinstance(sg, GlobalKeys):
        return sg if sg.flags.device == t.device else GlobalKeys(sg.flags.to(t.device), sg.blk.to(t.device))
    if sg is None or sg.ids.device == t.device:
        return sg
    return Segments(sg.ids.to(t.device), sg.blk.to(t.device))


_global_keys = global_keys  # the function, where a parameter of the same name shadows it
_block_lists = block_lists


def attention(q, k, v, *, scale: float = 1.0, causal: bool = False, key_padding_mask=None, bias_lut=None,
              dropout_p: float = 0.0, seed: int = 0, window: int | None = None, q_segments=None, k_segments=None,
              global_keys=None, block_lists=None, softcap: float | None = None):
    """Multi-head attention.  q ``[B,Sq,H,D]``, k/v ``[B,Sk,H,D]``; ``key_padding_mask`` bool
    ``[B,Sk]`` (True = attend); ``bias_lut`` from :func:`relative_bias_lut`; ``window``: keys with
    ``|j - i| > window`` are masked (needs ``Sq == Sk`` and ``causal=False``; None: full attention);
    ``q_segments`` / ``k_segments``: ids ``[B,Sq]`` / ``[B,Sk]`` or :class:`Segments` (both or neither, not with
    ``window``): a key is visible only to the queries of its own non-negative id; ``global_keys``: flags ``[B,Sk]``
    (nonzero = global) or :class:`GlobalKeys` (needs ``window``; not with ``causal`` or segments): such a key is
    visible to every query, inside its window or not; ``block_lists``: a :class:`BlockLists` (or what
    :func:`block_lists` takes; not with ``causal``, ``window``, segments or global keys): a key counts once per
    occurrence of its block in the list of the query's block; ``softcap``: ``c > 0`` caps the scaled scores to
    ``c * tanh(s / c)`` before the bias and every mask (None: no cap)."""
    softcap = _check_softcap(softcap)
    if window is not None:
        _check_window(window, q.shape[1], k.shape[1], causal)
    qs, ks = segments(q_segments), segments(k_segments)
    _check_segments(qs, ks, q.shape[0], q.shape[1], k.shape[1], window)
    gk = _global_keys(global_keys)
    _check_global(gk, q.shape[0], k.shape[1], window, causal, qs)
    bl = _block_lists(block_lists)
    _check_lists(bl, q.shape[2], q.shape[1], k.shape[1], window, causal, qs, gk)
    if _native(q, k, v, window=window, seg=qs is not None, glob=gk is not None, lists=bl, softcap=softcap,
               lut=bias_lut is not None):
        return _AttnFn.apply("sep", q, k, v, bias_lut, _prep_kpm(key_padding_mask), scale, causal, dropout_p, seed,
                             window, _on(qs, q), _on(ks, q), _on(gk, q), bl, softcap)
    return _reference(q, k, v, scale, causal, key_padding_mask, bias_lut, dropout_p, seed, window, qs, ks, gk, bl,
                      softcap)


def attention_qkv(qkv, **kw):
    """Self-attention on the fused projection output ``qkv`` = [B, S, 3, H, D]; ``segments=`` serves both sides."""
    kw = dict(kw)
    if "segments" in kw:
        kw["q_segments"] = kw["k_segments"] = segments(kw.pop("segments"))
    window = kw.get("window")
    if window is not None:
        _check_window(window, qkv.shape[1], qkv.shape[1], kw.get("causal", False))
    qs, ks = segments(kw.get("q_segments")), segments(kw.get("k_segments"))
    _check_segments(qs, ks, qkv.shape[0], qkv.shape[1], qkv.shape[1], window)
    gk = kw["global_keys"] = _global_keys(kw.get("global_keys"))
    _check_global(gk, qkv.shape[0], qkv.shape[1], window, kw.get("causal", False), qs)
    bl = kw["block_lists"] = _block_lists(kw.get("block_lists"))
    _check_lists(bl, qkv.shape[3], qkv.shape[1], qkv.shape[1], window, kw.get("causal", False), qs, gk)
    cap = kw["softcap"] = _check_softcap(kw.get("softcap"))
    if _native(qkv, window=window, seg=qs is not None, glob=gk is not None, lists=bl, softcap=cap,
               lut=kw.get("bias_lut") is not None):
        return _AttnFn.apply("qkv", qkv, None, None, kw.get("bias_lut"), _prep_kpm(kw.get("key_padding_mask")),
                             kw.get("scale", 1.0), kw.get("causal", False), kw.get("dropout_p", 0.0), kw.get("seed", 0),
                             window, _on(qs, qkv), _on(ks, qkv), _on(gk, qkv), bl, cap)
    return attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], **kw)


def attention_q_kv(q, kv, **kw):
    """Cross-attention with q = [B, Sq, H, D] and the fused key/value projection kv = [B, Sk, 2, H, D]."""
    window = kw.get("window")
    if window is not None:
        _check_window(window, q.shape[1], kv.shape[1], kw.get("causal", False))
    qs, ks = segments(kw.get("q_segments")), segments(kw.get("k_segments"))
    _check_segments(qs, ks, q.shape[0], q.shape[1], kv.shape[1], window)
    gk = _global_keys(kw.get("global_keys"))
    _check_global(gk, q.shape[0], kv.shape[1], window, kw.get("causal", False), qs)
    if gk is not None:
        kw = dict(kw, global_keys=gk)
    bl = _block_lists(kw.get("block_lists"))
    _check_lists(bl, q.shape[2], q.shape[1], kv.shape[1], window, kw.get("causal", False), qs, gk)
    if bl is not None:
        kw = dict(kw, block_lists=bl)
    cap = _check_softcap(kw.get("softcap"))
    if _native(q, kv, window=window, seg=qs is not None, glob=gk is not None, lists=bl, softcap=cap,
               lut=kw.get("bias_lut") is not None):
        return _AttnFn.apply("q_kv", q, kv, None, kw.get("bias_lut"), _prep_kpm(kw.get("key_padding_mask")),
                             kw.get("scale", 1.0), kw.get("causal", False), kw.get("dropout_p", 0.0), kw.get("seed", 0),
                             window, _on(qs, q), _on(ks, q), _on(gk, q), bl, cap)
    return attention(q, kv[:, :, 0], kv[:, :, 1], **kw)
