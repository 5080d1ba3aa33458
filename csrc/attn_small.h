// Device helpers shared by the two simple attention families, csrc/attn_f32.hip (fp32) and csrc/attn_hd.hip (bf16,
// head dims other than 64).  Both walk 64 x 64 (query, key) blocks with 4 waves of 16 rows on a 16x16 MFMA whose C/D
// map leaves a lane (c = lane & 15, g = lane >> 4) with keys 16 t + 4 g + i of one row, so the dropout decisions, the
// reductions over the 4 lane groups, the key mask and the bias window read the same in both.  The kernels themselves
// differ on purpose (MFMA shape, LDS images, LSE in natural-log units for fp32 and log2 units for bf16).
#pragma once
#include "common.h"

namespace {

using namespace dllm;

constexpr int BQ = 64, BKY = 64, NT = 256;  // query rows / keys per block, threads per workgroup

// Attention dropout (ops/rng.py attention_keep_mask, bit-exact): the row-Weyl hash of common.h with one row per
// (b, h, query), rh = mix32(seed, row).
// keep decision of key j of the row whose hash is rh
DLLM_DEVICE bool keep_key(uint32_t rh, int j, uint32_t thr) {
  const uint32_t y = rw_pair_y(rw_gbase(rh, (uint32_t)(j >> 1)));
  const uint32_t half = (j & 1) ? (y >> 16) : (y & 0xFFFFu);
  return (half ^ 0x8000u) >= thr;
}
// keep bits of keys j0 .. j0 + 3 (j0 % 4 == 0): bit i <-> key j0 + i; two hashes (one per key pair)
DLLM_DEVICE uint32_t keep4(uint32_t rh, int j0, uint32_t thr) {
  const uint32_t g0 = rw_gbase(rh, (uint32_t)(j0 >> 1));
  uint32_t bits = 0;
#pragma unroll
  for (int pp = 0; pp < 2; ++pp) {
    const uint32_t y = rw_pair_y(g0 + (uint32_t)pp * RW_G);
    bits |= (((y & 0xFFFFu) ^ 0x8000u) >= thr ? 1u : 0u) << (2 * pp);
    bits |= (((y >> 16) ^ 0x8000u) >= thr ? 1u : 0u) << (2 * pp + 1);
  }
  return bits;
}

DLLM_DEVICE float grp_max(float v) {  // over the 4 lane groups (same lane & 15)
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
DLLM_DEVICE float grp_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// key in range and not padding (the causal test is per (row, key), done by the callers)
template <class Params>
DLLM_DEVICE bool key_ok(const Params& P, int b, int key) {
  return key < P.Sk && (P.kpm == nullptr || P.kpm[(long)b * P.Sk + key] != 0);
}

// Sliding window (attn_params.h `window`, -1: none): the pair (row, key) lies outside the band
template <class Params>
DLLM_DEVICE bool off_band(const Params& P, int row, int key) {
  return P.window >= 0 && (key > row ? key - row : row - key) > P.window;
}
// Narrows [lo, hi), the positions a block walk covers in steps of 64 from lo, to the 64-blocks that intersect
// [x0 - window, x0 + 63 + window]: the partners the 64-block at x0 can see.  Blocks outside are never loaded.
template <class Params>
DLLM_DEVICE void band_range(const Params& P, int x0, int& lo, int& hi) {
  if (P.window >= 0) {
    const int w = min(P.window, max(P.Sq, P.Sk));  // no overflow for any window
    lo = max(lo, max(0, x0 - w) / 64 * 64);
    hi = min(hi, x0 + 64 + w);
  }
}

// Global keys (attn_params.h k_glob / k_gblk, nullptr: none).  The block walk of forward and dQ: the 64-blocks of the
// band [lo, hi) (lo % 64 == 0) merged with the batch row's ascending list gl[0 .. n) of blocks that hold a global key,
// each once and in ascending order.  next() returns the first such block start after `prev` (-64 to begin), DONE after
// the last.  Without a list it is the plain walk of [lo, hi).  Everything here is uniform over the workgroup, so the
// barriers of the walked blocks stay matched.  Entries outside [0, ceil(S / 64)) are passed over.
struct BlockWalk {
  static constexpr int DONE = 0x7FFFFFFF;
  int gi, ge, lo, hi;  // the list as indices gi .. ge - 1 into k_gblk (no pointer kept: fewer scalar registers)
  template <class Params>
  DLLM_DEVICE BlockWalk(const Params& P, int b, int lo_, int hi_) : gi(0), ge(0), lo(lo_), hi(hi_) {
    if (P.k_glob != nullptr) {
      const int nblk = (P.Sk + 63) / 64;
      gi = b * (nblk + 1) + 1;
      ge = gi + min(P.k_gblk[gi - 1], nblk);
    }
  }
  template <class Params>
  DLLM_DEVICE int next(const Params& P, int prev) {
    const int cand = prev + 64;
    int nb = max(cand, lo);
    if (nb >= hi) nb = DONE;
    while (gi < ge) {
      const int e = P.k_gblk[gi];
      if ((unsigned)e < ((unsigned)P.Sk + 63u) / 64u && e * 64 >= cand) {
        nb = min(nb, e * 64);
        break;
      }
      ++gi;
    }
    return nb;
  }
};
// Block lists (attn_params.h kl_ptr / kl_idx and ql_ptr / ql_idx, nullptr: none): the third walk, "follow a list",
// of the kernels' LISTS instantiations.  list_range gives the entries [i, e) of the list of 64-block `x` of head `h` in
// a CSR table whose rows are `n` blocks long, clamped to the index array; list_block the start of the block that entry
// `i` names, or -1 for an entry outside [0, nblk) (passed over, as BlockWalk does).  A block listed twice is walked
// twice: that is the contract.  Uniform over the workgroup, so the barriers of the walked blocks stay matched.
template <class Params>
DLLM_DEVICE void list_range(const Params& P, const int* ptr, int h, int n, int x, int& i, int& e) {
  const int* lp = ptr + (long)(P.Hl > 1 ? h : 0) * (n + 1) + x;
  i = max(lp[0], 0);
  e = min(lp[1], P.l_nnz);
}
DLLM_DEVICE int list_block(const int* idx, int i, int nblk) {
  const int e = idx[i];
  return (unsigned)e < (unsigned)nblk ? e * 64 : -1;
}
// The staged key bytes of forward / dQ carry the global flag in bit 1 (bit 0: key valid).
template <class Params>
DLLM_DEVICE uint8_t key_byte(const Params& P, int b, int key) {
  uint8_t m = key_ok(P, b, key) ? 1 : 0;
  if (P.k_glob != nullptr && key < P.Sk && P.k_glob[(long)b * P.Sk + key] != 0) m |= 2;
  return m;
}
// glob_bits: bit 16 + 4 t + i <-> the key at 16 t + 4 g + i is global; OR-ed into the visibility word of key_bits
template <class Params>
DLLM_DEVICE uint32_t glob_bits(const Params& P, const uint8_t* mk, int g) {
  uint32_t m = 0u;
  if (P.k_glob != nullptr) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(mk + 16 * t + 4 * g) >> 1;
      m |= ((w & 1u) | ((w >> 7) & 2u) | ((w >> 14) & 4u) | ((w >> 21) & 8u)) << (16 + 4 * t);
    }
  }
  return m;
}
// element predicate of forward / dQ: the pair at (t, i) lies outside the band and its key is not global
template <class Params>
DLLM_DEVICE bool off_band(const Params& P, int row, int key, uint32_t bits, int t, int i) {
  return off_band(P, row, key) && ((bits >> (16 + 4 * t + i)) & 1u) == 0u;
}
// dK / dV: the window of the lane's key — none (INT_MAX) for a valid global key, else P.window — and whether the
// workgroup's key block at k0 holds a valid global key (the block then walks every query block).  Every wave reads the
// block's 64 flags, one per lane, and votes: the same answer in all four waves without a barrier or LDS, so uniform
// over the workgroup.  (Plain loads and a ballot only: nothing here that would keep the compiler from reading the
// segment tables through the scalar cache.)
template <class Params>
DLLM_DEVICE int key_window(const Params& P, int b, int k0, int key, bool kok, bool& any) {
  any = false;
  if (P.k_glob == nullptr) return P.window;
  const int kl = k0 + (int)(threadIdx.x & 63u);
  const bool g = key_ok(P, b, kl) && P.k_glob[(long)b * P.Sk + kl] != 0;  // key_ok: kl < Sk
  any = __ballot(g) != 0ull;
  const bool kg = kok && P.k_glob[(long)b * P.Sk + key] != 0;  // kok: key < Sk
  return kg ? 0x7FFFFFFF : P.window;
}
// off_band against a lane's own window wl >= 0 (the caller tests P.window >= 0 first: uniform, so calls without a
// window skip the per-element work as before)
DLLM_DEVICE bool off_band_w(int wl, int row, int key) { return (key > row ? key - row : row - key) > wl; }

// Segments (attn_params.h q_seg / k_seg, nullptr: none).  Id of position x of a [B, S] id tensor; padding (-1) past S
DLLM_DEVICE int seg_at(const int* seg, int b, int S, int x) { return x < S ? seg[(long)b * S + x] : -1; }
// Visibility of the lane's 16 pairs of a block as one word: bit 4 t + i <-> the partner at 16 t + 4 g + i.  One
// register through the block, and 4 (+ 4) 16-B / 4-B LDS reads instead of one per pair.
// seg_bits: against the segment `own` of the lane's row (forward, dQ: `ids` = the block's key ids) or key (dK / dV:
// `ids` = the block's row ids), staged in LDS (16-B aligned): set <-> both ids are equal and not padding.  All ones
// without segments.
template <class Params>
DLLM_DEVICE uint32_t seg_bits(const Params& P, const int* ids, int own, int g) {
  uint32_t m = 0xFFFFu;
  if (P.q_seg != nullptr) {
    m = 0u;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const i32x4 v = *reinterpret_cast<const i32x4*>(ids + 16 * t + 4 * g);
#pragma unroll
      for (int i = 0; i < 4; ++i) m |= (v[i] >= 0 && v[i] == own ? 1u : 0u) << (4 * t + i);
    }
  }
  return m;
}
// key_bits: seg_bits and the staged key validity bytes `mk` (0 / 1 per key of the block, 4-B aligned) of forward / dQ
template <class Params>
DLLM_DEVICE uint32_t key_bits(const Params& P, const uint8_t* mk, const int* ids, int own, int g) {
  uint32_t m = 0u;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(mk + 16 * t + 4 * g);
    m |= ((w & 1u) | ((w >> 7) & 2u) | ((w >> 14) & 4u) | ((w >> 21) & 8u)) << (4 * t);
  }
  return m & seg_bits(P, ids, own, g);
}
// element predicate: the pair at (t, i) is hidden
DLLM_DEVICE bool hidden(uint32_t bits, int t, int i) { return ((bits >> (4 * t + i)) & 1u) == 0u; }
// no query of the 64-block at q0 shares a segment with a key of the 64-block at k0 (by the blocks' (min, max) ids):
// the block walks skip such a pair without loading it.  Uniform over the workgroup.
template <class Params>
DLLM_DEVICE bool seg_apart(const Params& P, int b, int q0, int k0) {
  if (P.q_seg == nullptr) return false;
  const int* qb = P.q_blk + 2 * ((long)b * ((P.Sq + 63) / 64) + q0 / 64);
  const int* kb = P.k_blk + 2 * ((long)b * ((P.Sk + 63) / 64) + k0 / 64);
  return qb[0] > kb[1] || kb[0] > qb[1];
}

// bias window of the (q0, k0) block, times `pre` (log2(e) where scores are in log2 units, 1.f where not): bias of
// (key, row) at Ls[key - row - (k0 - q0 - 63)]
template <class Params>
DLLM_DEVICE void stage_bias(const Params& P, int h, int q0, int k0, float* Ls, int tid, float pre) {
  if (P.lut && tid < 2 * BKY - 1) {
    const long L = (long)P.Sq + P.Sk - 1;
    long idx = (long)k0 - q0 - 63 + tid + P.Sq - 1;
    idx = idx < 0 ? 0 : (idx >= L ? L - 1 : idx);
    Ls[tid] = P.lut[(long)h * L + idx] * pre;
  }
}

// bias gradient of the (q0, k0) block from its dS tile Ds (row stride BKY + 1: a diagonal walk is bank-conflict free):
// per diagonal d = key - row + 63, one thread walks its diagonal (LDS reads, no atomics) and adds the sum to dlut once.
// The caller has made the tile visible (barrier).
template <class Params>
DLLM_DEVICE void dlut_add_diagonals(const Params& P, int h, int q0, int k0, const float* Ds, int tid) {
  if (tid < 2 * BKY - 1) {
    const long L = (long)P.Sq + P.Sk - 1;
    const int d = tid;
    const int r0 = d < 63 ? 63 - d : 0, r1 = d < 63 ? 63 : 126 - d;
    float v = 0.f;
    for (int r = r0; r <= r1; ++r) v += Ds[r * (BKY + 1) + r + d - 63];
    const long idx = (long)k0 - q0 - 63 + d + P.Sq - 1;
    if (v != 0.f && idx >= 0 && idx < L) atomicAdd(&P.dlut[(long)h * L + idx], v);
  }
}

}  // namespace
