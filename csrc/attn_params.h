// The attention contract: one parameter block for the three kernel families, filled by the host binding
// (csrc/bind_attn.cpp fill_common / fill_bwd) and passed by value to every kernel.
//
//   AttnParamsT<float>     AttnF32Params   csrc/attn_f32.hip   fp32, head dim 64
//   AttnParamsT<uint16_t>  AttnHdParams    csrc/attn_hd.hip    bf16, head dims 32 .. 128 other than 64
//   AttnParams (+ extras)                  csrc/attn.hip       bf16, head dim 64 (the tuned kernels)
//
// Tensors: q, o, dout, dq are [B, Sq, H, D] views and k, v, dk, dv [B, Sk, H, D] views of element type T with the head
// dim contiguous.  x_sb / x_ss / x_sh are the batch / sequence / head strides IN ELEMENTS, each a multiple of
// 16 bytes, and every base pointer is 16-byte aligned (16-B vector loads of row starts).
// Masks: key j is visible to query i iff kpm[b][j] != 0 (when given) and, if causal, j <= i + causal_off
// (bottom-right aligned).  Causal with Sq > Sk is served, not rejected: causal_off < 0, so the first Sq - Sk query rows
// see no key and are rows without a visible key (below); tests/test_attn_rows_gpu.py test_masks holds the kernels to it.
// Window: with window >= 0 key j is visible to query i iff, besides the above, |j - i| <= window (a band around the
// diagonal); -1: no window.  Windowed calls have Sq == Sk and causal == 0 (the binding checks both).  The block walks of
// csrc/attn_hd.hip and csrc/attn_f32.hip skip the 64 x 64 blocks outside the band, so work and traffic are
// O(S * window); csrc/attn.hip has no window and is never given one.  With a window a row can lack a visible key only
// through the padding mask.
// Segments (sequence packing): with q_seg / k_seg given (both or neither) key j is visible to query i iff, besides the
// above, k_seg[b][j] >= 0 && q_seg[b][i] == k_seg[b][j]; a negative id is padding, so a query row with a negative id is
// a row without a visible key.  q_blk / k_blk hold, per 64-block, the min and max of its non-negative ids ((INT_MAX, -1)
// for a block without one): forward and dQ skip the key blocks, dK / dV the query blocks, whose [min, max] does not
// overlap their own — never loaded, so work and traffic follow the sum of the squared segment lengths.  The block test
// is correct for any ids and exact for non-decreasing ones (what data/packing.py emits).  Segments compose with kpm,
// causal, the bias and dropout (the keep hash still indexes (b, h, row, key)), not with a window (the binding
// rejects it); csrc/attn.hip has no segments and is never given any.
// Global keys (Longformer / LED): k_glob is given only with window >= 0, together with k_gblk. With it key j is visible
// to query i iff key_ok && (!off_band || k_glob[b][j]): a global key is seen by every query, inside its window or not
// (and counts once where it lies inside). k_gblk lists, per batch row, the 64-key blocks that hold a global key: [b][0]
// = their number n, [b][1 .. n] their indices, ascending (the rest of the row is not read). Forward and dQ walk the
// band blocks and the listed blocks outside it, each block once and in ascending key order, so a call whose k_glob is
// all zero is the window-only call, bit for bit; dK / dV walk every query block from a key block that holds a valid
// global key (every wave reads the block's 64 flags and votes, so uniform) and the band from any other. Blocks neither
// in the band nor listed are never loaded: work and traffic are O(S * (window + 64 * listed blocks)). Global keys
// compose with kpm, the bias LUT (indexed by j - i as always) and dropout (the keep hash still indexes (b, h, row,
// key)), not with causal or segments (the binding rejects both); csrc/attn.hip has none, and csrc/attn_hd.hip none at
// head dim 32 (the binding rejects it).
// Block lists (block-sparse attention, BigBird): with kl_ptr / kl_idx / ql_ptr / ql_idx given (all four or none) the
// walks follow explicit lists of 64-blocks instead of a range. nq = ceil(Sq / 64), nk = ceil(Sk / 64); kl_ptr is
// [Hl, nq + 1] and ql_ptr [Hl, nk + 1] (CSR row starts into kl_idx / ql_idx, both [nnz]), Hl = H or 1 (one list shared
// by all heads), the same for every batch row. For head h and query block x, forward and dQ visit the key blocks
// kl_idx[kl_ptr[h][x] .. kl_ptr[h][x + 1]) in list order; dK / dV visit, for a key block, the query blocks of ql_idx
// alike — the transpose of the key lists, with the same multiplicities (the host builds both, ops/attention.py
// block_lists). Key j contributes to query i once per occurrence of block j / 64 in the list of block i / 64, if
// key_ok: a block listed n times is visited n times, and the online softmax, dS and the bias gradient count its keys n
// times (as a dense mask: + log n on the scores). BigBird's own plans repeat blocks, so this is the contract and not
// an accident. An empty list gives rows without a visible key (output 0, LSE +inf); a key block in no list gets
// dK = dV = 0; entries outside [0, nk) / [0, nq) are passed over, as BlockWalk does, and row starts are clamped to
// [0, nnz]; blocks not listed are never loaded. A list of every block once, ascending, is the list-free call bit for
// bit. Everything in the walk is uniform over the workgroup. Lists compose with kpm, the bias LUT (indexed by j - i)
// and its gradient, and dropout (the keep hash indexes (b, h, row, key), so the copies of a repeated key are kept or
// dropped together), not with causal, a window, segments or global keys (the binding rejects each); csrc/attn.hip has
// none, and csrc/attn_hd.hip none at head dim 32 (the binding rejects it).
// Soft cap (Gemma 2 / T5Gemma attn_logit_softcapping): with softcap = c > 0 the score of (i, j) is c * tanh(scale *
// q_i.k_j / c), formed before every mask (and, in the bf16 family, before the log2(e) factor); backward recomputes t =
// tanh(.) and scales dS by 1 - t^2: dS_raw = P o (dP_kept - delta) o (1 - t^2).  It lives in kernel instantiations of
// its own (template parameter CAP), so a call without a cap runs the code it ran before.  The cap composes with kpm,
// causal (Sq != Sk included), a window and dropout, not with the bias LUT, segments, global keys or block lists (the
// binding rejects each); csrc/attn.hip has none, and csrc/attn_hd.hip none at head dim 32 (the binding rejects it).
// The bf16 family forms tanh as 1 - 2 / (1 + exp2(2 log2(e) z)), which saturates to +-1 at +-inf; the fp32 family
// uses the device library's tanhf, relatively accurate near 0 where that form cancels.
// Bias: lut[h][(j - i) + Sq - 1] is added to the scaled score.
// LSE: [B, H, Sq] fp32, forward writes and backward reads; +inf marks a row without a visible key (its output row is
// 0).  The bf16 families store it in log2 units (scores are scaled by log2(e), softmax by exp2), fp32 in natural-log
// units.
// Dropout: probabilities are dropped by the counter-based hash of ops/rng.py attention_keep_mask with `seed`; a key is
// kept iff its 16-bit hash half (sign bit flipped) >= thr, thr = min(65535, p_drop * 65536) (ops/rng.py threshold16).
#pragma once
#include <stdint.h>

template <class T>
struct AttnParamsT {
  typedef T elem;
  const T* q;
  const T* k;
  const T* v;
  const T* o;          // bwd: forward output
  const T* dout;       // bwd: output gradient
  T* o_out;            // fwd output
  float* lse;          // [B, H, Sq]
  float* delta;        // [B, H, Sq]: rowsum(dO * O), written by the backward's first kernel
  T* dq;
  T* dk;
  T* dv;
  float* dlut;         // [H, Sq + Sk - 1] fp32 (bwd, accumulated with atomics; zeroed by the host); nullptr: not wanted
                       // (csrc/attn.hip: always given with lut)
  const uint8_t* kpm;  // [B, Sk] 1 = attend; nullptr: none
  const float* lut;    // [H, Sq + Sk - 1]; nullptr: none
  const int* q_seg;    // [B, Sq] segment ids, < 0: padding; nullptr: no segments (csrc/attn_hd.hip, csrc/attn_f32.hip only)
  const int* k_seg;    // [B, Sk]; given with q_seg
  const int* q_blk;    // [B, ceil(Sq / 64), 2] (min, max) of the ids >= 0 of each 64-block of q_seg; given with q_seg
  const int* k_blk;    // [B, ceil(Sk / 64), 2]
  const uint8_t* k_glob;  // [B, Sk] 1 = global key; nullptr: none; only with window >= 0 (csrc/attn_hd.hip,
                          // csrc/attn_f32.hip only)
  const int* k_gblk;   // [B, 1 + ceil(Sk / 64)]: the number of 64-key blocks with a global key, then their indices
                       // (ascending); given with k_glob
  long q_sb, q_ss, q_sh;
  long k_sb, k_ss, k_sh;
  long v_sb, v_ss, v_sh;
  long o_sb, o_ss, o_sh;  // o and o_out
  long do_sb, do_ss, do_sh;
  long dq_sb, dq_ss, dq_sh;
  long dk_sb, dk_ss, dk_sh;
  long dv_sb, dv_ss, dv_sh;
  int B, H, Sq, Sk;
  int D;           // head dim: 64, or for csrc/attn_hd.hip 32 .. 128 (% 8 == 0; its kernels are instantiated for D
                   // rounded up to 32)
  float scale;
  int causal;
  int causal_off;  // Sk - Sq
  int window;      // -1: none; w >= 0: keys with |j - i| > w are masked (csrc/attn_hd.hip, csrc/attn_f32.hip only)
  float p_drop;
  uint32_t seed;
  uint32_t thr;    // set by the host (csrc/attn.hip: by its launchers)
  // block lists, after everything else: the fields above keep the offsets (and the kernels the argument loads) they had
  const int* kl_ptr;   // [Hl, ceil(Sq / 64) + 1] row starts into kl_idx; nullptr: no block lists (csrc/attn_hd.hip,
                       // csrc/attn_f32.hip only)
  const int* kl_idx;   // [nnz] 64-key block indices, forward and dQ; given with kl_ptr
  const int* ql_ptr;   // [Hl, ceil(Sk / 64) + 1] row starts into ql_idx; given with kl_ptr
  const int* ql_idx;   // [nnz] 64-query block indices, dK / dV: the transpose of kl, multiplicities kept
  int Hl;          // heads of the block lists: H, or 1 (shared by all heads); 0 without lists
  int l_nnz;       // length of kl_idx and of ql_idx
  // soft cap, after the block lists for the same reason
  float softcap;   // 0: none; c > 0: the score is c * tanh(scale * q.k / c) (csrc/attn_hd.hip, csrc/attn_f32.hip only)
};

using AttnF32Params = AttnParamsT<float>;
using AttnHdParams = AttnParamsT<uint16_t>;

struct AttnParams : AttnParamsT<uint16_t> {
  float* rowrec;    // [B*H][sq_pad / 64][4][64] per-row terms for dK/dV (written by the dQ kernel):
                    // -lse2, c_lo - lse2, c_hi - lse2, -delta (rows >= Sq: -inf, -inf, -inf, 0).  Left unwritten by
                    // the one-pass cross-attention backward, whose single kernel forms the terms in LDS
  uint32_t* dmask;  // [B*H][n_ktiles][2][sq_pad] dropout keep bits written by fwd, read by bwd
  // Saturated bias ranges (T5 relative buckets): LUT entries [0, sat_lo] all equal lut[0] and [sat_hi, L) all
  // equal lut[L-1], and the LUT gradient is only consumed per bucket.  A (forward, dQ, dK/dV) tile whose LUT
  // indices all fall in one range adds a scalar bias (no LDS lookups) and its dS sum is credited to lut[0] /
  // lut[L-1] (no diagonal shear).  Disabled: sat_lo = INT_MIN / 2, sat_hi = INT_MAX / 2.
  int sat_lo;
  int sat_hi;
  // bwd, optional: per-block column sums of dQ / dK / dV (the bias gradients of the projections that produced q / k /
  // v).  Row b * ceil(S / 128) + block (S = Sq for csq, Sk for csk / csv), columns h * 64 + d, row strides csq_ld /
  // cskv_ld floats; the host sums the rows (ops/attention.py).  nullptr: not wanted.
  float* csq;
  float* csk;
  float* csv;
  long csq_ld, cskv_ld;
  // filled by the launchers
  int n_tiles;   // fwd: q tiles; bwd: key blocks
  int n_ktiles;  // 64-key tiles (key-mask array length / 64)
  int sq_pad;    // rows of the dropout bit-mask planes (query tiles x 128)
};
