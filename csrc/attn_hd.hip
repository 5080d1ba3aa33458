// bf16 flash attention (forward + backward) for head dims 32 .. 128 other than 64 (head dim 64 runs csrc/attn.hip):
// the bf16 sibling of csrc/attn_f32.hip, templated on the padded head dim DP in {32, 64, 96, 128}.  bf16 in, bf16 out,
// fp32 accumulation on v_mfma_f32_16x16x32_bf16.  Same op and semantics as csrc/attn.hip / csrc/attn_f32.hip: softmax
// scale, T5 relative-position bias LUT [H, Sq + Sk - 1] (+ its fp32 gradient), key-padding mask, causal mask with
// causal_off = Sk - Sq, and attention-probability dropout with the exact keep decisions of ops/rng.py
// attention_keep_mask.  O(S) memory.  LSE convention of csrc/attn.hip: log2 units, +inf for a row without a valid key
// (its output row is 0) — parallel/context.py _merge combines blocks by it.
//
// The real head dim D (D % 8 == 0, 32 <= D <= DP) is a runtime field: columns D .. DP-1 are staged as zeros and never
// stored.  bias / kpm / causal / window are runtime flags; only DP, DROP, LISTS and CAP are template parameters (24
// kernel instantiations, 18 that follow block lists and 18 that cap the scores).
//
// Sliding window (AttnParamsT::window >= 0, LongT5-local; Sq == Sk, not causal): forward and dQ walk only the key
// blocks that intersect [q0 - w, q0 + 63 + w], dK / dV only the query blocks that intersect [k0 - w, k0 + 63 + w]
// (attn_small.h band_range) — the others are never loaded — and the element mask gains |key - row| > w (off_band).
// Windowed calls at head dim 64 run here too (DP = 64): csrc/attn.hip has no window.
//
// Segments (AttnParamsT::q_seg / k_seg, sequence packing): the element mask gains "same non-negative id" (attn_small.h
// seg_bits / key_bits: one 16-bit visibility word per lane and block from the ids and key validity staged in LDS) and
// the walks skip — never load — the blocks whose (min, max) id range does not overlap the workgroup's own (seg_apart,
// uniform per workgroup, so the barriers stay matched).  A runtime flag like the window; packed calls at head dim 64
// run here too.
//
// Global keys (AttnParamsT::k_glob / k_gblk, Longformer / LED; only with a window): a global key is visible to every
// query, in its band or not.  Forward and dQ walk the band blocks merged with the batch row's list of blocks that hold
// a global key (attn_small.h BlockWalk: each block once, ascending, so an all-zero k_glob is the window-only call bit
// for bit); dK / dV walk every query block from a key block with a valid global key (key_window: a vote over the
// block's flags) and the band from the others.  Blocks neither in the band nor listed are never loaded.  A runtime
// flag like the window.
//
// Block lists (AttnParamsT::kl_ptr / kl_idx / ql_ptr / ql_idx, block-sparse attention such as BigBird's): forward and
// dQ follow the query block's list of 64-key blocks, dK / dV the key block's list of 64-query blocks (attn_small.h
// list_range / list_block) — a third loop over the same block body.  A block listed n times is walked n times and so
// counts n times (attn_params.h says why that is the contract); unlisted blocks are never loaded.  The third loop
// lives in instantiations of its own (template parameter LISTS, head dims other than 32): in the kernels that serve
// every other call it cost scalar spills (dQ) or occupancy, so those are the code they were
// (profiles/attn_block_lists.txt).  No causal, window, segments or global keys with lists, and none at head dim 32
// (the launchers refuse, the op takes the composite).
//
// Soft cap (AttnParamsT::softcap > 0, Gemma 2 / T5Gemma): the score is c tanh(scale s / c), formed before the log2(e)
// factor and every mask; dQ and dK / dV recompute the tanh and scale dS by 1 - tanh^2.  Like the lists it lives in
// instantiations of its own (template parameter CAP, head dims other than 32, never with LISTS): the per-score VALU
// work (an exp2, a reciprocal and three multiply-adds) and its registers stay out of the kernels of every other call,
// which are the code they were (profiles/attn_softcap.txt).  Capped calls at head dim 64 run here too: csrc/attn.hip
// has no cap.  No bias LUT, segments, global keys or lists with a cap, and none at head dim 32 (the launchers refuse,
// the op takes the composite).
//
// Layout trick of csrc/attn_f32.hip, carried over to the 16x16x32 bf16 MFMA: its C/D map puts rows 4g .. 4g+3
// (g = lane >> 4) of column (lane & 15) in a lane's 4 registers, and its A/B maps take reduction indices k = 8g + j
// (j = 0 .. 7) from lane group g.  S^T = K Q^T leaves each lane with keys 16t + 4g + i of ONE query row; two such
// 16-key tiles (t = 2u, 2u+1) packed to bf16 are the B operand of the next product as they stand, reducing over keys
// {32u + 4g + j, 32u + 16 + 4g + j : j < 4} — the other operand is read in the same key order by two hardware-
// transposed LDS reads (ds_read_b64_tr_b16) of the row-major image.  No LDS round trip for P or dS, and one image per
// staged tensor.
//
//   forward    grid (Sq/64, B*H), 4 waves x 16 query rows; per 64-key block: K and V staged row-major in LDS,
//              S^T = K Q^T, online softmax + dropout in registers, O^T += V^T P^T.
//   delta      rowsum(dO * O), one 16-lane group per row.
//   dQ         grid (Sq/64, B*H): S^T, dP^T = V dO^T, dS = P (dP_kept - delta), dQ^T += K^T dS^T; the bias gradient is
//              summed per diagonal of the block's dS tile in LDS and added to dlut once per block (fp32 atomics).
//   dK / dV    grid (Sk/64, B*H), 4 waves x 16 keys: S = Q K^T, dP = dO V^T, dV^T += dO^T P_kept, dK^T += Q^T dS.
#include "common.h"
#include "attn_params.h"
#include "attn_small.h"

using namespace dllm;

DLLM_SEED_STEP_TU(attn_hd)

namespace {

constexpr float LOG2E = 1.4426950408889634f;

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8v;
typedef __attribute__((ext_vector_type(4))) short s16x4;

DLLM_DEVICE f32x4 mma(bf16x8v a, bf16x8v b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

DLLM_DEVICE float ex2(float x) { return __builtin_amdgcn_exp2f(x); }  // v_exp_f32: exp2(-inf) = 0

// tanh(z) from z2 = 2 log2(e) z: 1 - 2 / (1 + exp2(z2)).  Saturates exactly: exp2 = inf gives 1, exp2 = 0 gives -1.
// Its absolute error (a few 1e-8 from the cancellation near 0) is far below bf16's.
DLLM_DEVICE float tanh_ex2(float z2) { return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + ex2(z2)); }

// LDS image of a 64-row tile: [64][DP + 8] bf16, row-major.  The 16-B pad per row spreads the 16 rows of one
// ds_read_b128 fragment read over all banks (row stride = DP / 2 + 4 dwords: 4 r mod 64 distinct for r < 16).
template <int DP> struct Img {
  static constexpr int LD = DP + 8, CPR = DP / 8, SIZE = 64 * LD;
};

// stage rows [r0, r0 + 64) of a [*, S, H, D] view (row stride ss) into the image: rows >= S and columns >= D as zeros.
// 256 threads, DP / 32 16-B chunks each.
template <int DP>
DLLM_DEVICE void stage(const uint16_t* base, long ss, int r0, int S, int D, uint16_t* img, int tid) {
  constexpr int LD = Img<DP>::LD, CPR = Img<DP>::CPR;
#pragma unroll
  for (int j = 0; j < DP / 32; ++j) {
    const int idx = tid + NT * j, r = idx / CPR, ch = idx % CPR;
    u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (r0 + r < S && 8 * ch < D) v = *reinterpret_cast<const u16x8*>(base + (long)(r0 + r) * ss + 8 * ch);
    *reinterpret_cast<u16x8*>(img + r * LD + 8 * ch) = v;
  }
}

// the DP / 32 operand fragments of one row from global memory: fragment ks = columns 32 ks + 8 g .. + 7 (0 past D)
template <int DP>
DLLM_DEVICE void load_row_frags(const uint16_t* rowp, int g, int D, bf16x8v (&f)[DP / 32]) {
#pragma unroll
  for (int ks = 0; ks < DP / 32; ++ks) {
    const int d0 = 32 * ks + 8 * g;
    u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (d0 < D) v = *reinterpret_cast<const u16x8*>(rowp + d0);
    f[ks] = __builtin_bit_cast(bf16x8v, v);
  }
}

// MFMA operand whose reduction index is the head dim: row r, columns 32 ks + 8 g .. + 7 of the image
template <int DP>
DLLM_DEVICE bf16x8v ld_row(const uint16_t* img, int r, int ks, int g) {
  return __builtin_bit_cast(bf16x8v, *reinterpret_cast<const u16x8*>(img + r * Img<DP>::LD + 32 * ks + 8 * g));
}

// MFMA operand whose reduction index is the tile row (sequence): for the lane (c, g), column c0 + c of rows
// rb + 4 g + {0..3} (elements 0..3) and rb + 16 + 4 g + {0..3} (elements 4..7) — the key order of two packed
// accumulator tiles.  ds_read_b64_tr_b16: a 16-lane group reads 4 rows x 16 columns, lane 4 q + p supplies the
// address of row q, columns 4 p .. 4 p + 3, and group lane i receives column i of the 4 rows.  EXEC must be full.
template <int DP>
DLLM_DEVICE bf16x8v ld_tr2(const uint16_t* img, int rb, int c0, int c, int g) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const uint16_t* p = img + (rb + 4 * g + (c >> 2)) * Img<DP>::LD + c0 + 4 * (c & 3);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 16 * Img<DP>::LD));
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  const s16x8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  return __builtin_bit_cast(bf16x8v, v);
}

// two accumulator tiles (t = 2u, 2u + 1) as one bf16 operand: element j <- a[j], element 4 + j <- b[j]
DLLM_DEVICE bf16x8v pack8(f32x4 a, f32x4 b) {
  const u32x4 r = {pack_bf16x2(a.x, a.y), pack_bf16x2(a.z, a.w), pack_bf16x2(b.x, b.y), pack_bf16x2(b.z, b.w)};
  return __builtin_bit_cast(bf16x8v, r);
}

// 4 bf16 of an accumulator tile to columns d0 .. d0 + 3 of a row (8-B store)
DLLM_DEVICE void st4(uint16_t* p, f32x4 v) { Elem<uint16_t>::store4(p, v); }

// Waves per SIMD each instantiation is held to (the second __launch_bounds__ argument): what its register count gave
// before the segment hooks, so that the runtime flags added since cannot cost the unsegmented calls their occupancy —
// raised, where the segment hooks' build ran at more, to what it ran at before the global keys
// (profiles/attn_global_keys.txt).
// Head dim 32 serves no global keys, and its three kernels are the code they were, under the floors they had: its
// dropout forward runs at 6 waves in 80 registers, and every form of a second walk tried there either spilled into
// the loop of the calls without global keys or slowed them by 2 - 29 % (profiles/attn_global_keys.txt, section 5).
// The launchers refuse k_glob at DP = 32 and the op sends such a call to the composite; forward and dQ include their
// block body in place there, and the global-key terms are compiled out by `DP != 32` constants inside the
// short-circuit mask chain (evaluated before the chain they cost a branch sequence per element).
constexpr int occ_fwd(int DP, bool DROP) {
  return DP == 32 ? 5 : DP == 64 ? 4 : DP == 96 ? (DROP ? 3 : 4) : 3;
}
constexpr int occ_dq(int DP, bool DROP) {
  return DP == 32 ? 4 : DP == 64 ? (DROP ? 3 : 4) : DP == 96 ? 3 : (DROP ? 3 : 2);
}
constexpr int occ_dkdv(int DP) { return DP == 32 ? 3 : DP == 64 ? 3 : 2; }

// ================================================================================================ forward
template <int DP, bool DROP, bool LISTS = false, bool CAP = false>
__global__ __launch_bounds__(NT, occ_fwd(DP, DROP)) void attn_hd_fwd_kernel(AttnHdParams P) {
  constexpr int KS = DP / 32, DT = DP / 16;
  __shared__ __attribute__((aligned(16))) uint16_t Ks[Img<DP>::SIZE];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[Img<DP>::SIZE];
  __shared__ float Ls[2 * BKY];
  __shared__ __attribute__((aligned(16))) uint8_t Mk[BKY];  // 1: key valid (in range, not padding)
  __shared__ __attribute__((aligned(16))) int Sg[BKY];  // the keys' segment ids (with segments)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
  const int bh = blockIdx.y, b = bh / P.H, h = bh % P.H;
  const int q0 = blockIdx.x * BQ;
  const int row = q0 + 16 * w + c;
  const int rowc = min(row, P.Sq - 1);
  const int qsg = P.q_seg ? seg_at(P.q_seg, b, P.Sq, row) : 0;
  bf16x8v qf[KS];
  load_row_frags<DP>(P.q + (long)b * P.q_sb + (long)rowc * P.q_ss + (long)h * P.q_sh, g, P.D, qf);
  const uint32_t rh = DROP ? mix32(eff_seed(P.seed), (uint32_t)((long)bh * P.Sq + rowc)) : 0u;
  const float dscale = DROP ? 1.f / (1.f - P.p_drop) : 1.f;
  const float scale2 = P.scale * LOG2E;
  // soft cap: x = c log2(e) tanh(scale s / c), tanh from exp2(2 log2(e) z) (tanh_ex2)
  const float capz2 = CAP ? P.scale / P.softcap * (2.f * LOG2E) : 0.f;
  const float capc2 = CAP ? P.softcap * LOG2E : 0.f;
  float m = -INFINITY, l = 0.f;
  f32x4 acc[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const uint16_t* kb = P.k + (long)b * P.k_sb + (long)h * P.k_sh;
  const uint16_t* vb = P.v + (long)b * P.v_sb + (long)h * P.v_sh;
  int kend = P.Sk;
  if (P.causal) kend = min(P.Sk, max(0, q0 + BQ + P.causal_off));
  int kstart = 0;
  band_range(P, q0, kstart, kend);
  if constexpr (LISTS) {
    // follow the query block's list of key blocks, repeats included (no causal, window, segments or global keys here)
    int li, le;
    list_range(P, P.kl_ptr, h, (P.Sq + 63) / 64, (int)blockIdx.x, li, le);
    for (; li < le; ++li) {
      const int k0 = list_block(P.kl_idx, li, (P.Sk + 63) / 64);
      if (k0 < 0) continue;
#include "attn_hd_fwd_block.h"
    }
  } else if constexpr (DP == 32) {
    // Head dim 32 has no global keys (above): the loop and the block body as they were, in place.  (Through the lambda
    // below its dropout instantiation no longer fits the 80 registers of its 6 waves, with or without a second loop.)
    for (int k0 = kstart; k0 < kend; k0 += BKY) {
      if (seg_apart(P, b, q0, k0)) continue;
#include "attn_hd_fwd_block.h"
    }
  } else {
    // one 64-key block of the walk.  Expanded twice on purpose, once per loop below: calls without global keys keep
    // the affine loop they had (a single data-dependent walk for both cost the segment calls 9 - 17 %,
    // profiles/attn_global_keys.txt)
    auto block = [&](int k0) __attribute__((always_inline)) {
#include "attn_hd_fwd_block.h"
    };
    if (P.k_glob == nullptr) {  // the walk as it was before the global keys: the band (or all), segment skips
      for (int k0 = kstart; k0 < kend; k0 += BKY) {
        if (seg_apart(P, b, q0, k0)) continue;
        block(k0);
      }
    } else {  // the band merged with the listed blocks outside it (no segments with global keys)
      BlockWalk walk(P, b, kstart, kend);
      for (int k0 = walk.next(P, -BKY); k0 != BlockWalk::DONE; k0 = walk.next(P, k0)) block(k0);
    }
  }
  // acc[dt][i] = O[row][d = 16 dt + 4 g + i] (unnormalised)
  if (row < P.Sq) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    uint16_t* op = P.o_out + (long)b * P.o_sb + (long)row * P.o_ss + (long)h * P.o_sh;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
      if (16 * dt + 4 * g < P.D) st4(op + 16 * dt + 4 * g, acc[dt] * inv);
    if (g == 0) P.lse[(long)bh * P.Sq + row] = l > 0.f ? m + __log2f(l) : INFINITY;
  }
}

// ================================================================================================ backward
// delta[bh][row] = sum_d dO * O; one 16-lane group per row, lane j takes columns 8 j .. 8 j + 7 (D <= 128)
__global__ __launch_bounds__(NT) void attn_hd_delta_kernel(AttnHdParams P) {
  const long rows = (long)P.B * P.H * P.Sq;
  const long r = (long)blockIdx.x * (NT / 16) + (threadIdx.x >> 4);
  const int j = threadIdx.x & 15;
  float s = 0.f;
  if (r < rows && 8 * j < P.D) {
    const int row = (int)(r % P.Sq);
    const long bh = r / P.Sq;
    const int b = (int)(bh / P.H), h = (int)(bh % P.H);
    const u16x8 o = *reinterpret_cast<const u16x8*>(P.o + (long)b * P.o_sb + (long)row * P.o_ss + (long)h * P.o_sh + 8 * j);
    const u16x8 d = *reinterpret_cast<const u16x8*>(P.dout + (long)b * P.do_sb + (long)row * P.do_ss +
                                                    (long)h * P.do_sh + 8 * j);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += bf2f(o[e]) * bf2f(d[e]);
  }
#pragma unroll
  for (int mm = 8; mm >= 1; mm >>= 1) s += __shfl_xor(s, mm, 16);
  if (r < rows && j == 0) P.delta[r] = s;
}

template <int DP, bool DROP, bool LISTS = false, bool CAP = false>
__global__ __launch_bounds__(NT, occ_dq(DP, DROP)) void attn_hd_dq_kernel(AttnHdParams P) {
  constexpr int KS = DP / 32, DT = DP / 16;
  __shared__ __attribute__((aligned(16))) uint16_t Ks[Img<DP>::SIZE];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[Img<DP>::SIZE];
  __shared__ float Ls[2 * BKY];
  __shared__ float Ds[BQ * (BKY + 1)];  // dS tile of the block, row stride 65: a diagonal walk is bank-conflict free
  __shared__ __attribute__((aligned(16))) uint8_t Mk[BKY];
  __shared__ __attribute__((aligned(16))) int Sg[BKY];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
  const int bh = blockIdx.y, b = bh / P.H, h = bh % P.H;
  const int q0 = blockIdx.x * BQ;
  const int row = q0 + 16 * w + c;
  const int rowc = min(row, P.Sq - 1);
  const int qsg = P.q_seg ? seg_at(P.q_seg, b, P.Sq, row) : 0;
  const bool row_ok = row < P.Sq;
  bf16x8v qf[KS], dof[KS];
  load_row_frags<DP>(P.q + (long)b * P.q_sb + (long)rowc * P.q_ss + (long)h * P.q_sh, g, P.D, qf);
  load_row_frags<DP>(P.dout + (long)b * P.do_sb + (long)rowc * P.do_ss + (long)h * P.do_sh, g, P.D, dof);
  const float lse = row_ok ? P.lse[(long)bh * P.Sq + row] : INFINITY;
  const float dlt = row_ok ? P.delta[(long)bh * P.Sq + row] : 0.f;
  const uint32_t rh = DROP ? mix32(eff_seed(P.seed), (uint32_t)((long)bh * P.Sq + rowc)) : 0u;
  const float dscale = DROP ? 1.f / (1.f - P.p_drop) : 1.f;
  const float scale2 = P.scale * LOG2E;
  // soft cap: x = c log2(e) tanh(scale s / c), tanh from exp2(2 log2(e) z) (tanh_ex2)
  const float capz2 = CAP ? P.scale / P.softcap * (2.f * LOG2E) : 0.f;
  const float capc2 = CAP ? P.softcap * LOG2E : 0.f;
  const bool want_dlut = P.dlut != nullptr && P.lut != nullptr;
  // the row's dQ address, formed here: two vector registers through the walk instead of the eight scalar ones of the
  // base and strides, which the walk's own scalars would otherwise push out to spills
  uint16_t* dqp = P.dq + (long)b * P.dq_sb + (long)rowc * P.dq_ss + (long)h * P.dq_sh;
  if constexpr (DP != 32) asm volatile("" : "+v"(dqp));  // formed here, not sunk to the epilogue (DP = 32: no walk)
  f32x4 acc[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const uint16_t* kb = P.k + (long)b * P.k_sb + (long)h * P.k_sh;
  const uint16_t* vb = P.v + (long)b * P.v_sb + (long)h * P.v_sh;
  int kend = P.Sk;
  if (P.causal) kend = min(P.Sk, max(0, q0 + BQ + P.causal_off));
  int kstart = 0;
  band_range(P, q0, kstart, kend);
  if constexpr (LISTS) {
    // follow the query block's list of key blocks, repeats included, as the forward
    int li, le;
    list_range(P, P.kl_ptr, h, (P.Sq + 63) / 64, (int)blockIdx.x, li, le);
    for (; li < le; ++li) {
      const int k0 = list_block(P.kl_idx, li, (P.Sk + 63) / 64);
      if (k0 < 0) continue;
#include "attn_hd_dq_block.h"
    }
  } else if constexpr (DP == 32) {
    // Head dim 32 has no global keys: the loop and the block body of before, in place, as in the forward
    for (int k0 = kstart; k0 < kend; k0 += BKY) {
      if (seg_apart(P, b, q0, k0)) continue;
#include "attn_hd_dq_block.h"
    }
  } else {
    // one 64-key block of the walk.  Expanded twice on purpose, once per loop below: calls without global keys keep
    // the affine loop they had (a single data-dependent walk for both cost the segment calls 9 - 17 %,
    // profiles/attn_global_keys.txt)
    auto block = [&](int k0) __attribute__((always_inline)) {
#include "attn_hd_dq_block.h"
    };
    if (P.k_glob == nullptr) {  // the walk as it was before the global keys: the band (or all), segment skips
      for (int k0 = kstart; k0 < kend; k0 += BKY) {
        if (seg_apart(P, b, q0, k0)) continue;
        block(k0);
      }
    } else {  // the band merged with the listed blocks outside it (no segments with global keys)
      BlockWalk walk(P, b, kstart, kend);
      for (int k0 = walk.next(P, -BKY); k0 != BlockWalk::DONE; k0 = walk.next(P, k0)) block(k0);
    }
  }
  // acc[dt][i] = dQ[row][d = 16 dt + 4 g + i] / scale
  if (row_ok) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
      if (16 * dt + 4 * g < P.D) st4(dqp + 16 * dt + 4 * g, acc[dt] * P.scale);
  }
}

template <int DP, bool DROP, bool LISTS = false, bool CAP = false>
__global__ __launch_bounds__(NT, occ_dkdv(DP)) void attn_hd_dkdv_kernel(AttnHdParams P) {
  constexpr int KS = DP / 32, DT = DP / 16;
  __shared__ __attribute__((aligned(16))) uint16_t Qs[Img<DP>::SIZE];
  __shared__ __attribute__((aligned(16))) uint16_t Os[Img<DP>::SIZE];  // dO
  __shared__ float Ls[2 * BQ];
  __shared__ float Rl[BQ], Rd[BQ];
  __shared__ uint32_t Rh[BQ];
  __shared__ __attribute__((aligned(16))) int Rs[BQ];  // the rows' segment ids (with segments)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
  const int bh = blockIdx.y, b = bh / P.H, h = bh % P.H;
  const int k0 = blockIdx.x * BKY;
  const int key = k0 + 16 * w + c;
  const int keyc = min(key, P.Sk - 1);
  bf16x8v kf[KS], vf[KS];
  load_row_frags<DP>(P.k + (long)b * P.k_sb + (long)keyc * P.k_ss + (long)h * P.k_sh, g, P.D, kf);
  load_row_frags<DP>(P.v + (long)b * P.v_sb + (long)keyc * P.v_ss + (long)h * P.v_sh, g, P.D, vf);
  const float dscale = DROP ? 1.f / (1.f - P.p_drop) : 1.f;
  const float scale2 = P.scale * LOG2E;
  // soft cap: x = c log2(e) tanh(scale s / c), tanh from exp2(2 log2(e) z) (tanh_ex2)
  const float capz2 = CAP ? P.scale / P.softcap * (2.f * LOG2E) : 0.f;
  const float capc2 = CAP ? P.softcap * LOG2E : 0.f;
  const uint32_t seed = DROP ? eff_seed(P.seed) : 0u;
  const bool kok = key_ok(P, b, key);
  const int ksg = P.q_seg ? seg_at(P.k_seg, b, P.Sk, key) : 0;
  f32x4 dk[DT], dv[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) {
    dk[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    dv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const uint16_t* qb = P.q + (long)b * P.q_sb + (long)h * P.q_sh;
  const uint16_t* ob = P.dout + (long)b * P.do_sb + (long)h * P.do_sh;
  int qstart = 0;
  if (P.causal) qstart = max(0, (k0 - P.causal_off) / BQ * BQ);
  int qend = P.Sq;
  bool glob_blk = false;  // the block holds a valid global key: every query block sees it
  int kwin = P.window;
  if constexpr (DP != 32) kwin = key_window(P, b, k0, key, kok, glob_blk);  // no global keys at head dim 32
  if (!glob_blk) band_range(P, k0, qstart, qend);
  if constexpr (LISTS) {
    // follow the key block's list of query blocks — the transpose of the key lists, repeats included
    int li, le;
    list_range(P, P.ql_ptr, h, (P.Sk + 63) / 64, (int)blockIdx.x, li, le);
    for (; li < le; ++li) {
      const int q0 = list_block(P.ql_idx, li, (P.Sq + 63) / 64);
      if (q0 < 0) continue;
#include "attn_hd_dkdv_block.h"
    }
  } else {
    for (int q0 = qstart; q0 < qend; q0 += BQ) {
      if (seg_apart(P, b, q0, k0)) continue;
#include "attn_hd_dkdv_block.h"
    }
  }
  // dk[dt][i] = dK[key][d = 16 dt + 4 g + i] / scale
  if (key < P.Sk) {
    uint16_t* dkp = P.dk + (long)b * P.dk_sb + (long)key * P.dk_ss + (long)h * P.dk_sh;
    uint16_t* dvp = P.dv + (long)b * P.dv_sb + (long)key * P.dv_ss + (long)h * P.dv_sh;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      if (16 * dt + 4 * g < P.D) {
        st4(dkp + 16 * dt + 4 * g, dk[dt] * P.scale);
        st4(dvp + 16 * dt + 4 * g, dv[dt]);
      }
    }
  }
}

template <int DP>
int launch_fwd(const AttnHdParams& P, hipStream_t st) {
  dim3 grid((P.Sq + BQ - 1) / BQ, P.B * P.H);
  if constexpr (DP != 32) {  // the instantiations that follow block lists (none at head dim 32: refused before)
    if (P.kl_ptr != nullptr) {
      if (P.p_drop > 0.f) hipLaunchKernelGGL((attn_hd_fwd_kernel<DP, true, true>), grid, dim3(NT), 0, st, P);
      else hipLaunchKernelGGL((attn_hd_fwd_kernel<DP, false, true>), grid, dim3(NT), 0, st, P);
      DLLM_CHECK_LAUNCH();
      return 0;
    }
  }
  if constexpr (DP != 32) {  // the instantiations that cap the scores (none at head dim 32, never with lists)
    if (P.softcap > 0.f) {
      if (P.p_drop > 0.f) hipLaunchKernelGGL((attn_hd_fwd_kernel<DP, true, false, true>), grid, dim3(NT), 0, st, P);
      else hipLaunchKernelGGL((attn_hd_fwd_kernel<DP, false, false, true>), grid, dim3(NT), 0, st, P);
      DLLM_CHECK_LAUNCH();
      return 0;
    }
  }
  if (P.p_drop > 0.f) hipLaunchKernelGGL((attn_hd_fwd_kernel<DP, true>), grid, dim3(NT), 0, st, P);
  else hipLaunchKernelGGL((attn_hd_fwd_kernel<DP, false>), grid, dim3(NT), 0, st, P);
  DLLM_CHECK_LAUNCH();
  return 0;
}

template <int DP>
int launch_bwd(const AttnHdParams& P, hipStream_t st) {
  dim3 gq((P.Sq + BQ - 1) / BQ, P.B * P.H), gk((P.Sk + BKY - 1) / BKY, P.B * P.H);
  if constexpr (DP != 32) {  // the instantiations that follow block lists, as in launch_fwd
    if (P.kl_ptr != nullptr) {
      if (P.p_drop > 0.f) {
        hipLaunchKernelGGL((attn_hd_dq_kernel<DP, true, true>), gq, dim3(NT), 0, st, P);
        hipLaunchKernelGGL((attn_hd_dkdv_kernel<DP, true, true>), gk, dim3(NT), 0, st, P);
      } else {
        hipLaunchKernelGGL((attn_hd_dq_kernel<DP, false, true>), gq, dim3(NT), 0, st, P);
        hipLaunchKernelGGL((attn_hd_dkdv_kernel<DP, false, true>), gk, dim3(NT), 0, st, P);
      }
      DLLM_CHECK_LAUNCH();
      return 0;
    }
  }
  if constexpr (DP != 32) {  // the instantiations that cap the scores, as in launch_fwd
    if (P.softcap > 0.f) {
      if (P.p_drop > 0.f) {
        hipLaunchKernelGGL((attn_hd_dq_kernel<DP, true, false, true>), gq, dim3(NT), 0, st, P);
        hipLaunchKernelGGL((attn_hd_dkdv_kernel<DP, true, false, true>), gk, dim3(NT), 0, st, P);
      } else {
        hipLaunchKernelGGL((attn_hd_dq_kernel<DP, false, false, true>), gq, dim3(NT), 0, st, P);
        hipLaunchKernelGGL((attn_hd_dkdv_kernel<DP, false, false, true>), gk, dim3(NT), 0, st, P);
      }
      DLLM_CHECK_LAUNCH();
      return 0;
    }
  }
  if (P.p_drop > 0.f) {
    hipLaunchKernelGGL((attn_hd_dq_kernel<DP, true>), gq, dim3(NT), 0, st, P);
    hipLaunchKernelGGL((attn_hd_dkdv_kernel<DP, true>), gk, dim3(NT), 0, st, P);
  } else {
    hipLaunchKernelGGL((attn_hd_dq_kernel<DP, false>), gq, dim3(NT), 0, st, P);
    hipLaunchKernelGGL((attn_hd_dkdv_kernel<DP, false>), gk, dim3(NT), 0, st, P);
  }
  DLLM_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// -1: head dim outside the kernels' range (the binding checks it first)
extern "C" int dllm_attn_hd_fwd(AttnHdParams* pp, hipStream_t st) {
  const AttnHdParams& P = *pp;
  if (P.D < 32 || P.D > 128 || P.D % 8) return -1;
  if (P.D == 32 && (P.k_glob != nullptr || P.kl_ptr != nullptr || P.softcap > 0.f)) return -2;  // the binding checks it
  if (P.softcap > 0.f && (P.kl_ptr != nullptr || P.lut != nullptr || P.q_seg != nullptr || P.k_glob != nullptr)) return -2;
  switch ((P.D + 31) / 32) {
    case 1: return launch_fwd<32>(P, st);
    case 2: return launch_fwd<64>(P, st);
    case 3: return launch_fwd<96>(P, st);
    default: return launch_fwd<128>(P, st);
  }
}

extern "C" int dllm_attn_hd_bwd(AttnHdParams* pp, hipStream_t st) {
  const AttnHdParams& P = *pp;
  if (P.D < 32 || P.D > 128 || P.D % 8) return -1;
  if (P.D == 32 && (P.k_glob != nullptr || P.kl_ptr != nullptr || P.softcap > 0.f)) return -2;
  if (P.softcap > 0.f && (P.kl_ptr != nullptr || P.lut != nullptr || P.q_seg != nullptr || P.k_glob != nullptr)) return -2;
  const long rows = (long)P.B * P.H * P.Sq;
  hipLaunchKernelGGL(attn_hd_delta_kernel, dim3((unsigned)((rows + NT / 16 - 1) / (NT / 16))), dim3(NT), 0, st, P);
  DLLM_CHECK_LAUNCH();
  switch ((P.D + 31) / 32) {
    case 1: return launch_bwd<32>(P, st);
    case 2: return launch_bwd<64>(P, st);
    case 3: return launch_bwd<96>(P, st);
    default: return launch_bwd<128>(P, st);
  }
}
