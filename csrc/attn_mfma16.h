// Tile helpers shared by the two bf16 attention families on v_mfma_f32_16x16x32_bf16, csrc/attn_hd.hip (head dims up to
// 128) and csrc/attn_wide.hip (head dims up to 256, grouped K/V heads): the row-major LDS image of a 64-row tile
// templated on the padded head dim DP, its staging, the operand fragments read from it along either axis, and the
// "two packed accumulator tiles are the next B operand" packing csrc/attn_hd.hip's header explains.
#pragma once
#include "common.h"
#include "attn_small.h"

namespace {

using namespace dllm;

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

}  // namespace
