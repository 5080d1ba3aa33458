// Row walk of the loss kernels over [N, V] logits (csrc/ce.hip, csrc/kd.hip).
#pragma once
#include "common.h"

namespace dllm {

// Rows of any length V: row r starts at logits + r * V, 16-B aligned only when V is a multiple of 16 / sizeof(T)
// (BART's V = 50265 is odd).  Each row is walked as a scalar head up to the first 16-B boundary, 16-B vectors (8 bf16
// or 4 fp32 per thread and step: one global_load_dwordx4), and a scalar tail — every row at the vector rate whatever
// its alignment (an odd V with element-wise loads ran at 1.5-2.3 TB/s on bart-large 1024/1024, r5 profile).
template <typename T>
DLLM_DEVICE int row_head(const T* p, int V) {
  const int mis = (int)(reinterpret_cast<uintptr_t>(p) & 15);
  return min(V, ((16 - mis) & 15) / (int)sizeof(T));
}

typedef u16x8 __attribute__((aligned(2))) u16x8_e;  // element-aligned 16-B groups
typedef f32x4 __attribute__((aligned(4))) f32x4_e;

template <typename T>
struct Vec16 {
  static constexpr int N = 16 / (int)sizeof(T);
  DLLM_DEVICE static void load(const T* p, float (&v)[16 / sizeof(T)]) {  // p 16-B aligned
    if constexpr (sizeof(T) == 2) {
      const u16x8 u = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = bf2f(u[k]);
    } else {
      const f32x4 u = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = u[k];
    }
  }
  // p at any element: a row walked on ANOTHER row's boundaries (csrc/kd.hip).  The compiler emits whatever the
  // target's unaligned-access mode allows (one dwordx4 on gfx950).
  DLLM_DEVICE static void load_e(const T* p, float (&v)[16 / sizeof(T)]) {
    if constexpr (sizeof(T) == 2) {
      const u16x8 u = *reinterpret_cast<const u16x8_e*>(p);
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = bf2f(u[k]);
    } else {
      const f32x4 u = *reinterpret_cast<const f32x4_e*>(p);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = u[k];
    }
  }
  DLLM_DEVICE static void store(T* p, const float (&v)[16 / sizeof(T)]) {  // p 16-B aligned
    if constexpr (sizeof(T) == 2) {
      u16x8 u;
#pragma unroll
      for (int k = 0; k < 8; ++k) u[k] = f2bf(v[k]);
      *reinterpret_cast<u16x8*>(p) = u;
    } else {
      *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
    }
  }
};

// eps * mean_v(x_v).  Without smoothing the term is left out, not multiplied by 0: a banned token's -inf logit (BART
// final_logits_bias) makes the row's sum of logits -inf, and 0 * -inf would turn a finite loss into NaN.
DLLM_DEVICE float smooth_term(float eps, float sum_x, int V) { return eps != 0.f ? eps * sum_x / (float)V : 0.f; }

// bias[i .. i + 3] of a vocabulary chunk: one 16-B load when that address is 16-B aligned, else four scalar loads (the
// ragged vocab tail chunk starts at c0 = V - Vc, odd for BART's V = 50265)
DLLM_DEVICE f32x4 bias4(const float* __restrict__ bias, int i) {
  if ((i & 3) == 0) return *reinterpret_cast<const f32x4*>(bias + i);
  return f32x4{bias[i], bias[i + 1], bias[i + 2], bias[i + 3]};
}

}  // namespace dllm
