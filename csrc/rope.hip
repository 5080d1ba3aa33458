// Rotary position embedding (rotate-half, Gemma 2 / T5Gemma self-attention), in place, for gfx950.
//
// x is a [B, S, n, H, D] view (head dim contiguous): the n listed slots of a packed projection output — q and k of a
// fused qkv, or a lone q or k — each with H heads of D columns; v is simply not part of the view.  For the token at
// position p = pos[b][s] (pos [B, S], or [S] shared by the batch) every head's halves x1 = x[.. d], x2 = x[.. d + D/2]
// (d < D / 2) become
//     x1' = x1 cos[p][d] - sign x2 sin[p][d],   x2' = x2 cos[p][d] + sign x1 sin[p][d]
// with cos / sin fp32 [max_pos, D / 2] built on the host (ops/rope.py rope_table).  sign = 1 is the forward; the
// rotation is orthogonal, so the backward is the same kernel on the gradient with sign = -1.  Products and sums are
// fp32, with the first product's rounding error compensated so that a cancelling pair keeps fp32's relative accuracy,
// and the result is rounded once to the tensor's dtype.
//
// One lane owns one 16-byte chunk of each half (8 bf16 / 4 fp32 columns d .. and the same columns + D / 2): two 16-B
// loads, two 16-B stores, the matching cos / sin floats; no LDS, nothing shared between lanes.  Memory-bound: x is read
// once and written once.  D % 16 == 0 (bf16) / D % 8 == 0 (fp32), 16-byte aligned rows: the binding checks.  A
// position outside [0, max_pos) is clamped to the table (the op checks lengths against the table on the host).
#include "common.h"

using namespace dllm;

namespace {

template <typename T>
__global__ __launch_bounds__(256) void rope_kernel(T* __restrict__ x, long sb, long ss, long sn, long sh, int n, int S,
                                                   int H, int D, const int* __restrict__ pos, long pos_sb,
                                                   const float* __restrict__ cos, const float* __restrict__ sin,
                                                   int max_pos, float sign, long total) {
  constexpr int E = 16 / (int)sizeof(T);  // columns per 16-B chunk
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int half = D / 2, cpr = half / E;
  const int ch = (int)(i % cpr);
  long r = i / cpr;
  const int h = (int)(r % H);
  r /= H;
  const int slot = (int)(r % n);
  r /= n;
  const int s = (int)(r % S);
  const long b = r / S;
  int p = pos[b * pos_sb + s];
  p = min(max(p, 0), max_pos - 1);
  T* x1 = x + b * sb + (long)s * ss + (long)slot * sn + (long)h * sh + ch * E;
  T* x2 = x1 + half;
  const float* cp = cos + (long)p * half + ch * E;
  const float* sp = sin + (long)p * half + ch * E;
  float a[E], c[E], cs[E], sn_[E];
  if constexpr (sizeof(T) == 2) {
    const u16x8 va = *reinterpret_cast<const u16x8*>(x1), vc = *reinterpret_cast<const u16x8*>(x2);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      a[k] = bf2f(va[k]);
      c[k] = bf2f(vc[k]);
    }
  } else {
    const f32x4 va = *reinterpret_cast<const f32x4*>(x1), vc = *reinterpret_cast<const f32x4*>(x2);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      a[k] = va[k];
      c[k] = vc[k];
    }
  }
#pragma unroll
  for (int k = 0; k < E; k += 4) {
    const f32x4 cv = *reinterpret_cast<const f32x4*>(cp + k), sv = *reinterpret_cast<const f32x4*>(sp + k);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cs[k + j] = cv[j];
      sn_[k + j] = sv[j] * sign;
    }
  }
  float o1[E], o2[E];
#pragma unroll
  for (int k = 0; k < E; ++k) {
    // a c - b s with the rounding error of the first product carried along (e = b s - fl(b s), exact from one fma):
    // where the two products cancel, the difference still has fp32's relative accuracy, not the products'
    const float p1 = c[k] * sn_[k], e1 = fmaf(c[k], sn_[k], -p1);
    const float p2 = a[k] * sn_[k], e2 = fmaf(a[k], sn_[k], -p2);
    o1[k] = fmaf(a[k], cs[k], -p1) - e1;
    o2[k] = fmaf(c[k], cs[k], p2) + e2;
  }
  if constexpr (sizeof(T) == 2) {
    const u32x4 w1 = {pack_bf16x2(o1[0], o1[1]), pack_bf16x2(o1[2], o1[3]), pack_bf16x2(o1[4], o1[5]),
                      pack_bf16x2(o1[6], o1[7])};
    const u32x4 w2 = {pack_bf16x2(o2[0], o2[1]), pack_bf16x2(o2[2], o2[3]), pack_bf16x2(o2[4], o2[5]),
                      pack_bf16x2(o2[6], o2[7])};
    *reinterpret_cast<u32x4*>(x1) = w1;
    *reinterpret_cast<u32x4*>(x2) = w2;
  } else {
    *reinterpret_cast<f32x4*>(x1) = f32x4{o1[0], o1[1], o1[2], o1[3]};
    *reinterpret_cast<f32x4*>(x2) = f32x4{o2[0], o2[1], o2[2], o2[3]};
  }
}

}  // namespace

// -2: a shape the kernel does not take (the binding checks it first)
extern "C" int dllm_rope(void* x, long x_sb, long x_ss, long x_sn, long x_sh, int n, int B, int S, int H, int D,
                         const int* pos, long pos_sb, const float* cos, const float* sin, int max_pos, float sign,
                         int is_bf16, hipStream_t st) {
  const int E = is_bf16 ? 8 : 4;
  if (B <= 0 || S <= 0 || n <= 0 || H <= 0 || D <= 0 || D % (2 * E) || max_pos <= 0) return -2;
  const long total = (long)B * S * n * H * (D / 2 / E);
  const long blocks = (total + 255) / 256;
  if (blocks >= (1L << 31)) return -2;
  if (is_bf16)
    hipLaunchKernelGGL(rope_kernel<uint16_t>, dim3((unsigned)blocks), dim3(256), 0, st, (uint16_t*)x, x_sb, x_ss, x_sn,
                       x_sh, n, S, H, D, pos, pos_sb, cos, sin, max_pos, sign, total);
  else
    hipLaunchKernelGGL(rope_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (float*)x, x_sb, x_ss, x_sn, x_sh,
                       n, S, H, D, pos, pos_sb, cos, sin, max_pos, sign, total);
  DLLM_CHECK_LAUNCH();
  return 0;
}
