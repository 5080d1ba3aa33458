// Fused (label-smoothed) cross-entropy on LM-head logits, for gfx950.
// fwd: one 256-thread block per row: online max/sum-exp over V (fp32 math on bf16 logits, optional
//      additive fp32 bias = BART final_logits_bias), writes loss_row and lse.
//      loss = lse - (1-eps)*x_y - eps*mean_v(x_v);  ignored rows (label == ignore_index) -> 0.
// bwd: dx_v = g * (exp(x_v - lse) - eps/V - (1-eps)*[v==y]) with g = *scale (device scalar, no host
//      sync), written as bf16 — optionally in place over the logits (the only consumer).
// Soft cap (Gemma 2 / T5Gemma final_logit_softcapping, template parameter CAP): every kernel reads x' = c tanh(x / c)
// where it read x (after the bias), in the same single pass; the backward writes dx = dx' (1 - tanh^2).  tanh is the
// device library's tanhf.  Without a cap the kernels are the code they were.
#include "common.h"
#include "row_walk.h"

using namespace dllm;

namespace {

// x' = c tanh(x / c) (inv = 1 / c), or x itself without a cap
template <bool CAP>
DLLM_DEVICE float capped(float v, float cap, float inv) {
  if constexpr (CAP) return cap * tanhf(v * inv);
  else return v;
}
// g (p - off - hit) on the capped logit, times the cap's derivative 1 - tanh^2
template <bool CAP>
DLLM_DEVICE float capped_grad(float v, float lse, float g, float sub, float cap, float inv) {
  if constexpr (CAP) {
    const float th = tanhf(v * inv);
    return g * (__expf(cap * th - lse) - sub) * (1.f - th * th);
  } else {
    return g * (__expf(v - lse) - sub);
  }
}

template <typename T, bool CAP>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ labels,
                                                     const float* __restrict__ bias, float* __restrict__ loss_out,
                                                     float* __restrict__ lse_out, int V, float eps, long ignore,
                                                     float cap) {
  __shared__ float red[4];
  constexpr int E = Vec16<T>::N;
  const float inv = CAP ? 1.f / cap : 0.f;
  const long row = blockIdx.x;
  const T* x = logits + row * (long)V;
  float m = -INFINITY, s = 0.f, sx = 0.f;
  auto add1 = [&](float v) {
    const float nm = fmaxf(m, v);
    if (nm != -INFINITY) {
      s = (m == -INFINITY ? 0.f : s * __expf(m - nm)) + __expf(v - nm);
      m = nm;
    }
    sx += v;
  };
  const int head = row_head(x, V);
  const int nvec = (V - head) / E;
  const int body_end = head + nvec * E;
  if ((int)threadIdx.x < head)
    add1(capped<CAP>(Elem<T>::load(x + threadIdx.x) + (bias != nullptr ? bias[threadIdx.x] : 0.f), cap, inv));
  for (int c = head + (int)threadIdx.x * E; c < body_end; c += 256 * E) {
    float v[E];
    Vec16<T>::load(x + c, v);
    if (bias != nullptr) {
#pragma unroll
      for (int k = 0; k < E; ++k) v[k] += bias[c + k];
    }
    if constexpr (CAP) {
#pragma unroll
      for (int k = 0; k < E; ++k) v[k] = capped<CAP>(v[k], cap, inv);
    }
    float lm = v[0];
#pragma unroll
    for (int k = 1; k < E; ++k) lm = fmaxf(lm, v[k]);
    const float nm = fmaxf(m, lm);
    if (nm != -INFINITY) {
      float e = 0.f;
#pragma unroll
      for (int k = 0; k < E; ++k) e += __expf(v[k] - nm);
      s = (m == -INFINITY ? 0.f : s * __expf(m - nm)) + e;
      m = nm;
    }
#pragma unroll
    for (int k = 0; k < E; ++k) sx += v[k];
  }
  for (int c = body_end + (int)threadIdx.x; c < V; c += 256)
    add1(capped<CAP>(Elem<T>::load(x + c) + (bias != nullptr ? bias[c] : 0.f), cap, inv));
  const float M = block_max<256>(m, red);
  const float scaled = (m == -INFINITY) ? 0.f : s * __expf(m - M);
  const float S = block_sum<256>(scaled, red);
  const float SX = block_sum<256>(sx, red);
  if (threadIdx.x == 0) {
    const float lse = M + __logf(S);
    const long y = labels[row];
    float loss = 0.f;
    if (y != ignore && y >= 0 && y < V) {
      float xy = Elem<T>::load(x + y);
      if (bias != nullptr) xy += bias[y];
      xy = capped<CAP>(xy, cap, inv);
      loss = lse - (1.f - eps) * xy - smooth_term(eps, SX, V);
    }
    loss_out[row] = loss;
    lse_out[row] = lse;
  }
}

template <typename T, bool CAP>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ scale, const T* __restrict__ logits,
                                                     const int64_t* __restrict__ labels,
                                                     const float* __restrict__ lse_in, const float* __restrict__ bias,
                                                     T* __restrict__ dlogits, int V, float eps, long ignore,
                                                     float cap) {
  constexpr int E = Vec16<T>::N;
  const float inv = CAP ? 1.f / cap : 0.f;
  const long row = blockIdx.x;
  const T* x = logits + row * (long)V;
  T* dx = dlogits + row * (long)V;
  const long y = labels[row];
  const bool valid = (y != ignore && y >= 0 && y < V);
  const float g = valid ? scale[0] : 0.f;
  const float lse = lse_in[row];
  const float off = eps / (float)V;
  const float hit = 1.f - eps;
  auto one = [&](int c) {
    const float v = Elem<T>::load(x + c) + (bias != nullptr ? bias[c] : 0.f);
    if constexpr (CAP) Elem<T>::store(dx + c, capped_grad<CAP>(v, lse, g, off + (c == y ? hit : 0.f), cap, inv));
    else Elem<T>::store(dx + c, g * (__expf(v - lse) - off - (c == y ? hit : 0.f)));
  };
  // vector body only when input and output rows share their 16-B phase (in place, or equally aligned buffers)
  if (((reinterpret_cast<uintptr_t>(x) ^ reinterpret_cast<uintptr_t>(dx)) & 15) != 0) {
    for (int c = threadIdx.x; c < V; c += 256) one(c);
    return;
  }
  const int head = row_head(x, V);
  const int body_end = head + ((V - head) / E) * E;
  if ((int)threadIdx.x < head) one(threadIdx.x);
  for (int c = head + (int)threadIdx.x * E; c < body_end; c += 256 * E) {
    float v[E];
    Vec16<T>::load(x + c, v);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const float b = bias != nullptr ? bias[c + k] : 0.f;
      if constexpr (CAP) v[k] = capped_grad<CAP>(v[k] + b, lse, g, off + ((c + k) == y ? hit : 0.f), cap, inv);
      else v[k] = g * (__expf(v[k] + b - lse) - off - ((c + k) == y ? hit : 0.f));
    }
    Vec16<T>::store(dx + c, v);
  }
  for (int c = body_end + (int)threadIdx.x; c < V; c += 256) one(c);
}

// ---- vocab-chunked LM head + CE (ops/lm_head.py): the logits exist one [N, Vc] chunk at a time
// Per row running state st[row] = {max, sum exp(x - max), sum x, x_label} merged over chunks; the last chunk writes
// loss_row and lse.  Chunk columns are global vocab ids c0 .. c0 + Vc - 1; eps / V uses the full vocab size.
template <bool CAP>
__global__ __launch_bounds__(256) void ce_chunk_fwd_kernel(const uint16_t* __restrict__ logits, long ld,
                                                           const int64_t* __restrict__ labels,
                                                           const float* __restrict__ bias, f32x4* __restrict__ st,
                                                           float* __restrict__ loss_out, float* __restrict__ lse_out,
                                                           int Vc, int c0, int V, float eps, long ignore, int first,
                                                           int last, int skip, float cap) {
  __shared__ float red[4];
  const float inv = CAP ? 1.f / cap : 0.f;
  const long row = blockIdx.x;
  const uint16_t* x = logits + row * ld;
  float m = -INFINITY, s = 0.f, sx = 0.f;
  for (int c = threadIdx.x * 4; c < Vc; c += 256 * 4) {  // Vc % 4 == 0
    f32x4 v = Elem<uint16_t>::load4(x + c);
    if (bias != nullptr) v += bias4(bias, c0 + c);
    if constexpr (CAP) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = capped<CAP>(v[k], cap, inv);
    }
    if (c < skip) {  // leading columns already covered by the previous chunk (ragged vocab tail)
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = c + k < skip ? -INFINITY : v[k];
    }
    const float lm = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
    const float nm = fmaxf(m, lm);
    if (nm != -INFINITY) {
      s = s * __expf(m - nm) + __expf(v.x - nm) + __expf(v.y - nm) + __expf(v.z - nm) + __expf(v.w - nm);
      m = nm;
    }
    if (c < skip) {
#pragma unroll
      for (int k = 0; k < 4; ++k) sx += c + k < skip ? 0.f : v[k];
    } else {
      sx += (v.x + v.y) + (v.z + v.w);
    }
  }
  const float M = block_max<256>(m, red);
  const float scaled = (m == -INFINITY) ? 0.f : s * __expf(m - M);
  const float S = block_sum<256>(scaled, red);
  const float SX = block_sum<256>(sx, red);
  if (threadIdx.x == 0) {
    const long y = labels[row];
    f32x4 cur = first ? f32x4{-INFINITY, 0.f, 0.f, 0.f} : st[row];
    const float nm = fmaxf(cur.x, M);
    cur.y = (cur.x == -INFINITY ? 0.f : cur.y * __expf(cur.x - nm)) + (M == -INFINITY ? 0.f : S * __expf(M - nm));
    cur.x = nm;
    cur.z += SX;
    if (y >= c0 + skip && y < c0 + Vc)
      cur.w = capped<CAP>(Elem<uint16_t>::load(x + (y - c0)) + (bias != nullptr ? bias[y] : 0.f), cap, inv);
    st[row] = cur;
    if (last) {
      const float lse = cur.x + __logf(cur.y);
      const bool valid = y != ignore && y >= 0 && y < V;
      loss_out[row] = valid ? lse - (1.f - eps) * cur.w - smooth_term(eps, cur.z, V) : 0.f;
      lse_out[row] = lse;
    }
  }
}

// dlogits of one chunk, in place: g * (exp(x - lse) - eps / V - (1 - eps) [c0 + col == y])
template <bool CAP>
__global__ __launch_bounds__(256) void ce_chunk_bwd_kernel(const float* __restrict__ scale, uint16_t* __restrict__ x_io,
                                                           long ld, const int64_t* __restrict__ labels,
                                                           const float* __restrict__ lse_in,
                                                           const float* __restrict__ bias, int Vc, int c0, int V,
                                                           float eps, long ignore, int skip, float cap) {
  const float inv = CAP ? 1.f / cap : 0.f;
  const long row = blockIdx.x;
  uint16_t* x = x_io + row * ld;
  const long y = labels[row];
  const bool valid = (y != ignore && y >= 0 && y < V);
  const float g = valid ? scale[0] : 0.f;
  const float lse = lse_in[row];
  const float off = eps / (float)V;
  const float hit = 1.f - eps;
  const long yl = y - c0;
  for (int c = threadIdx.x * 4; c < Vc; c += 256 * 4) {
    f32x4 v = Elem<uint16_t>::load4(x + c);
    if (bias != nullptr) v += bias4(bias, c0 + c);
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if constexpr (CAP)
        r[k] = c + k < skip ? 0.f : capped_grad<CAP>(v[k], lse, g, off + ((c + k) == yl ? hit : 0.f), cap, inv);
      else
        r[k] = c + k < skip ? 0.f : g * (__expf(v[k] - lse) - off - ((c + k) == yl ? hit : 0.f));
    Elem<uint16_t>::store4(x + c, r);
  }
}

// LM-head CE forward, fused path (ops/lm_head.py): merge the per-(row, 128-column) online-softmax partials the
// W4_EPI_CEF GEMM epilogue wrote (csrc/gemm_w4.hip) into the row's lse and loss.  One wave per row.
__global__ __launch_bounds__(256) void ce_merge_kernel(const f32x4* __restrict__ part, int np, long pstride,
                                                       const float* __restrict__ xlab, const int64_t* __restrict__ labels,
                                                       float* __restrict__ loss_out, float* __restrict__ lse_out, long N,
                                                       int V, float eps, long ignore) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= N) return;
  const f32x4* pr = part + row * pstride;
  float m = -INFINITY, s = 0.f, sx = 0.f;
  for (int c = lane; c < np; c += 64) {
    const f32x4 v = pr[c];
    const float nm = fmaxf(m, v.x);
    if (nm != -INFINITY) {
      s = (m == -INFINITY ? 0.f : s * __expf(m - nm)) + (v.x == -INFINITY ? 0.f : v.y * __expf(v.x - nm));
      m = nm;
    }
    sx += v.z;
  }
  const float M = wave_max(m);
  const float S = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - M));
  const float SX = wave_sum(sx);
  if (lane == 0) {
    const long y = labels[row];
    const bool valid = y != ignore && y >= 0 && y < V;
    const float lse = M + __logf(S);
    loss_out[row] = valid ? lse - (1.f - eps) * xlab[row] - smooth_term(eps, SX, V) : 0.f;
    lse_out[row] = lse;
  }
}

}  // namespace

extern "C" int dllm_ce_chunk_fwd(const void* logits, long ld, const int64_t* labels, const float* bias, float* state,
                                 float* loss, float* lse, long N, int Vc, int c0, int V, float eps, long ignore,
                                 int first, int last, int skip, float cap, hipStream_t st) {
  if (Vc % 4 || ld % 4 || N <= 0 || skip < 0 || skip >= Vc || !(cap >= 0.f)) return -2;
  if (cap > 0.f)
    hipLaunchKernelGGL(ce_chunk_fwd_kernel<true>, dim3(N), dim3(256), 0, st, (const uint16_t*)logits, ld, labels, bias,
                       (f32x4*)state, loss, lse, Vc, c0, V, eps, ignore, first, last, skip, cap);
  else
    hipLaunchKernelGGL(ce_chunk_fwd_kernel<false>, dim3(N), dim3(256), 0, st, (const uint16_t*)logits, ld, labels, bias,
                       (f32x4*)state, loss, lse, Vc, c0, V, eps, ignore, first, last, skip, cap);
  DLLM_CHECK_LAUNCH();
  return 0;
}

extern "C" int dllm_ce_chunk_bwd(const float* scale, void* logits, long ld, const int64_t* labels, const float* lse,
                                 const float* bias, long N, int Vc, int c0, int V, float eps, long ignore, int skip,
                                 float cap, hipStream_t st) {
  if (Vc % 4 || ld % 4 || N <= 0 || skip < 0 || skip >= Vc || !(cap >= 0.f)) return -2;
  if (cap > 0.f)
    hipLaunchKernelGGL(ce_chunk_bwd_kernel<true>, dim3(N), dim3(256), 0, st, scale, (uint16_t*)logits, ld, labels, lse,
                       bias, Vc, c0, V, eps, ignore, skip, cap);
  else
    hipLaunchKernelGGL(ce_chunk_bwd_kernel<false>, dim3(N), dim3(256), 0, st, scale, (uint16_t*)logits, ld, labels, lse,
                       bias, Vc, c0, V, eps, ignore, skip, cap);
  DLLM_CHECK_LAUNCH();
  return 0;
}

extern "C" int dllm_ce_fwd(const void* logits, const int64_t* labels, const float* bias, float* loss, float* lse,
                           long N, int V, float eps, long ignore, int is_bf16, float cap, hipStream_t st) {
  dim3 g(N), b(256);
  if (!(cap >= 0.f)) return -2;
#define L(T, CAP)                                                                                                  \
  hipLaunchKernelGGL((ce_fwd_kernel<T, CAP>), g, b, 0, st, (const T*)logits, labels, bias, loss, lse, V, eps, ignore, cap)
  if (is_bf16) {
    if (cap > 0.f) L(uint16_t, true);
    else L(uint16_t, false);
  } else {
    if (cap > 0.f) L(float, true);
    else L(float, false);
  }
#undef L
  DLLM_CHECK_LAUNCH();
  return 0;
}

extern "C" int dllm_ce_bwd(const float* scale, const void* logits, const int64_t* labels, const float* lse,
                           const float* bias, void* dlogits, long N, int V, float eps, long ignore, int is_bf16,
                           float cap, hipStream_t st) {
  dim3 g(N), b(256);
  if (!(cap >= 0.f)) return -2;
#define L(T, CAP)                                                                                                   \
  hipLaunchKernelGGL((ce_bwd_kernel<T, CAP>), g, b, 0, st, scale, (const T*)logits, labels, lse, bias, (T*)dlogits, V, \
                     eps, ignore, cap)
  if (is_bf16) {
    if (cap > 0.f) L(uint16_t, true);
    else L(uint16_t, false);
  } else {
    if (cap > 0.f) L(float, true);
    else L(float, false);
  }
#undef L
  DLLM_CHECK_LAUNCH();
  return 0;
}

extern "C" int dllm_ce_merge(const float* part, int np, long pstride, const float* xlab, const int64_t* labels,
                             float* loss, float* lse, long N, int V, float eps, long ignore, hipStream_t st) {
  if (N <= 0 || np <= 0 || pstride < np) return -2;
  hipLaunchKernelGGL(ce_merge_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, (const f32x4*)part, np, pstride,
                     xlab, labels, loss, lse, N, V, eps, ignore);
  DLLM_CHECK_LAUNCH();
  return 0;
}
