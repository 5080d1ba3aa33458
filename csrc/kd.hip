// Fused knowledge-distillation loss on a pair of LM-head logits tensors, for gfx950 (ops/distill.py).
// Per row, with student logits s (+ bias_s), teacher logits t (+ bias_t), label y, smoothing eps, temperature T:
//   ce = lse(s) - (1-eps) s_y - eps mean_v(s_v)                                   (what csrc/ce.hip computes)
//   kl = sum_v p_v (log p_v - log q_v),  p = softmax(t/T), q = softmax(s/T)
//      = (1/T) sum_v p_v (t_v - s_v) - lse(t/T) + lse(s/T)
// fwd: one 256-thread block per row, ONE pass that reads both rows once and keeps three online softmaxes
//      {m_s, sum exp(s-m_s), sum exp((s-m_s)/T)}, {m_t, sum exp((t-m_t)/T), A = sum exp((t-m_t)/T) (t-s)} and sum s;
//      writes ce_row, kl_row and stats[row] = {lse(s), lse(s/T), lse(t/T)}.  T == 1 (template) drops the second
//      student exponential: lse(s/T) is lse(s).
// bwd: ds_v = w_ce (softmax(s)_v - eps/V - (1-eps)[v==y]) + w_kl T (q_v - p_v), w_ce / w_kl device scalars (no host
//      sync), written in the logits dtype, optionally in place over the student logits.  The teacher gets no gradient.
// -inf logits: a column with p_v = 0 adds nothing to kl whatever s_v is; p_v > 0 with s_v = -inf gives kl = +inf (not
//      NaN); with eps == 0 the smoothing term is absent (row_walk.h smooth_term), so ce stays finite with -inf off the
//      label; the gradient is finite wherever stats is.
// No atomics: every sum has a fixed order, reruns are bit-identical.
#include "common.h"
#include "row_walk.h"

using namespace dllm;

namespace {

// Row walk of csrc/ce.hip (row_walk.h): a scalar head up to the first 16-B boundary, 16-B vectors, a scalar tail.
// Three rows are walked together here (student, teacher, output) and each may sit at its own 16-B phase (V odd, views
// into larger buffers).  The boundaries come from ONE row (the output's in bwd, where the stores must be whole
// vectors; the student's in fwd); the other rows' 16-B groups are read through element-aligned vector types
// (Vec16::load_e), for which the compiler emits whatever the target's unaligned-access mode allows (one dwordx4 on
// gfx950) — no row's alignment is assumed from another's.

// -inf logits (a banned token: BART's final_logits_bias).  A column whose teacher weight w = exp((t - m_t)/T) is 0
// contributes nothing to A, whatever s is: w (t - s) would be 0 * -inf, or 0 * NaN when both models ban the column.
// A column with w > 0 and s = -inf makes A, and with it kl, +inf; such an A is carried through a rescale whose factor
// has underflowed to 0 as 0 (its columns' weights are 0 at the new maximum), never as inf * 0.
DLLM_DEVICE float kd_term(float w, float d) { return w != 0.f ? w * d : 0.f; }
DLLM_DEVICE float kd_rescale(float a, float f) { return f != 0.f ? a * f : 0.f; }

// Per-thread running state of the three softmaxes of one row.
template <bool T1>
struct KdAcc {
  float ms = -INFINITY, zs = 0.f, zsT = 0.f, sx = 0.f;  // student: max, sum exp(s-ms), sum exp((s-ms)/T), sum s
  float mt = -INFINITY, zt = 0.f, A = 0.f;              // teacher: max, sum exp((t-mt)/T), sum exp((t-mt)/T)(t-s)

  // E columns at once: ONE rescale per group and softmax
  template <int E>
  DLLM_DEVICE void add(const float (&s)[E], const float (&t)[E], float invT) {
    float ls = s[0], lt = t[0];
#pragma unroll
    for (int k = 1; k < E; ++k) {
      ls = fmaxf(ls, s[k]);
      lt = fmaxf(lt, t[k]);
    }
    const float ns = fmaxf(ms, ls);
    if (ns != -INFINITY) {
      float e = 0.f, eT = 0.f;
#pragma unroll
      for (int k = 0; k < E; ++k) {
        e += __expf(s[k] - ns);
        if constexpr (!T1) eT += __expf((s[k] - ns) * invT);
      }
      const float d = ms - ns;  // <= 0; -inf on the first group
      zs = (ms == -INFINITY ? 0.f : zs * __expf(d)) + e;
      if constexpr (!T1) zsT = (ms == -INFINITY ? 0.f : zsT * __expf(d * invT)) + eT;
      ms = ns;
    }
    const float nt = fmaxf(mt, lt);
    if (nt != -INFINITY) {
      float e = 0.f, a = 0.f;
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const float w = __expf((t[k] - nt) * invT);
        e += w;
        a += w * (t[k] - s[k]);
      }
      const float f = mt == -INFINITY ? 0.f : __expf((mt - nt) * invT);
      float An = A * f + a;
      if (An != An) {  // a zero weight met an infinite factor (0 * inf): the group again, by the rules above.  The
        a = 0.f;       // selects stay out of the common path: one per column cost the T != 1 forward 2 %.
#pragma unroll
        for (int k = 0; k < E; ++k) a += kd_term(__expf((t[k] - nt) * invT), t[k] - s[k]);
        An = kd_rescale(A, f) + a;
      }
      zt = zt * f + e;
      A = An;
      mt = nt;
    }
#pragma unroll
    for (int k = 0; k < E; ++k) sx += s[k];
  }
};

// Block-wide merge of the per-thread states; every thread returns the row's totals.
struct KdRow {
  float Ms, Zs, ZsT, SX, Mt, Zt, A;
};

template <bool T1>
DLLM_DEVICE KdRow kd_block_merge(const KdAcc<T1>& a, float invT, float* red) {
  KdRow r;
  r.Ms = block_max<256>(a.ms, red);
  const float ds = a.ms - r.Ms;
  r.Zs = block_sum<256>(a.ms == -INFINITY ? 0.f : a.zs * __expf(ds), red);
  r.ZsT = T1 ? r.Zs : block_sum<256>(a.ms == -INFINITY ? 0.f : a.zsT * __expf(ds * invT), red);
  r.SX = block_sum<256>(a.sx, red);
  r.Mt = block_max<256>(a.mt, red);
  const float ft = a.mt == -INFINITY ? 0.f : __expf((a.mt - r.Mt) * invT);
  r.Zt = block_sum<256>(a.zt * ft, red);
  r.A = block_sum<256>(kd_rescale(a.A, ft), red);
  return r;
}

template <typename T, bool T1>
__global__ __launch_bounds__(256) void kd_fwd_kernel(const T* __restrict__ student, const T* __restrict__ teacher,
                                                     const int64_t* __restrict__ labels,
                                                     const float* __restrict__ bias_s,
                                                     const float* __restrict__ bias_t, float* __restrict__ ce_out,
                                                     float* __restrict__ kl_out, float* __restrict__ stats, int V,
                                                     float eps, long ignore, float invT) {
  __shared__ float red[4];
  constexpr int E = Vec16<T>::N;
  const long row = blockIdx.x;
  const T* x = student + row * (long)V;
  const T* tt = teacher + row * (long)V;
  KdAcc<T1> acc;
  auto add1 = [&](int c) {
    const float s[1] = {Elem<T>::load(x + c) + (bias_s != nullptr ? bias_s[c] : 0.f)};
    const float t[1] = {Elem<T>::load(tt + c) + (bias_t != nullptr ? bias_t[c] : 0.f)};
    acc.template add<1>(s, t, invT);
  };
  const int head = row_head(x, V);
  const int body_end = head + ((V - head) / E) * E;
  if ((int)threadIdx.x < head) add1(threadIdx.x);
  for (int c = head + (int)threadIdx.x * E; c < body_end; c += 256 * E) {
    float s[E], t[E];
    Vec16<T>::load_e(x + c, s);
    Vec16<T>::load_e(tt + c, t);
    if (bias_s != nullptr) {
#pragma unroll
      for (int k = 0; k < E; ++k) s[k] += bias_s[c + k];
    }
    if (bias_t != nullptr) {
#pragma unroll
      for (int k = 0; k < E; ++k) t[k] += bias_t[c + k];
    }
    acc.template add<E>(s, t, invT);
  }
  for (int c = body_end + (int)threadIdx.x; c < V; c += 256) add1(c);
  const KdRow r = kd_block_merge<T1>(acc, invT, red);
  if (threadIdx.x == 0) {
    const float lse_s = r.Ms + __logf(r.Zs);
    const float lse_sT = T1 ? lse_s : r.Ms * invT + __logf(r.ZsT);
    const float lse_tT = r.Mt * invT + __logf(r.Zt);
    const long y = labels[row];
    float ce = 0.f, kl = 0.f;
    if (y != ignore && y >= 0 && y < V) {
      float xy = Elem<T>::load(x + y);
      if (bias_s != nullptr) xy += bias_s[y];
      ce = lse_s - (1.f - eps) * xy - smooth_term(eps, r.SX, V);
      kl = r.A / r.Zt * invT - lse_tT + lse_sT;
    }
    ce_out[row] = ce;
    kl_out[row] = kl;
    stats[row * 3 + 0] = lse_s;
    stats[row * 3 + 1] = lse_sT;
    stats[row * 3 + 2] = lse_tT;
  }
}

// one column's gradient; kT = w_kl * T
template <bool T1>
DLLM_DEVICE float kd_grad(float s, float t, float gce, float kT, float lse_s, float lse_sT, float lse_tT, float invT,
                          float off, float hit) {
  const float sm = __expf(s - lse_s);
  const float q = T1 ? sm : __expf(s * invT - lse_sT);
  const float p = __expf(t * invT - lse_tT);
  return gce * (sm - off - hit) + kT * (q - p);
}

template <typename T, bool T1>
__global__ __launch_bounds__(256) void kd_bwd_kernel(const float* __restrict__ w_ce, const float* __restrict__ w_kl,
                                                     const T* __restrict__ student, const T* __restrict__ teacher,
                                                     const int64_t* __restrict__ labels,
                                                     const float* __restrict__ stats,
                                                     const float* __restrict__ bias_s,
                                                     const float* __restrict__ bias_t, T* __restrict__ dlogits, int V,
                                                     float eps, long ignore, float invT, float Tmp) {
  constexpr int E = Vec16<T>::N;
  const long row = blockIdx.x;
  const T* x = student + row * (long)V;
  const T* tt = teacher + row * (long)V;
  T* dx = dlogits + row * (long)V;
  const long y = labels[row];
  const bool valid = (y != ignore && y >= 0 && y < V);
  const float gce = valid ? w_ce[0] : 0.f;
  const float kT = valid ? w_kl[0] * Tmp : 0.f;
  const float lse_s = stats[row * 3 + 0], lse_sT = stats[row * 3 + 1], lse_tT = stats[row * 3 + 2];
  const float off = eps / (float)V;
  const float hit = 1.f - eps;
  auto one = [&](int c) {
    const float s = Elem<T>::load(x + c) + (bias_s != nullptr ? bias_s[c] : 0.f);
    const float t = Elem<T>::load(tt + c) + (bias_t != nullptr ? bias_t[c] : 0.f);
    Elem<T>::store(dx + c, kd_grad<T1>(s, t, gce, kT, lse_s, lse_sT, lse_tT, invT, off, c == y ? hit : 0.f));
  };
  const int head = row_head(dx, V);  // whole-vector stores: the output row sets the boundaries
  const int body_end = head + ((V - head) / E) * E;
  if ((int)threadIdx.x < head) one(threadIdx.x);
  for (int c = head + (int)threadIdx.x * E; c < body_end; c += 256 * E) {
    float s[E], t[E];
    Vec16<T>::load_e(x + c, s);
    Vec16<T>::load_e(tt + c, t);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const float bs = bias_s != nullptr ? bias_s[c + k] : 0.f;
      const float bt = bias_t != nullptr ? bias_t[c + k] : 0.f;
      s[k] = kd_grad<T1>(s[k] + bs, t[k] + bt, gce, kT, lse_s, lse_sT, lse_tT, invT, off, (c + k) == y ? hit : 0.f);
    }
    Vec16<T>::store(dx + c, s);
  }
  for (int c = body_end + (int)threadIdx.x; c < V; c += 256) one(c);
}

// ---- vocab-chunked form (ops/distill.py lm_head_distill_loss): both logits exist one [N, Vc] chunk at a time.
// Per row running state st[row] = {m_s, sum exp(s-m_s), sum s, s_label, sum exp((s-m_s)/T), m_t, sum exp((t-m_t)/T), A}
// merged over chunks; the last chunk writes ce_row, kl_row and stats.  Conventions of ce_chunk_fwd: chunk columns are
// global vocab ids c0 .. c0 + Vc - 1, eps / V uses the full vocab size, the first `skip` columns were covered by the
// previous chunk (ragged vocab tail).
template <bool T1>
__global__ __launch_bounds__(256) void kd_chunk_fwd_kernel(const uint16_t* __restrict__ student, long ld_s,
                                                           const uint16_t* __restrict__ teacher, long ld_t,
                                                           const int64_t* __restrict__ labels,
                                                           const float* __restrict__ bias_s,
                                                           const float* __restrict__ bias_t, float* __restrict__ st,
                                                           float* __restrict__ ce_out, float* __restrict__ kl_out,
                                                           float* __restrict__ stats, int Vc, int c0, int V, float eps,
                                                           long ignore, float invT, int first, int last, int skip) {
  __shared__ float red[4];
  const long row = blockIdx.x;
  const uint16_t* x = student + row * ld_s;
  const uint16_t* tt = teacher + row * ld_t;
  KdAcc<T1> acc;
  for (int c = threadIdx.x * 4; c < Vc; c += 256 * 4) {  // Vc % 4 == 0
    f32x4 sv = Elem<uint16_t>::load4(x + c);
    f32x4 tv = Elem<uint16_t>::load4(tt + c);
    if (bias_s != nullptr) sv += bias4(bias_s, c0 + c);
    if (bias_t != nullptr) tv += bias4(bias_t, c0 + c);
    if (c + 4 <= skip) continue;
    if (c < skip) {  // the group straddling the skip boundary: column by column
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (c + k >= skip) {
          const float s1[1] = {sv[k]}, t1[1] = {tv[k]};
          acc.template add<1>(s1, t1, invT);
        }
      }
    } else {
      const float s4[4] = {sv.x, sv.y, sv.z, sv.w}, t4[4] = {tv.x, tv.y, tv.z, tv.w};
      acc.template add<4>(s4, t4, invT);
    }
  }
  const KdRow r = kd_block_merge<T1>(acc, invT, red);
  if (threadIdx.x == 0) {
    const long y = labels[row];
    float* cur = st + row * 8;
    float ms = -INFINITY, zs = 0.f, sx = 0.f, sy = 0.f, zsT = 0.f, mt = -INFINITY, zt = 0.f, A = 0.f;
    if (!first) {
      ms = cur[0], zs = cur[1], sx = cur[2], sy = cur[3], zsT = cur[4], mt = cur[5], zt = cur[6], A = cur[7];
    }
    const float ns = fmaxf(ms, r.Ms);
    const float fo = ms == -INFINITY ? 0.f : __expf(ms - ns), fn = r.Ms == -INFINITY ? 0.f : __expf(r.Ms - ns);
    zs = zs * fo + r.Zs * fn;
    if constexpr (!T1) {
      const float foT = ms == -INFINITY ? 0.f : __expf((ms - ns) * invT);
      const float fnT = r.Ms == -INFINITY ? 0.f : __expf((r.Ms - ns) * invT);
      zsT = zsT * foT + r.ZsT * fnT;
    }
    ms = ns;
    sx += r.SX;
    const float nt = fmaxf(mt, r.Mt);
    const float go = mt == -INFINITY ? 0.f : __expf((mt - nt) * invT);
    const float gn = r.Mt == -INFINITY ? 0.f : __expf((r.Mt - nt) * invT);
    zt = zt * go + r.Zt * gn;
    A = kd_rescale(A, go) + kd_rescale(r.A, gn);
    mt = nt;
    if (y >= c0 + skip && y < c0 + Vc)
      sy = Elem<uint16_t>::load(x + (y - c0)) + (bias_s != nullptr ? bias_s[y] : 0.f);
    cur[0] = ms, cur[1] = zs, cur[2] = sx, cur[3] = sy, cur[4] = zsT, cur[5] = mt, cur[6] = zt, cur[7] = A;
    if (last) {
      const float lse_s = ms + __logf(zs);
      const float lse_sT = T1 ? lse_s : ms * invT + __logf(zsT);
      const float lse_tT = mt * invT + __logf(zt);
      const bool valid = y != ignore && y >= 0 && y < V;
      ce_out[row] = valid ? lse_s - (1.f - eps) * sy - smooth_term(eps, sx, V) : 0.f;
      kl_out[row] = valid ? A / zt * invT - lse_tT + lse_sT : 0.f;
      stats[row * 3 + 0] = lse_s;
      stats[row * 3 + 1] = lse_sT;
      stats[row * 3 + 2] = lse_tT;
    }
  }
}

// the student chunk's gradient, in place; a skipped column's gradient is 0
template <bool T1>
__global__ __launch_bounds__(256) void kd_chunk_bwd_kernel(const float* __restrict__ w_ce,
                                                           const float* __restrict__ w_kl, uint16_t* __restrict__ x_io,
                                                           long ld_s, const uint16_t* __restrict__ teacher, long ld_t,
                                                           const int64_t* __restrict__ labels,
                                                           const float* __restrict__ stats,
                                                           const float* __restrict__ bias_s,
                                                           const float* __restrict__ bias_t, int Vc, int c0, int V,
                                                           float eps, long ignore, float invT, float Tmp, int skip) {
  const long row = blockIdx.x;
  uint16_t* x = x_io + row * ld_s;
  const uint16_t* tt = teacher + row * ld_t;
  const long y = labels[row];
  const bool valid = (y != ignore && y >= 0 && y < V);
  const float gce = valid ? w_ce[0] : 0.f;
  const float kT = valid ? w_kl[0] * Tmp : 0.f;
  const float lse_s = stats[row * 3 + 0], lse_sT = stats[row * 3 + 1], lse_tT = stats[row * 3 + 2];
  const float off = eps / (float)V;
  const float hit = 1.f - eps;
  const long yl = y - c0;
  for (int c = threadIdx.x * 4; c < Vc; c += 256 * 4) {
    f32x4 sv = Elem<uint16_t>::load4(x + c);
    f32x4 tv = Elem<uint16_t>::load4(tt + c);
    if (bias_s != nullptr) sv += bias4(bias_s, c0 + c);
    if (bias_t != nullptr) tv += bias4(bias_t, c0 + c);
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      r[k] = c + k < skip ? 0.f
                          : kd_grad<T1>(sv[k], tv[k], gce, kT, lse_s, lse_sT, lse_tT, invT, off,
                                        (c + k) == yl ? hit : 0.f);
    Elem<uint16_t>::store4(x + c, r);
  }
}

}  // namespace

extern "C" int dllm_kd_fwd(const void* student, const void* teacher, const int64_t* labels, const float* bias_s,
                           const float* bias_t, float* ce, float* kl, float* stats, long N, int V, float eps,
                           long ignore, float T, int is_bf16, hipStream_t st) {
  if (N <= 0 || V <= 0 || !(T > 0.f)) return -2;
  dim3 g(N), b(256);
  const float invT = 1.f / T;
#define KD_FWD(TY, T1)                                                                                              \
  hipLaunchKernelGGL((kd_fwd_kernel<TY, T1>), g, b, 0, st, (const TY*)student, (const TY*)teacher, labels, bias_s, \
                     bias_t, ce, kl, stats, V, eps, ignore, invT)
  if (is_bf16) {
    if (T == 1.f) KD_FWD(uint16_t, true); else KD_FWD(uint16_t, false);
  } else {
    if (T == 1.f) KD_FWD(float, true); else KD_FWD(float, false);
  }
#undef KD_FWD
  DLLM_CHECK_LAUNCH();
  return 0;
}

extern "C" int dllm_kd_bwd(const float* w_ce, const float* w_kl, const void* student, const void* teacher,
                           const int64_t* labels, const float* stats, const float* bias_s, const float* bias_t,
                           void* dlogits, long N, int V, float eps, long ignore, float T, int is_bf16, hipStream_t st) {
  if (N <= 0 || V <= 0 || !(T > 0.f)) return -2;
  dim3 g(N), b(256);
  const float invT = 1.f / T;
#define KD_BWD(TY, T1)                                                                                           \
  hipLaunchKernelGGL((kd_bwd_kernel<TY, T1>), g, b, 0, st, w_ce, w_kl, (const TY*)student, (const TY*)teacher, \
                     labels, stats, bias_s, bias_t, (TY*)dlogits, V, eps, ignore, invT, T)
  if (is_bf16) {
    if (T == 1.f) KD_BWD(uint16_t, true); else KD_BWD(uint16_t, false);
  } else {
    if (T == 1.f) KD_BWD(float, true); else KD_BWD(float, false);
  }
#undef KD_BWD
  DLLM_CHECK_LAUNCH();
  return 0;
}

extern "C" int dllm_kd_chunk_fwd(const void* student, long ld_s, const void* teacher, long ld_t, const int64_t* labels,
                                 const float* bias_s, const float* bias_t, float* state, float* ce, float* kl,
                                 float* stats, long N, int Vc, int c0, int V, float eps, long ignore, float T,
                                 int first, int last, int skip, hipStream_t st) {
  if (Vc % 4 || ld_s % 4 || ld_t % 4 || N <= 0 || skip < 0 || skip >= Vc || !(T > 0.f)) return -2;
  const float invT = 1.f / T;
  if (T == 1.f)
    hipLaunchKernelGGL(kd_chunk_fwd_kernel<true>, dim3(N), dim3(256), 0, st, (const uint16_t*)student, ld_s,
                       (const uint16_t*)teacher, ld_t, labels, bias_s, bias_t, state, ce, kl, stats, Vc, c0, V, eps,
                       ignore, invT, first, last, skip);
  else
    hipLaunchKernelGGL(kd_chunk_fwd_kernel<false>, dim3(N), dim3(256), 0, st, (const uint16_t*)student, ld_s,
                       (const uint16_t*)teacher, ld_t, labels, bias_s, bias_t, state, ce, kl, stats, Vc, c0, V, eps,
                       ignore, invT, first, last, skip);
  DLLM_CHECK_LAUNCH();
  return 0;
}

extern "C" int dllm_kd_chunk_bwd(const float* w_ce, const float* w_kl, void* student, long ld_s, const void* teacher,
                                 long ld_t, const int64_t* labels, const float* stats, const float* bias_s,
                                 const float* bias_t, long N, int Vc, int c0, int V, float eps, long ignore, float T,
                                 int skip, hipStream_t st) {
  if (Vc % 4 || ld_s % 4 || ld_t % 4 || N <= 0 || skip < 0 || skip >= Vc || !(T > 0.f)) return -2;
  const float invT = 1.f / T;
  if (T == 1.f)
    hipLaunchKernelGGL(kd_chunk_bwd_kernel<true>, dim3(N), dim3(256), 0, st, w_ce, w_kl, (uint16_t*)student, ld_s,
                       (const uint16_t*)teacher, ld_t, labels, stats, bias_s, bias_t, Vc, c0, V, eps, ignore, invT, T,
                       skip);
  else
    hipLaunchKernelGGL(kd_chunk_bwd_kernel<false>, dim3(N), dim3(256), 0, st, w_ce, w_kl, (uint16_t*)student, ld_s,
                       (const uint16_t*)teacher, ld_t, labels, stats, bias_s, bias_t, Vc, c0, V, eps, ignore, invT, T,
                       skip);
  DLLM_CHECK_LAUNCH();
  return 0;
}
