// Fused preference-optimisation (DPO / IPO / hinge) loss on a policy's and a frozen reference's LM-head logits, for
// gfx950 (ops/preference.py).  N = 2 P T logit rows: sequence s owns rows [s T, (s+1) T), pair i is the sequences
// (2i, 2i+1) = (chosen, rejected).  Per row with logits x (+ bias b) and label y (valid iff != ignore and in [0, V)):
//   lp_r = (x_y + b_y) - lse(x + b)   (0 on an invalid row; lse is written for every row)
// fwd:   one 256-thread block per row, ONE pass that reads the policy's and the reference's row once and keeps two
//        online softmaxes; writes lp_pi, lp_ref, lse_pi (fp32).  The reference may be absent (policy alone).
// pairs: ONE block over the 2P sequences: L_s = sum_r lp_r in ascending order in fp32, n_s = max(1, #valid rows),
//        h_i = beta [(L^pi_c - L^pi_r) - (L^ref_c - L^ref_r)], the pair loss l_i, the step's loss sum_i l_i / P_step,
//        the six logged statistics and the row coefficients c_r = -G dloss/dL_s (0 on an invalid row).  G and
//        1 / P_step are device scalars (no host sync).  The pair math runs in fp64 on the fp32 sums (a few hundred
//        operations per step), every sum has a fixed order: reruns are bit-identical.
// bwd:   dx_v = c_r (exp(x_v + b_v - lse_r) - [v == y_r]) in the logits dtype, optionally in place over the policy
//        logits; a row with c_r == 0 is written as exact zeros (the buffer held logits).
// The reference gets no gradient.  No atomics.
#include "common.h"
#include "row_walk.h"

using namespace dllm;

namespace {

// Per-thread running state of one online softmax.
struct PrefAcc {
  float m = -INFINITY, z = 0.f;

  // E columns at once: ONE rescale per group
  template <int E>
  DLLM_DEVICE void add(const float (&v)[E]) {
    float l = v[0];
#pragma unroll
    for (int k = 1; k < E; ++k) l = fmaxf(l, v[k]);
    const float n = fmaxf(m, l);
    if (n != -INFINITY) {
      float e = 0.f;
#pragma unroll
      for (int k = 0; k < E; ++k) e += __expf(v[k] - n);
      z = (m == -INFINITY ? 0.f : z * __expf(m - n)) + e;
      m = n;
    }
  }
};

// Block-wide merge: every thread returns the row's {max, sum exp(x - max)}.
struct PrefRow {
  float M, Z;
};

DLLM_DEVICE PrefRow pref_block_merge(const PrefAcc& a, float* red) {
  PrefRow r;
  r.M = block_max<256>(a.m, red);
  r.Z = block_sum<256>(a.m == -INFINITY ? 0.f : a.z * __expf(a.m - r.M), red);
  return r;
}

// Rows are walked as in csrc/kd.hip: the boundaries come from the policy's row, the reference's 16-B groups are read
// through element-aligned vector types (its row may sit at another 16-B phase).
template <typename T, bool REF>
__global__ __launch_bounds__(256) void pref_fwd_kernel(const T* __restrict__ policy, const T* __restrict__ ref,
                                                       const int64_t* __restrict__ labels,
                                                       const float* __restrict__ bias_p,
                                                       const float* __restrict__ bias_r, float* __restrict__ lp_pi,
                                                       float* __restrict__ lp_ref, float* __restrict__ lse_pi, int V,
                                                       long ignore) {
  __shared__ float red[4];
  constexpr int E = Vec16<T>::N;
  const long row = blockIdx.x;
  const T* x = policy + row * (long)V;
  const T* rr = REF ? ref + row * (long)V : nullptr;
  PrefAcc ap, ar;
  auto add1 = [&](int c) {
    const float p[1] = {Elem<T>::load(x + c) + (bias_p != nullptr ? bias_p[c] : 0.f)};
    ap.template add<1>(p);
    if constexpr (REF) {
      const float r[1] = {Elem<T>::load(rr + c) + (bias_r != nullptr ? bias_r[c] : 0.f)};
      ar.template add<1>(r);
    }
  };
  const int head = row_head(x, V);
  const int body_end = head + ((V - head) / E) * E;
  if ((int)threadIdx.x < head) add1(threadIdx.x);
  for (int c = head + (int)threadIdx.x * E; c < body_end; c += 256 * E) {
    float p[E];
    Vec16<T>::load_e(x + c, p);
    if (bias_p != nullptr) {
#pragma unroll
      for (int k = 0; k < E; ++k) p[k] += bias_p[c + k];
    }
    ap.template add<E>(p);
    if constexpr (REF) {
      float r[E];
      Vec16<T>::load_e(rr + c, r);
      if (bias_r != nullptr) {
#pragma unroll
        for (int k = 0; k < E; ++k) r[k] += bias_r[c + k];
      }
      ar.template add<E>(r);
    }
  }
  for (int c = body_end + (int)threadIdx.x; c < V; c += 256) add1(c);
  const PrefRow rp = pref_block_merge(ap, red);
  PrefRow rf = {0.f, 1.f};
  if constexpr (REF) rf = pref_block_merge(ar, red);
  if (threadIdx.x == 0) {
    const float lse_p = rp.M + __logf(rp.Z);
    const long y = labels[row];
    float a = 0.f, b = 0.f;
    if (y != ignore && y >= 0 && y < V) {
      a = Elem<T>::load(x + y) + (bias_p != nullptr ? bias_p[y] : 0.f) - lse_p;
      if constexpr (REF) b = Elem<T>::load(rr + y) + (bias_r != nullptr ? bias_r[y] : 0.f) - (rf.M + __logf(rf.Z));
    }
    lp_pi[row] = a;
    lp_ref[row] = b;
    lse_pi[row] = lse_p;
  }
}

// log sigmoid(h) = -softplus(-h), stable for any h
DLLM_DEVICE double log_sigmoid(double h) { return fmin(h, 0.0) - log1p(exp(-fabs(h))); }
DLLM_DEVICE double sigmoid(double h) {
  const double e = exp(-fabs(h));
  return h >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

// pair_out[i * PREF_PAIR_COLS + k]
enum { PP_LOSS = 0, PP_H, PP_RW_C, PP_RW_R, PP_LP_C, PP_LP_R, PP_N_C, PP_N_R, PREF_PAIR_COLS };
// out[k]: the step's loss and the six statistics (means over the call's pairs)
enum { PO_LOSS = 0, PO_RW_C, PO_RW_R, PO_MARGIN, PO_ACC, PO_LP_C, PO_LP_R, PREF_OUT_COLS };

// ONE block of 1024 threads.  seq_sum [2P, 3] = {L^pi_s, L^ref_s, n_s} is scratch the block fills first.
constexpr int PREF_PAIRS_THREADS = 1024;
__global__ __launch_bounds__(PREF_PAIRS_THREADS) void pref_pairs_kernel(const float* __restrict__ lp_pi,
                                                         const float* __restrict__ lp_ref,
                                                         const int64_t* __restrict__ labels,
                                                         const float* __restrict__ G,
                                                         const float* __restrict__ inv_pairs,
                                                         float* seq_sum, float* pair_out,
                                                         float* __restrict__ out, float* __restrict__ coef, long P,
                                                         int T, int V, long ignore, double beta, int kind, double eps,
                                                         double sft_alpha) {
  const long S = 2 * P;
  // (1) ordered per-sequence sums: unit u = 2 s + model, one thread each.  Rows are loaded eight at a time (independent
  // loads in flight) and added in ascending order.
  for (long u = threadIdx.x; u < 2 * S; u += PREF_PAIRS_THREADS) {
    const long s = u >> 1;
    const float* lp = ((u & 1) ? lp_ref : lp_pi) + s * T;
    const int64_t* lab = labels + s * T;
    float L = 0.f;
    int n = 0;
    for (int t0 = 0; t0 < T; t0 += 8) {
      float v[8];
      bool ok[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int t = min(t0 + k, T - 1);
        const long y = lab[t];
        ok[k] = t0 + k < T && y != ignore && y >= 0 && y < V;
        v[k] = lp[t];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (ok[k]) {
          L += v[k];
          ++n;
        }
      }
    }
    seq_sum[s * 3 + (u & 1)] = L;
    if (!(u & 1)) seq_sum[s * 3 + 2] = (float)max(n, 1);
  }
  __syncthreads();
  // (2) per pair: h, loss, rewards, and the two sequences' dloss/dL (left in seq_sum[s * 3 + 1], no longer needed)
  const double g = G != nullptr ? (double)G[0] : 1.0;
  const double ip = (double)inv_pairs[0];
  for (long i = threadIdx.x; i < P; i += PREF_PAIRS_THREADS) {
    const long c = 2 * i, r = 2 * i + 1;
    const double Lc = seq_sum[c * 3], Lr = seq_sum[r * 3], Rc = seq_sum[c * 3 + 1], Rr = seq_sum[r * 3 + 1];
    const double nc = seq_sum[c * 3 + 2], nr = seq_sum[r * 3 + 2];
    const double b = beta;
    const double h = b * ((Lc - Lr) - (Rc - Rr));
    double l, dc, dr;  // loss, dl/dL^pi_c, dl/dL^pi_r
    if (kind == 0) {   // sigmoid
      l = -(1.0 - eps) * log_sigmoid(h) - eps * log_sigmoid(-h);
      const double dh = -(1.0 - eps) * sigmoid(-h) + eps * sigmoid(h);
      dc = dh * b, dr = -dh * b;
    } else if (kind == 1) {  // hinge
      l = fmax(0.0, 1.0 - h);
      const double dh = h < 1.0 ? -1.0 : 0.0;
      dc = dh * b, dr = -dh * b;
    } else {  // ipo: length-averaged log-ratios
      const double hb = (Lc / nc - Lr / nr) - (Rc / nc - Rr / nr);
      const double d = hb - 1.0 / (2.0 * b);
      l = d * d;
      dc = 2.0 * d / nc, dr = -2.0 * d / nr;
    }
    l += sft_alpha * (-Lc / nc);
    dc += -sft_alpha / nc;
    float* po = pair_out + i * PREF_PAIR_COLS;
    po[PP_LOSS] = (float)l;
    po[PP_H] = (float)h;
    po[PP_RW_C] = (float)(b * (Lc - Rc));
    po[PP_RW_R] = (float)(b * (Lr - Rr));
    po[PP_LP_C] = (float)Lc;
    po[PP_LP_R] = (float)Lr;
    po[PP_N_C] = (float)nc;
    po[PP_N_R] = (float)nr;
    seq_sum[c * 3 + 1] = (float)(-g * ip * dc);
    seq_sum[r * 3 + 1] = (float)(-g * ip * dr);
  }
  __syncthreads();
  // (3) row coefficients
  for (long r = threadIdx.x; r < S * T; r += PREF_PAIRS_THREADS) {
    const long y = labels[r];
    coef[r] = (y != ignore && y >= 0 && y < V) ? seq_sum[(r / T) * 3 + 1] : 0.f;
  }
  // (4) the step's loss and statistics: thread k sums column k over the pairs, in ascending order (eight loads in flight)
  if (threadIdx.x < PREF_OUT_COLS) {
    const int k = threadIdx.x;
    double a = 0.0;
    for (long i0 = 0; i0 < P; i0 += 8) {
      float rc[8], rr[8], x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float* po = pair_out + min(i0 + j, P - 1) * PREF_PAIR_COLS;
        rc[j] = po[PP_RW_C];
        rr[j] = po[PP_RW_R];
        x[j] = k == PO_LOSS ? po[PP_LOSS] : k == PO_LP_C ? po[PP_LP_C] : po[PP_LP_R];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (i0 + j >= P) break;
        switch (k) {
          case PO_RW_C: a += rc[j]; break;
          case PO_RW_R: a += rr[j]; break;
          case PO_MARGIN: a += (double)rc[j] - (double)rr[j]; break;
          case PO_ACC: a += rc[j] > rr[j] ? 1.0 : 0.0; break;
          default: a += x[j]; break;  // PO_LOSS, PO_LP_C, PO_LP_R
        }
      }
    }
    out[k] = (float)(k == PO_LOSS ? a * ip : a / (double)P);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void pref_bwd_kernel(const float* __restrict__ coef, const T* __restrict__ policy,
                                                       const int64_t* __restrict__ labels,
                                                       const float* __restrict__ lse_pi,
                                                       const float* __restrict__ bias_p, T* __restrict__ dlogits,
                                                       int V) {
  constexpr int E = Vec16<T>::N;
  const long row = blockIdx.x;
  const T* x = policy + row * (long)V;
  T* dx = dlogits + row * (long)V;
  const float c = coef[row];  // 0 on an invalid row: y is only compared below
  const long y = labels[row];
  const float lse = lse_pi[row];
  const int head = row_head(dx, V);  // whole-vector stores: the output row sets the boundaries
  const int body_end = head + ((V - head) / E) * E;
  if (c == 0.f) {  // block-uniform: exact zeros, nothing read
    float z[E];
#pragma unroll
    for (int k = 0; k < E; ++k) z[k] = 0.f;
    if ((int)threadIdx.x < head) Elem<T>::store(dx + threadIdx.x, 0.f);
    for (int col = head + (int)threadIdx.x * E; col < body_end; col += 256 * E) Vec16<T>::store(dx + col, z);
    for (int col = body_end + (int)threadIdx.x; col < V; col += 256) Elem<T>::store(dx + col, 0.f);
    return;
  }
  auto one = [&](int col) {
    const float s = Elem<T>::load(x + col) + (bias_p != nullptr ? bias_p[col] : 0.f);
    Elem<T>::store(dx + col, c * (__expf(s - lse) - (col == y ? 1.f : 0.f)));
  };
  if ((int)threadIdx.x < head) one(threadIdx.x);
  for (int col = head + (int)threadIdx.x * E; col < body_end; col += 256 * E) {
    float s[E];
    Vec16<T>::load_e(x + col, s);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const float b = bias_p != nullptr ? bias_p[col + k] : 0.f;
      s[k] = c * (__expf(s[k] + b - lse) - ((col + k) == y ? 1.f : 0.f));
    }
    Vec16<T>::store(dx + col, s);
  }
  for (int col = body_end + (int)threadIdx.x; col < V; col += 256) one(col);
}

// ---- vocab-chunked form (ops/preference.py lm_head_preference_loss): both logits exist one [N, Vc] bf16 chunk at a
// time.  Per row running state st[row] = {m_pi, sum exp(x - m_pi), x_label, m_ref, sum exp(r - m_ref), r_label} merged
// over chunks; the last chunk writes lp_pi, lp_ref and lse_pi.  Conventions of ce_chunk_fwd / kd_chunk_fwd: chunk
// columns are global vocab ids c0 .. c0 + Vc - 1, the first `skip` columns were covered by the previous chunk.
__global__ __launch_bounds__(256) void pref_chunk_fwd_kernel(const uint16_t* __restrict__ policy, long ld_p,
                                                             const uint16_t* __restrict__ ref, long ld_r,
                                                             const int64_t* __restrict__ labels,
                                                             const float* __restrict__ bias_p,
                                                             const float* __restrict__ bias_r, float* __restrict__ st,
                                                             float* __restrict__ lp_pi, float* __restrict__ lp_ref,
                                                             float* __restrict__ lse_pi, int Vc, int c0, int V,
                                                             long ignore, int first, int last, int skip) {
  __shared__ float red[4];
  const long row = blockIdx.x;
  const uint16_t* x = policy + row * ld_p;
  const uint16_t* rr = ref + row * ld_r;
  PrefAcc ap, ar;
  for (int c = threadIdx.x * 4; c < Vc; c += 256 * 4) {  // Vc % 4 == 0
    if (c + 4 <= skip) continue;
    f32x4 pv = Elem<uint16_t>::load4(x + c);
    f32x4 rv = Elem<uint16_t>::load4(rr + c);
    if (bias_p != nullptr) pv += bias4(bias_p, c0 + c);
    if (bias_r != nullptr) rv += bias4(bias_r, c0 + c);
    if (c < skip) {  // the group straddling the skip boundary: column by column
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (c + k >= skip) {
          const float p1[1] = {pv[k]}, r1[1] = {rv[k]};
          ap.add<1>(p1);
          ar.add<1>(r1);
        }
      }
    } else {
      const float p4[4] = {pv.x, pv.y, pv.z, pv.w}, r4[4] = {rv.x, rv.y, rv.z, rv.w};
      ap.add<4>(p4);
      ar.add<4>(r4);
    }
  }
  const PrefRow rp = pref_block_merge(ap, red);
  const PrefRow rf = pref_block_merge(ar, red);
  if (threadIdx.x == 0) {
    const long y = labels[row];
    float* cur = st + row * 6;
    float mp = -INFINITY, zp = 0.f, xy = 0.f, mr = -INFINITY, zr = 0.f, ry = 0.f;
    if (!first) mp = cur[0], zp = cur[1], xy = cur[2], mr = cur[3], zr = cur[4], ry = cur[5];
    const float np = fmaxf(mp, rp.M);
    zp = (mp == -INFINITY ? 0.f : zp * __expf(mp - np)) + (rp.M == -INFINITY ? 0.f : rp.Z * __expf(rp.M - np));
    mp = np;
    const float nr = fmaxf(mr, rf.M);
    zr = (mr == -INFINITY ? 0.f : zr * __expf(mr - nr)) + (rf.M == -INFINITY ? 0.f : rf.Z * __expf(rf.M - nr));
    mr = nr;
    if (y >= c0 + skip && y < c0 + Vc) {
      xy = Elem<uint16_t>::load(x + (y - c0)) + (bias_p != nullptr ? bias_p[y] : 0.f);
      ry = Elem<uint16_t>::load(rr + (y - c0)) + (bias_r != nullptr ? bias_r[y] : 0.f);
    }
    cur[0] = mp, cur[1] = zp, cur[2] = xy, cur[3] = mr, cur[4] = zr, cur[5] = ry;
    if (last) {
      const float lse_p = mp + __logf(zp);
      const bool valid = y != ignore && y >= 0 && y < V;
      lp_pi[row] = valid ? xy - lse_p : 0.f;
      lp_ref[row] = valid ? ry - (mr + __logf(zr)) : 0.f;
      lse_pi[row] = lse_p;
    }
  }
}

// the policy chunk's gradient, in place; a skipped column's gradient is 0, a c_r == 0 row is exact zeros
__global__ __launch_bounds__(256) void pref_chunk_bwd_kernel(const float* __restrict__ coef, uint16_t* __restrict__ x_io,
                                                             long ld_p, const int64_t* __restrict__ labels,
                                                             const float* __restrict__ lse_pi,
                                                             const float* __restrict__ bias_p, int Vc, int c0,
                                                             int skip) {
  const long row = blockIdx.x;
  uint16_t* x = x_io + row * ld_p;
  const float cr = coef[row];
  const float lse = lse_pi[row];
  const long yl = labels[row] - c0;
  for (int c = threadIdx.x * 4; c < Vc; c += 256 * 4) {
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if (cr != 0.f) {  // block-uniform
      f32x4 pv = Elem<uint16_t>::load4(x + c);
      if (bias_p != nullptr) pv += bias4(bias_p, c0 + c);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        r[k] = c + k < skip ? 0.f : cr * (__expf(pv[k] - lse) - ((c + k) == yl ? 1.f : 0.f));
    }
    Elem<uint16_t>::store4(x + c, r);
  }
}

}  // namespace

extern "C" int dllm_pref_fwd(const void* policy, const void* ref, const int64_t* labels, const float* bias_p,
                             const float* bias_r, float* lp_pi, float* lp_ref, float* lse_pi, long N, int V,
                             long ignore, int is_bf16, hipStream_t st) {
  if (N <= 0 || V <= 0) return -2;
  dim3 g(N), b(256);
#define PREF_FWD(TY, REF)                                                                                        \
  hipLaunchKernelGGL((pref_fwd_kernel<TY, REF>), g, b, 0, st, (const TY*)policy, (const TY*)ref, labels, bias_p, \
                     bias_r, lp_pi, lp_ref, lse_pi, V, ignore)
  if (is_bf16) {
    if (ref != nullptr) PREF_FWD(uint16_t, true); else PREF_FWD(uint16_t, false);
  } else {
    if (ref != nullptr) PREF_FWD(float, true); else PREF_FWD(float, false);
  }
#undef PREF_FWD
  DLLM_CHECK_LAUNCH();
  return 0;
}

extern "C" int dllm_pref_pair_cols() { return PREF_PAIR_COLS; }
extern "C" int dllm_pref_out_cols() { return PREF_OUT_COLS; }

extern "C" int dllm_pref_pairs(const float* lp_pi, const float* lp_ref, const int64_t* labels, const float* G,
                               const float* inv_pairs, float* seq_sum, float* pair_out, float* out, float* coef,
                               long P, int T, int V, long ignore, double beta, int kind, double eps, double sft_alpha,
                               hipStream_t st) {
  if (P <= 0 || T <= 0 || V <= 0 || !(beta > 0.0) || kind < 0 || kind > 2 || !(eps >= 0.0 && eps < 0.5)) return -2;
  hipLaunchKernelGGL(pref_pairs_kernel, dim3(1), dim3(PREF_PAIRS_THREADS), 0, st, lp_pi, lp_ref, labels, G, inv_pairs, seq_sum,
                     pair_out, out, coef, P, T, V, ignore, beta, kind, eps, sft_alpha);
  DLLM_CHECK_LAUNCH();
  return 0;
}

extern "C" int dllm_pref_bwd(const float* coef, const void* policy, const int64_t* labels, const float* lse_pi,
                             const float* bias_p, void* dlogits, long N, int V, int is_bf16, hipStream_t st) {
  if (N <= 0 || V <= 0) return -2;
  dim3 g(N), b(256);
  if (is_bf16)
    hipLaunchKernelGGL(pref_bwd_kernel<uint16_t>, g, b, 0, st, coef, (const uint16_t*)policy, labels, lse_pi, bias_p,
                       (uint16_t*)dlogits, V);
  else
    hipLaunchKernelGGL(pref_bwd_kernel<float>, g, b, 0, st, coef, (const float*)policy, labels, lse_pi, bias_p,
                       (float*)dlogits, V);
  DLLM_CHECK_LAUNCH();
  return 0;
}

extern "C" int dllm_pref_chunk_fwd(const void* policy, long ld_p, const void* ref, long ld_r, const int64_t* labels,
                                   const float* bias_p, const float* bias_r, float* state, float* lp_pi, float* lp_ref,
                                   float* lse_pi, long N, int Vc, int c0, int V, long ignore, int first, int last,
                                   int skip, hipStream_t st) {
  if (Vc % 4 || ld_p % 4 || ld_r % 4 || N <= 0 || skip < 0 || skip >= Vc) return -2;
  hipLaunchKernelGGL(pref_chunk_fwd_kernel, dim3(N), dim3(256), 0, st, (const uint16_t*)policy, ld_p,
                     (const uint16_t*)ref, ld_r, labels, bias_p, bias_r, state, lp_pi, lp_ref, lse_pi, Vc, c0, V,
                     ignore, first, last, skip);
  DLLM_CHECK_LAUNCH();
  return 0;
}

extern "C" int dllm_pref_chunk_bwd(const float* coef, void* policy, long ld_p, const int64_t* labels,
                                   const float* lse_pi, const float* bias_p, long N, int Vc, int c0, int skip,
                                   hipStream_t st) {
  if (Vc % 4 || ld_p % 4 || N <= 0 || skip < 0 || skip >= Vc) return -2;
  hipLaunchKernelGGL(pref_chunk_bwd_kernel, dim3(N), dim3(256), 0, st, coef, (uint16_t*)policy, ld_p, labels, lse_pi,
                     bias_p, Vc, c0, skip);
  DLLM_CHECK_LAUNCH();
  return 0;
}
