// bf16 flash attention (forward + backward) for head dims 136 .. 256 with grouped K/V heads (grouped-query attention:
// T5Gemma 2b-2b / 9b-9b, Gemma 2): q, o, dout, dq are [B, Sq, H, D] and k, v, dk, dv [B, Sk, Hkv, D] with H % Hkv == 0;
// query head h reads K/V head h / G, G = H / Hkv (G = 1: plain multi-head attention at these head dims).  bf16 in, bf16
// out, fp32 accumulation on v_mfma_f32_16x16x32_bf16.  Semantics of csrc/attn_params.h (AttnWideParams): softmax scale,
// key-padding mask, causal mask with causal_off = Sk - Sq (Sq != Sk included: the decode steps), sliding window
// (Sq == Sk, not causal; blocks outside the band are never loaded), soft cap c tanh(scale s / c) before the log2(e)
// factor and every mask, LSE [B, H, Sq] in log2 units, and for a row without a visible key output 0, LSE +inf and no
// gradient.  No bias LUT, segments, global keys, block lists or dropout: the binding refuses each by name and
// ops/attention.py attention_grouped takes the composite for them.
//
// The real head dim D (D % 8 == 0) is a runtime field under ONE padded instantiation DP = 256: columns D .. 255 are
// staged as zeros and never stored (the convention of csrc/attn_hd.hip).  The MFMA layout trick, the LDS image and the
// transposed reads are csrc/attn_hd.hip's (attn_mfma16.h): S^T = K Q^T leaves two packed accumulator tiles as the B
// operand of the next product, so P and dS take no LDS round trip.
//
// What differs from csrc/attn_hd.hip is who shares a staged tile and where dK / dV are summed:
//
//   forward, dQ   grid (ceil(Sq / R), B * Hkv * G / gw), 256 threads.  A workgroup belongs to a K/V head: each 64-key K
//                 and V block is staged in LDS once (2 x 33 KB) and consumed by gw = 4, 2 or 1 query heads of the group
//                 at once (the largest of those that divides G; G / gw passes on the grid's y axis for any other G).
//                 The 4 waves split (query head) x (16-row slice): R = 64 / gw query rows per workgroup — 32 rows of
//                 both heads at G = 2, 64 rows at G = 1, 16 rows of four heads at G = 4.  So K/V traffic from HBM and
//                 through LDS staging is 1 / gw of what repeated K/V tensors cost.  Per wave: Q (dQ: and dO) as 8
//                 register fragments, online softmax in registers, O^T / dQ^T in 16 accumulator tiles (64 registers).
//   delta         sum_j P dP (= rowsum(dO o O) in exact arithmetic) by the dQ kernel's DELTA instantiation: the same walk
//                 without the dQ product, in fp32 from the unrounded probabilities (the kernel says why not from o).
//   dK / dV       grid (ceil(Sk / 64), B * Hkv): 4 waves x 16 keys, the wave's K and V fragments in registers.  It loops
//                 over the G query heads of the group and, within each, over the 64-row query blocks (from the causal
//                 diagonal on, or the band under a window), Q and dO staged in LDS; dK^T and dV^T of the K/V head
//                 accumulate in registers across the whole group (2 x 64 registers per lane) and are written once: no
//                 atomics, no [B, Sk, H, D] intermediate, no second reduction kernel.
//
// Every loop bound is uniform over the workgroup, so the barriers stay matched.
//
// Budget (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, profiles/attn_wide.txt): forward and dQ
// hold 64 accumulator registers and fit 256 registers, so they are bounded to 2 waves per SIMD — two workgroups per CU
// (2 x 67.7 KB of the 160 KB LDS), each hiding the other's staging, instead of the one workgroup with double-buffered
// images the design started from: same LDS, no second image to manage.  dK / dV needs the whole register file
// (128 accumulators + 64 operand registers): 1 wave per SIMD, one workgroup per CU.  No scratch anywhere.
// The cap is a template parameter (CAP): its per-score exp2, reciprocal and multiply-adds and their registers stay out
// of the uncapped kernels, as in csrc/attn_hd.hip; 2 x 4 instantiations in all.
#include "common.h"
#include "attn_params.h"
#include "attn_small.h"
#include "attn_mfma16.h"

using namespace dllm;

namespace {

constexpr int DP = 256, KS = DP / 32, DT = DP / 16;

// visibility of the lane's 16 keys of a block from the staged validity bytes: bit 4 t + i <-> key 16 t + 4 g + i
DLLM_DEVICE uint32_t valid_bits(const uint8_t* mk, int g) {
  uint32_t m = 0u;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(mk + 16 * t + 4 * g);
    m |= ((w & 1u) | ((w >> 7) & 2u) | ((w >> 14) & 4u) | ((w >> 21) & 8u)) << (4 * t);
  }
  return m;
}

// Where a wave of forward / dQ works: batch row b, K/V head hk, query head h, the workgroup's first row q0 and its row
// count R, the lane's row.
struct WideTile {
  int b, hk, h, q0, R, row, rowc;
  DLLM_DEVICE WideTile(const AttnWideParams& P, int w, int c) {
    const int spw = 4 / P.gw, npass = P.G / P.gw;  // 16-row slices per head; head passes on the y axis
    const int by = blockIdx.y, bk = by / npass;
    b = bk / P.Hkv;
    hk = bk % P.Hkv;
    h = hk * P.G + (by % npass) * P.gw + w / spw;
    R = BQ / P.gw;
    q0 = blockIdx.x * R;
    row = q0 + 16 * (w % spw) + c;
    rowc = min(row, P.Sq - 1);
  }
};

// the key blocks [kstart, kend) a workgroup at rows [q0, q0 + R) walks: up to the causal diagonal, within the band
DLLM_DEVICE void key_range(const AttnWideParams& P, int q0, int R, int& kstart, int& kend) {
  kstart = 0;
  kend = P.Sk;
  if (P.causal) kend = min(P.Sk, max(0, q0 + R + P.causal_off));
  band_range(P, q0, kstart, kend);  // the band of the 64 rows from q0: a superset of the R rows' (elements are masked)
}

// ================================================================================================ forward
template <bool CAP>
__global__ __launch_bounds__(NT, 2) void attn_wide_fwd_kernel(AttnWideParams P) {
  __shared__ __attribute__((aligned(16))) uint16_t Ks[Img<DP>::SIZE];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[Img<DP>::SIZE];
  __shared__ __attribute__((aligned(16))) uint8_t Mk[BKY];  // 1: key valid (in range, not padding)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
  const WideTile T(P, w, c);
  const int b = T.b, row = T.row;
  bf16x8v qf[KS];
  load_row_frags<DP>(P.q + (long)b * P.q_sb + (long)T.rowc * P.q_ss + (long)T.h * P.q_sh, g, P.D, qf);
  const float scale2 = P.scale * LOG2E;
  // soft cap: x = c log2(e) tanh(scale s / c), tanh from exp2(2 log2(e) z) (tanh_ex2)
  const float capz2 = CAP ? P.scale / P.softcap * (2.f * LOG2E) : 0.f;
  const float capc2 = CAP ? P.softcap * LOG2E : 0.f;
  float m = -INFINITY, l = 0.f;
  f32x4 acc[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const uint16_t* kb = P.k + (long)b * P.k_sb + (long)T.hk * P.k_sh;
  const uint16_t* vb = P.v + (long)b * P.v_sb + (long)T.hk * P.v_sh;
  int kstart, kend;
  key_range(P, T.q0, T.R, kstart, kend);
  for (int k0 = kstart; k0 < kend; k0 += BKY) {
    __syncthreads();  // the previous block's LDS reads are done
    stage<DP>(kb, P.k_ss, k0, P.Sk, P.D, Ks, tid);
    stage<DP>(vb, P.v_ss, k0, P.Sk, P.D, Vs, tid);
    if (tid < BKY) Mk[tid] = (uint8_t)key_ok(P, b, k0 + tid);
    __syncthreads();
    const uint32_t vis = valid_bits(Mk, g);
    f32x4 st[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) st[t] = mma(ld_row<DP>(Ks, 16 * t + c, ks, g), qf[ks], st[t]);
    }
    // st[t][i] = S[row][key = k0 + 16 t + 4 g + i]
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = k0 + 16 * t + 4 * g + i;
        float x;
        if constexpr (CAP) x = capc2 * tanh_ex2(st[t][i] * capz2);  // c tanh(scale s / c), in log2 units
        else x = st[t][i] * scale2;
        if (hidden(vis, t, i) || (P.causal && key > row + P.causal_off) || off_band(P, row, key)) x = -INFINITY;
        st[t][i] = x;
        mx = fmaxf(mx, x);
      }
    }
    mx = grp_max(mx);
    const float mn = fmaxf(m, mx);
    const float mu = mn == -INFINITY ? 0.f : mn;
    const float alpha = ex2(m - mu);
    float ls = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pr = ex2(st[t][i] - mu);
        ls += pr;
        st[t][i] = pr;
      }
    }
    ls = grp_sum(ls);
    l = l * alpha + ls;
    m = mn;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] *= alpha;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bf16x8v pb = pack8(st[2 * u], st[2 * u + 1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) acc[dt] = mma(ld_tr2<DP>(Vs, 32 * u, 16 * dt, c, g), pb, acc[dt]);
    }
  }
  // acc[dt][i] = O[row][d = 16 dt + 4 g + i] (unnormalised)
  if (row < P.Sq) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    uint16_t* op = P.o_out + (long)b * P.o_sb + (long)row * P.o_ss + (long)T.h * P.o_sh;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
      if (16 * dt + 4 * g < P.D) st4(op + 16 * dt + 4 * g, acc[dt] * inv);
    if (g == 0) P.lse[((long)b * P.H + T.h) * P.Sq + row] = l > 0.f ? m + __log2f(l) : INFINITY;
  }
}

// ================================================================================================ backward
// DELTA: the pass that writes delta[bh][row] = sum_j P dP and nothing else — the same walk, S^T and dP^T without the
// dQ product.  In exact arithmetic that is rowsum(dO o O), what the other families read from the stored output; here
// it is summed in fp32 from the unrounded probabilities, because the stored bf16 o carries a rounding (2^-9 of o) that
// dP - delta does not cancel: on a row whose softmax is one-hot (a causal row with a handful of keys under a cap) dS and
// dq are far smaller than that, and were noise (profiles/attn_wide.txt, "accuracy").
template <bool CAP, bool DELTA>
__global__ __launch_bounds__(NT, 2) void attn_wide_dq_kernel(AttnWideParams P) {
  __shared__ __attribute__((aligned(16))) uint16_t Ks[Img<DP>::SIZE];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[Img<DP>::SIZE];
  __shared__ __attribute__((aligned(16))) uint8_t Mk[BKY];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
  const WideTile T(P, w, c);
  const int b = T.b, row = T.row;
  const bool row_ok = row < P.Sq;
  bf16x8v qf[KS], dof[KS];
  load_row_frags<DP>(P.q + (long)b * P.q_sb + (long)T.rowc * P.q_ss + (long)T.h * P.q_sh, g, P.D, qf);
  load_row_frags<DP>(P.dout + (long)b * P.do_sb + (long)T.rowc * P.do_ss + (long)T.h * P.do_sh, g, P.D, dof);
  const long lrow = ((long)b * P.H + T.h) * P.Sq + row;
  const float lse = row_ok ? P.lse[lrow] : INFINITY;
  const float dlt = !DELTA && row_ok ? P.delta[lrow] : 0.f;
  float dsum = 0.f;  // DELTA: the lane's share of sum_j P dP
  const float scale2 = P.scale * LOG2E;
  const float capz2 = CAP ? P.scale / P.softcap * (2.f * LOG2E) : 0.f;
  const float capc2 = CAP ? P.softcap * LOG2E : 0.f;
  f32x4 acc[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const uint16_t* kb = P.k + (long)b * P.k_sb + (long)T.hk * P.k_sh;
  const uint16_t* vb = P.v + (long)b * P.v_sb + (long)T.hk * P.v_sh;
  int kstart, kend;
  key_range(P, T.q0, T.R, kstart, kend);
  for (int k0 = kstart; k0 < kend; k0 += BKY) {
    __syncthreads();
    stage<DP>(kb, P.k_ss, k0, P.Sk, P.D, Ks, tid);
    stage<DP>(vb, P.v_ss, k0, P.Sk, P.D, Vs, tid);
    if (tid < BKY) Mk[tid] = (uint8_t)key_ok(P, b, k0 + tid);
    __syncthreads();
    const uint32_t vis = valid_bits(Mk, g);
    f32x4 st[4], dpt[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      dpt[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        st[t] = mma(ld_row<DP>(Ks, 16 * t + c, ks, g), qf[ks], st[t]);
        dpt[t] = mma(ld_row<DP>(Vs, 16 * t + c, ks, g), dof[ks], dpt[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = k0 + 16 * t + 4 * g + i;
        float x, dtanh = 1.f;  // dtanh = 1 - tanh^2, the cap's derivative
        if constexpr (CAP) {
          const float th = tanh_ex2(st[t][i] * capz2);
          x = capc2 * th;
          dtanh = 1.f - th * th;
        } else {
          x = st[t][i] * scale2;
        }
        const bool msk = hidden(vis, t, i) || (P.causal && key > row + P.causal_off) || off_band(P, row, key);
        const float pr = msk ? 0.f : ex2(x - lse);  // 0 for rows >= Sq and rows without a key (lse = inf)
        if constexpr (DELTA) dsum += pr * dpt[t][i];
        else st[t][i] = CAP ? pr * (dpt[t][i] - dlt) * dtanh : pr * (dpt[t][i] - dlt);
      }
    }
    if constexpr (!DELTA) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bf16x8v sb = pack8(st[2 * u], st[2 * u + 1]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc[dt] = mma(ld_tr2<DP>(Ks, 32 * u, 16 * dt, c, g), sb, acc[dt]);
      }
    }
  }
  if constexpr (DELTA) {
    dsum = grp_sum(dsum);
    if (row_ok && g == 0) P.delta[lrow] = dsum;
    return;
  }
  // acc[dt][i] = dQ[row][d = 16 dt + 4 g + i] / scale
  if (row_ok) {
    uint16_t* dqp = P.dq + (long)b * P.dq_sb + (long)row * P.dq_ss + (long)T.h * P.dq_sh;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
      if (16 * dt + 4 * g < P.D) st4(dqp + 16 * dt + 4 * g, acc[dt] * P.scale);
  }
}

template <bool CAP>
__global__ __launch_bounds__(NT, 1) void attn_wide_dkdv_kernel(AttnWideParams P) {
  __shared__ __attribute__((aligned(16))) uint16_t Qs[Img<DP>::SIZE];
  __shared__ __attribute__((aligned(16))) uint16_t Os[Img<DP>::SIZE];  // dO
  __shared__ float Rl[BQ], Rd[BQ];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
  const int b = blockIdx.y / P.Hkv, hk = blockIdx.y % P.Hkv;
  const int k0 = blockIdx.x * BKY;
  const int key = k0 + 16 * w + c;
  const int keyc = min(key, P.Sk - 1);
  bf16x8v kf[KS], vf[KS];
  load_row_frags<DP>(P.k + (long)b * P.k_sb + (long)keyc * P.k_ss + (long)hk * P.k_sh, g, P.D, kf);
  load_row_frags<DP>(P.v + (long)b * P.v_sb + (long)keyc * P.v_ss + (long)hk * P.v_sh, g, P.D, vf);
  const float scale2 = P.scale * LOG2E;
  const float capz2 = CAP ? P.scale / P.softcap * (2.f * LOG2E) : 0.f;
  const float capc2 = CAP ? P.softcap * LOG2E : 0.f;
  const bool kok = key_ok(P, b, key);
  f32x4 dk[DT], dv[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) {
    dk[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    dv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  int qstart = 0, qend = P.Sq;
  if (P.causal) qstart = max(0, (k0 - P.causal_off) / BQ * BQ);
  band_range(P, k0, qstart, qend);
  for (int hg = 0; hg < P.G; ++hg) {  // the query heads this K/V head serves: one register accumulator for all
    const int h = hk * P.G + hg;
    const long bh = (long)b * P.H + h;
    const uint16_t* qb = P.q + (long)b * P.q_sb + (long)h * P.q_sh;
    const uint16_t* ob = P.dout + (long)b * P.do_sb + (long)h * P.do_sh;
    for (int q0 = qstart; q0 < qend; q0 += BQ) {
      __syncthreads();
      stage<DP>(qb, P.q_ss, q0, P.Sq, P.D, Qs, tid);
      stage<DP>(ob, P.do_ss, q0, P.Sq, P.D, Os, tid);
      if (tid < BQ) {
        const int r = q0 + tid;
        const bool ok = r < P.Sq;
        Rl[tid] = ok ? P.lse[bh * P.Sq + r] : INFINITY;
        Rd[tid] = ok ? P.delta[bh * P.Sq + r] : 0.f;
      }
      __syncthreads();
      f32x4 sc[4], dp[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          sc[t] = mma(ld_row<DP>(Qs, 16 * t + c, ks, g), kf[ks], sc[t]);
          dp[t] = mma(ld_row<DP>(Os, 16 * t + c, ks, g), vf[ks], dp[t]);
        }
      }
      // sc[t][i] = S[row = q0 + 16 t + 4 g + i][key]; pd = P, sc <- dS
      f32x4 pd[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int rl = 16 * t + 4 * g + i, row = q0 + rl;
          float x, dtanh = 1.f;
          if constexpr (CAP) {
            const float th = tanh_ex2(sc[t][i] * capz2);
            x = capc2 * th;
            dtanh = 1.f - th * th;
          } else {
            x = sc[t][i] * scale2;
          }
          const bool msk = !kok || (P.causal && key > row + P.causal_off) || off_band(P, row, key);
          const float pr = msk ? 0.f : ex2(x - Rl[rl]);
          pd[t][i] = pr;
          sc[t][i] = CAP ? pr * (dp[t][i] - Rd[rl]) * dtanh : pr * (dp[t][i] - Rd[rl]);
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bf16x8v pb = pack8(pd[2 * u], pd[2 * u + 1]);
        const bf16x8v sb = pack8(sc[2 * u], sc[2 * u + 1]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          dv[dt] = mma(ld_tr2<DP>(Os, 32 * u, 16 * dt, c, g), pb, dv[dt]);
          dk[dt] = mma(ld_tr2<DP>(Qs, 32 * u, 16 * dt, c, g), sb, dk[dt]);
        }
      }
    }
  }
  // dk[dt][i] = dK[key][d = 16 dt + 4 g + i] / scale, summed over the group's query heads
  if (key < P.Sk) {
    uint16_t* dkp = P.dk + (long)b * P.dk_sb + (long)key * P.dk_ss + (long)hk * P.dk_sh;
    uint16_t* dvp = P.dv + (long)b * P.dv_sb + (long)key * P.dv_ss + (long)hk * P.dv_sh;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      if (16 * dt + 4 * g < P.D) {
        st4(dkp + 16 * dt + 4 * g, dk[dt] * P.scale);
        st4(dvp + 16 * dt + 4 * g, dv[dt]);
      }
    }
  }
}

// the shapes and combinations the kernels serve (the binding checks each first, with a message); sets G and gw
int prepare(AttnWideParams& P) {
  if (P.D < 136 || P.D > 256 || P.D % 8) return -1;
  if (P.Hkv <= 0 || P.H % P.Hkv) return -2;
  if (P.window >= 0 && (P.causal || P.Sq != P.Sk)) return -3;
  if (P.softcap < 0.f) return -4;
  P.G = P.H / P.Hkv;
  P.gw = P.G % 4 == 0 ? 4 : P.G % 2 == 0 ? 2 : 1;
  return 0;
}

}  // namespace

extern "C" int dllm_attn_wide_fwd(AttnWideParams* pp, hipStream_t st) {
  AttnWideParams P = *pp;
  if (const int rc = prepare(P)) return rc;
  const int R = BQ / P.gw;
  dim3 grid((P.Sq + R - 1) / R, P.B * P.Hkv * (P.G / P.gw));
  if (P.softcap > 0.f) hipLaunchKernelGGL(attn_wide_fwd_kernel<true>, grid, dim3(NT), 0, st, P);
  else hipLaunchKernelGGL(attn_wide_fwd_kernel<false>, grid, dim3(NT), 0, st, P);
  DLLM_CHECK_LAUNCH();
  return 0;
}

extern "C" int dllm_attn_wide_bwd(AttnWideParams* pp, hipStream_t st) {
  AttnWideParams P = *pp;
  if (const int rc = prepare(P)) return rc;
  const int R = BQ / P.gw;
  dim3 gq((P.Sq + R - 1) / R, P.B * P.Hkv * (P.G / P.gw)), gk((P.Sk + BKY - 1) / BKY, P.B * P.Hkv);
  if (P.softcap > 0.f) {
    hipLaunchKernelGGL((attn_wide_dq_kernel<true, true>), gq, dim3(NT), 0, st, P);  // delta, read by the two below
    hipLaunchKernelGGL((attn_wide_dq_kernel<true, false>), gq, dim3(NT), 0, st, P);
    hipLaunchKernelGGL(attn_wide_dkdv_kernel<true>, gk, dim3(NT), 0, st, P);
  } else {
    hipLaunchKernelGGL((attn_wide_dq_kernel<false, true>), gq, dim3(NT), 0, st, P);
    hipLaunchKernelGGL((attn_wide_dq_kernel<false, false>), gq, dim3(NT), 0, st, P);
    hipLaunchKernelGGL(attn_wide_dkdv_kernel<false>, gk, dim3(NT), 0, st, P);
  }
  DLLM_CHECK_LAUNCH();
  return 0;
}
