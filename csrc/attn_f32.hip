// fp32 flash attention (forward + backward) on the gfx950 f32-input matrix cores (v_mfma_f32_16x16x4_f32: exact
// f32 products, one rounding per product, fp32 accumulation — the reference's own precision, ref/train-torchrun.py
// 115-128 trains in fp32).  Same feature set and semantics as the bf16 kernels of csrc/attn.hip / ops/attention.py:
// T5 relative-position bias LUT [H, Sq + Sk - 1] (+ its gradient), key-padding mask, causal mask, softmax scale and
// attention-probability dropout with the exact keep decisions of ops/rng.py attention_keep_mask.  O(S) memory:
// probabilities are never materialised (the fp32 composite it replaces stored [B, H, Sq, Sk] scores + masks).
// Sliding window (AttnParamsT::window >= 0; Sq == Sk, not causal): as in csrc/attn_hd.hip, the block walks cover only
// the blocks that intersect the band (attn_small.h band_range) and the element mask gains |key - row| > w (off_band).
// Segments (AttnParamsT::q_seg / k_seg, sequence packing): as in csrc/attn_hd.hip, blocks of other segments are skipped
// by their (min, max) id tables (seg_apart) and the element mask gains "same non-negative id" (seg_bits).
// Global keys (AttnParamsT::k_glob / k_gblk, only with a window): as in csrc/attn_hd.hip, forward and dQ walk the band
// merged with the listed blocks that hold a global key (BlockWalk), dK / dV every query block from a key block with
// one.
// Block lists (AttnParamsT::kl_ptr / kl_idx / ql_ptr / ql_idx): as in csrc/attn_hd.hip, forward and dQ follow the query
// block's list of key blocks and dK / dV the key block's list of query blocks, repeats included (list_range), in
// instantiations of their own (template parameter LISTS): the kernels of every other call are the code they were.
// Soft cap (AttnParamsT::softcap > 0): as in csrc/attn_hd.hip the score is c tanh(scale s / c) before every mask, and
// dQ and dK / dV scale dS by 1 - tanh^2, in instantiations of their own (template parameter CAP).  tanh is the device
// library's tanhf: the exp2 form of the bf16 family cancels near 0 (absolute error ~6e-8, times c = 50 a 3e-6 error
// on the score), tanhf is relatively accurate there.
//
// Layout trick (no transposes through LDS for P or dS): the 16x16x4 f32 MFMA's C/D map puts rows 4g .. 4g+3
// (g = lane >> 4) of column (lane & 15) in a lane's 4 registers, and its A/B maps take reduction index k = g from
// lane group g.  Computing S^T = K Q^T (keys on the MFMA's M side) leaves each lane with keys 16t + 4g + i of ONE query
// row; feeding register i as the k-step-i operand of the next product reduces over keys {16t + 4g + i : g} — any key
// order is a valid reduction order as long as the other operand is read in the same order (its LDS image is laid out
// for that read: one ds_read_b128 per 4 k-steps).
//
//   forward    grid (Sq/64, B*H), 4 waves x 16 query rows; per 64-key block: K (row-major) and V (transposed) staged in
//              LDS, S^T = K Q^T (64 MFMAs / wave), online softmax + dropout in registers, O^T += V^T P^T (64 MFMAs).
//   dQ         grid (Sq/64, B*H): S^T, dP^T = V dO^T, dS = P (dP_kept - delta), dQ^T += K^T dS^T; the bias gradient is
//              summed per diagonal of the block's dS tile in LDS and added to dlut once per block (fp32 atomics).
//   dK / dV    grid (Sk/64, B*H), 4 waves x 16 keys: S = Q K^T, dP = dO V^T, dV += P_kept^T dO, dK += dS^T Q.
#include "common.h"
#include "attn_params.h"
#include "attn_small.h"

using namespace dllm;

DLLM_SEED_STEP_TU(attn_f32)

namespace {

constexpr int D = 64;

DLLM_DEVICE f32x4 mma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// [64][64] fp32 image, row-major, 16-B chunks XOR-swizzled by (row & 15)
DLLM_DEVICE int rm_off(int r, int c4) { return r * 64 + ((c4 ^ (r & 15)) << 2); }
// [64 cols][64 rows] transposed image of a row-major tile X[r][col]: element (col, r) at col * 64 + chunk(r>>2) ^ (col&15)
DLLM_DEVICE int tr_off(int col, int r) { return col * 64 + ((((r >> 2) ^ (col & 15))) << 2) + (r & 3); }

// stage rows [r0, r0 + 64) of a [*, S, H, 64] view into LDS: row-major image `rm` and/or transposed image `tr`
// (rows >= S read as 0).  256 threads, 4 x 16-B chunks each.
template <bool RM, bool TR>
DLLM_DEVICE void stage(const float* base, long ss, int r0, int S, float* rm, float* tr, int tid) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int idx = tid + NT * j, r = idx >> 4, c4 = idx & 15;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r0 + r < S) v = *reinterpret_cast<const f32x4*>(base + (long)(r0 + r) * ss + 4 * c4);
    if constexpr (RM) *reinterpret_cast<f32x4*>(rm + rm_off(r, c4)) = v;
    if constexpr (TR) {
      tr[tr_off(4 * c4 + 0, r)] = v.x;
      tr[tr_off(4 * c4 + 1, r)] = v.y;
      tr[tr_off(4 * c4 + 2, r)] = v.z;
      tr[tr_off(4 * c4 + 3, r)] = v.w;
    }
  }
}

// 16 floats of row r, columns 16 g .. 16 g + 15, from a row-major image
DLLM_DEVICE void rd_row16(const float* rm, int r, int g, float (&out)[16]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(rm + rm_off(r, 4 * g + j));
    out[4 * j] = v.x;
    out[4 * j + 1] = v.y;
    out[4 * j + 2] = v.z;
    out[4 * j + 3] = v.w;
  }
}
// 4 consecutive rows r4 .. r4 + 3 (r4 % 4 == 0) of column col, from a transposed image
DLLM_DEVICE f32x4 rd_col4(const float* tr, int col, int r4) {
  return *reinterpret_cast<const f32x4*>(tr + col * 64 + ((((r4 >> 2) ^ (col & 15))) << 2));
}

// The second __launch_bounds__ argument of the three kernels is the waves per SIMD their register counts gave before
// the segment hooks (3, 2, 2): with it the unsegmented fp32 step measures as before, at fewer registers
// (profiles/packing_regression_gate.txt; without it 0.7 % slower).
// ================================================================================================ forward
template <bool DROP, bool LISTS = false, bool CAP = false>
__global__ __launch_bounds__(NT, 3) void attn_f32_fwd_kernel(AttnF32Params P) {
  __shared__ __attribute__((aligned(16))) float Ks[BKY * D];
  __shared__ __attribute__((aligned(16))) float Vt[D * BKY];
  __shared__ float Ls[2 * BKY];
  __shared__ __attribute__((aligned(16))) uint8_t Mk[BKY];  // 1: key valid (in range, not padding)
  __shared__ __attribute__((aligned(16))) int Sg[BKY];  // the keys' segment ids (with segments)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
  const int bh = blockIdx.y, b = bh / P.H, h = bh % P.H;
  const int q0 = blockIdx.x * BQ;
  const int row = q0 + 16 * w + c;
  const int rowc = min(row, P.Sq - 1);
  const int qsg = P.q_seg ? seg_at(P.q_seg, b, P.Sq, row) : 0;
  float qf[16];
  {
    const float* qp = P.q + (long)b * P.q_sb + (long)rowc * P.q_ss + (long)h * P.q_sh + 16 * g;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(qp + 4 * j);
      qf[4 * j] = v.x;
      qf[4 * j + 1] = v.y;
      qf[4 * j + 2] = v.z;
      qf[4 * j + 3] = v.w;
    }
  }
  const uint32_t rh = DROP ? mix32(eff_seed(P.seed), (uint32_t)((long)bh * P.Sq + rowc)) : 0u;
  const float dscale = DROP ? 1.f / (1.f - P.p_drop) : 1.f;
  const float capinv = CAP ? 1.f / P.softcap : 0.f;
  float m = -INFINITY, l = 0.f;
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* kb = P.k + (long)b * P.k_sb + (long)h * P.k_sh;
  const float* vb = P.v + (long)b * P.v_sb + (long)h * P.v_sh;
  int kend = P.Sk;
  if (P.causal) kend = min(P.Sk, max(0, q0 + BQ + P.causal_off));
  int kstart = 0;
  band_range(P, q0, kstart, kend);
  // one 64-key block of the walk.  Expanded twice on purpose, once per loop below, as in csrc/attn_hd.hip: calls
  // without global keys keep the affine loop they had
  auto block = [&](int k0) __attribute__((always_inline)) {
    __syncthreads();  // the previous block's LDS reads are done
    stage<true, false>(kb, P.k_ss, k0, P.Sk, Ks, nullptr, tid);
    stage<false, true>(vb, P.v_ss, k0, P.Sk, nullptr, Vt, tid);
    stage_bias(P, h, q0, k0, Ls, tid, 1.f);
    if (tid < BKY) {
      Mk[tid] = key_byte(P, b, k0 + tid);
      if (P.q_seg) Sg[tid] = seg_at(P.k_seg, b, P.Sk, k0 + tid);
    }
    __syncthreads();
    // key valid and of the row's segment (low half); key global (high half)
    const uint32_t vis = key_bits(P, Mk, Sg, qsg, g) | glob_bits(P, Mk, g);
    f32x4 st[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float kf[16];
      rd_row16(Ks, 16 * t + c, g, kf);
      st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 16; ++s) st[t] = mma(kf[s], qf[s], st[t]);
    }
    // st[t][i] = S[row][key = k0 + 16 t + 4 g + i]
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = k0 + 16 * t + 4 * g + i;
        float x = st[t][i] * P.scale;
        if constexpr (CAP) x = P.softcap * tanhf(x * capinv);
        if (P.lut) x += Ls[key - row - (k0 - q0 - 63)];
        if (hidden(vis, t, i) || (P.causal && key > row + P.causal_off) || off_band(P, row, key, vis, t, i))
          x = -INFINITY;
        st[t][i] = x;
        mx = fmaxf(mx, x);
      }
    }
    mx = grp_max(mx);
    const float mn = fmaxf(m, mx);
    const float mu = mn == -INFINITY ? 0.f : mn;
    const float alpha = __expf(m - mu);
    float ls = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t kb4 = DROP ? keep4(rh, k0 + 16 * t + 4 * g, P.thr) : 0xFu;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pr = __expf(st[t][i] - mu);
        ls += pr;
        st[t][i] = DROP ? (((kb4 >> i) & 1u) ? pr * dscale : 0.f) : pr;
      }
    }
    ls = grp_sum(ls);
    l = l * alpha + ls;
    m = mn;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) acc[dt] *= alpha;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const f32x4 va = rd_col4(Vt, 16 * dt + c, 16 * t + 4 * g);
        acc[dt] = mma(va.x, st[t][0], acc[dt]);
        acc[dt] = mma(va.y, st[t][1], acc[dt]);
        acc[dt] = mma(va.z, st[t][2], acc[dt]);
        acc[dt] = mma(va.w, st[t][3], acc[dt]);
      }
    }
  };
  if constexpr (LISTS) {
    // follow the query block's list of key blocks, repeats included (no causal, window, segments or global keys here)
    int li, le;
    list_range(P, P.kl_ptr, h, (P.Sq + 63) / 64, (int)blockIdx.x, li, le);
    for (; li < le; ++li) {
      const int k0 = list_block(P.kl_idx, li, (P.Sk + 63) / 64);
      if (k0 >= 0) block(k0);
    }
  } else if (P.k_glob == nullptr) {  // the walk as it was before the global keys: the band (or everything), segment skips
    for (int k0 = kstart; k0 < kend; k0 += BKY) {
      if (seg_apart(P, b, q0, k0)) continue;
      block(k0);
    }
  } else {  // the band merged with the listed blocks outside it (no segments with global keys)
    BlockWalk walk(P, b, kstart, kend);
    for (int k0 = walk.next(P, -BKY); k0 != BlockWalk::DONE; k0 = walk.next(P, k0)) block(k0);
  }
  if (row < P.Sq) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    float* op = P.o_out + (long)b * P.o_sb + (long)row * P.o_ss + (long)h * P.o_sh;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<f32x4*>(op + 16 * dt + 4 * g) = acc[dt] * inv;
    if (g == 0) P.lse[(long)bh * P.Sq + row] = l > 0.f ? m + __logf(l) : INFINITY;
  }
}

// ================================================================================================ backward
// delta[bh][row] = sum_d dO * O; one 16-lane group per row
__global__ __launch_bounds__(NT) void attn_f32_delta_kernel(AttnF32Params P) {
  const long rows = (long)P.B * P.H * P.Sq;
  const long r = (long)blockIdx.x * (NT / 16) + (threadIdx.x >> 4);
  const int j = threadIdx.x & 15;
  float s = 0.f;
  if (r < rows) {
    const int row = (int)(r % P.Sq);
    const long bh = r / P.Sq;
    const int b = (int)(bh / P.H), h = (int)(bh % P.H);
    const f32x4 o = *reinterpret_cast<const f32x4*>(P.o + (long)b * P.o_sb + (long)row * P.o_ss + (long)h * P.o_sh + 4 * j);
    const f32x4 d = *reinterpret_cast<const f32x4*>(P.dout + (long)b * P.do_sb + (long)row * P.do_ss +
                                                    (long)h * P.do_sh + 4 * j);
    s = o.x * d.x + o.y * d.y + o.z * d.z + o.w * d.w;
  }
#pragma unroll
  for (int mm = 8; mm >= 1; mm >>= 1) s += __shfl_xor(s, mm, 16);
  if (r < rows && j == 0) P.delta[r] = s;
}

template <bool DROP, bool LISTS = false, bool CAP = false>
__global__ __launch_bounds__(NT, 2) void attn_f32_dq_kernel(AttnF32Params P) {
  __shared__ __attribute__((aligned(16))) float Ks[BKY * D];
  __shared__ __attribute__((aligned(16))) float Kt[D * BKY];
  __shared__ __attribute__((aligned(16))) float Vs[BKY * D];
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
  float qf[16], dof[16];
  {
    const float* qp = P.q + (long)b * P.q_sb + (long)rowc * P.q_ss + (long)h * P.q_sh + 16 * g;
    const float* dp = P.dout + (long)b * P.do_sb + (long)rowc * P.do_ss + (long)h * P.do_sh + 16 * g;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(qp + 4 * j);
      const f32x4 d = *reinterpret_cast<const f32x4*>(dp + 4 * j);
      qf[4 * j] = v.x; qf[4 * j + 1] = v.y; qf[4 * j + 2] = v.z; qf[4 * j + 3] = v.w;
      dof[4 * j] = d.x; dof[4 * j + 1] = d.y; dof[4 * j + 2] = d.z; dof[4 * j + 3] = d.w;
    }
  }
  const float lse = row_ok ? P.lse[(long)bh * P.Sq + row] : INFINITY;
  const float dlt = row_ok ? P.delta[(long)bh * P.Sq + row] : 0.f;
  const uint32_t rh = DROP ? mix32(eff_seed(P.seed), (uint32_t)((long)bh * P.Sq + rowc)) : 0u;
  const float dscale = DROP ? 1.f / (1.f - P.p_drop) : 1.f;
  const float capinv = CAP ? 1.f / P.softcap : 0.f;
  const bool want_dlut = P.dlut != nullptr && P.lut != nullptr;
  // the row's dQ address, formed here as in csrc/attn_hd.hip: two vector registers through the walk instead of the
  // eight scalar ones of the base and strides, which the walk's own scalars would otherwise push out to spills
  float* dqp = P.dq + (long)b * P.dq_sb + (long)rowc * P.dq_ss + (long)h * P.dq_sh;
  asm volatile("" : "+v"(dqp));  // formed here, not sunk to the epilogue
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* kb = P.k + (long)b * P.k_sb + (long)h * P.k_sh;
  const float* vb = P.v + (long)b * P.v_sb + (long)h * P.v_sh;
  int kend = P.Sk;
  if (P.causal) kend = min(P.Sk, max(0, q0 + BQ + P.causal_off));
  int kstart = 0;
  band_range(P, q0, kstart, kend);
  // one 64-key block of the walk.  Expanded twice on purpose, once per loop below, as in csrc/attn_hd.hip: calls
  // without global keys keep the affine loop they had
  auto block = [&](int k0) __attribute__((always_inline)) {
    __syncthreads();
    stage<true, true>(kb, P.k_ss, k0, P.Sk, Ks, Kt, tid);
    stage<true, false>(vb, P.v_ss, k0, P.Sk, Vs, nullptr, tid);
    stage_bias(P, h, q0, k0, Ls, tid, 1.f);
    if (tid < BKY) {
      Mk[tid] = key_byte(P, b, k0 + tid);
      if (P.q_seg) Sg[tid] = seg_at(P.k_seg, b, P.Sk, k0 + tid);
    }
    __syncthreads();
    // key valid and of the row's segment (low half); key global (high half)
    const uint32_t vis = key_bits(P, Mk, Sg, qsg, g) | glob_bits(P, Mk, g);
    f32x4 st[4], dpt[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float kf[16], vf[16];
      rd_row16(Ks, 16 * t + c, g, kf);
      rd_row16(Vs, 16 * t + c, g, vf);
      st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      dpt[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        st[t] = mma(kf[s], qf[s], st[t]);
        dpt[t] = mma(vf[s], dof[s], dpt[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t kb4 = DROP ? keep4(rh, k0 + 16 * t + 4 * g, P.thr) : 0xFu;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = k0 + 16 * t + 4 * g + i;
        const int di = key - row - (k0 - q0 - 63);
        float x = st[t][i] * P.scale, dtanh = 1.f;  // dtanh = 1 - tanh^2, the cap's derivative
        if constexpr (CAP) {
          const float th = tanhf(x * capinv);
          x = P.softcap * th;
          dtanh = 1.f - th * th;
        }
        if (P.lut) x += Ls[di];
        const bool msk =
            hidden(vis, t, i) || (P.causal && key > row + P.causal_off) || off_band(P, row, key, vis, t, i);
        const float pr = msk ? 0.f : __expf(x - lse);
        const float dpk = DROP ? (((kb4 >> i) & 1u) ? dpt[t][i] * dscale : 0.f) : dpt[t][i];
        const float ds = CAP ? pr * (dpk - dlt) * dtanh : pr * (dpk - dlt);
        st[t][i] = ds;
        if (want_dlut) Ds[(16 * w + c) * (BKY + 1) + 16 * t + 4 * g + i] = ds;  // 0 for rows >= Sq (lse = inf)
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const f32x4 ka = rd_col4(Kt, 16 * dt + c, 16 * t + 4 * g);
        acc[dt] = mma(ka.x, st[t][0], acc[dt]);
        acc[dt] = mma(ka.y, st[t][1], acc[dt]);
        acc[dt] = mma(ka.z, st[t][2], acc[dt]);
        acc[dt] = mma(ka.w, st[t][3], acc[dt]);
      }
    }
    if (want_dlut) {
      __syncthreads();  // the block's dS tile is complete
      dlut_add_diagonals(P, h, q0, k0, Ds, tid);
    }
  };
  if constexpr (LISTS) {
    // follow the query block's list of key blocks, repeats included (no causal, window, segments or global keys here)
    int li, le;
    list_range(P, P.kl_ptr, h, (P.Sq + 63) / 64, (int)blockIdx.x, li, le);
    for (; li < le; ++li) {
      const int k0 = list_block(P.kl_idx, li, (P.Sk + 63) / 64);
      if (k0 >= 0) block(k0);
    }
  } else if (P.k_glob == nullptr) {  // the walk as it was before the global keys: the band (or everything), segment skips
    for (int k0 = kstart; k0 < kend; k0 += BKY) {
      if (seg_apart(P, b, q0, k0)) continue;
      block(k0);
    }
  } else {  // the band merged with the listed blocks outside it (no segments with global keys)
    BlockWalk walk(P, b, kstart, kend);
    for (int k0 = walk.next(P, -BKY); k0 != BlockWalk::DONE; k0 = walk.next(P, k0)) block(k0);
  }
  if (row_ok) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<f32x4*>(dqp + 16 * dt + 4 * g) = acc[dt] * P.scale;
  }
}

template <bool DROP, bool LISTS = false, bool CAP = false>
__global__ __launch_bounds__(NT, 2) void attn_f32_dkdv_kernel(AttnF32Params P) {
  __shared__ __attribute__((aligned(16))) float Qs[BQ * D];
  __shared__ __attribute__((aligned(16))) float Qt[D * BQ];
  __shared__ __attribute__((aligned(16))) float Os[BQ * D];  // dO, row-major
  __shared__ __attribute__((aligned(16))) float Ot[D * BQ];  // dO, transposed
  __shared__ float Ls[2 * BQ];
  __shared__ float Rl[BQ], Rd[BQ];
  __shared__ uint32_t Rh[BQ];
  __shared__ __attribute__((aligned(16))) int Rs[BQ];  // the rows' segment ids (with segments)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
  const int bh = blockIdx.y, b = bh / P.H, h = bh % P.H;
  const int k0 = blockIdx.x * BKY;
  const int key = k0 + 16 * w + c;
  const int keyc = min(key, P.Sk - 1);
  float kf[16], vf[16];
  {
    const float* kp = P.k + (long)b * P.k_sb + (long)keyc * P.k_ss + (long)h * P.k_sh + 16 * g;
    const float* vp = P.v + (long)b * P.v_sb + (long)keyc * P.v_ss + (long)h * P.v_sh + 16 * g;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(kp + 4 * j);
      const f32x4 v = *reinterpret_cast<const f32x4*>(vp + 4 * j);
      kf[4 * j] = a.x; kf[4 * j + 1] = a.y; kf[4 * j + 2] = a.z; kf[4 * j + 3] = a.w;
      vf[4 * j] = v.x; vf[4 * j + 1] = v.y; vf[4 * j + 2] = v.z; vf[4 * j + 3] = v.w;
    }
  }
  const float dscale = DROP ? 1.f / (1.f - P.p_drop) : 1.f;
  const float capinv = CAP ? 1.f / P.softcap : 0.f;
  const uint32_t seed = DROP ? eff_seed(P.seed) : 0u;
  const bool kok = key_ok(P, b, key);
  const int ksg = P.q_seg ? seg_at(P.k_seg, b, P.Sk, key) : 0;
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    dk[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    dv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float* qb = P.q + (long)b * P.q_sb + (long)h * P.q_sh;
  const float* ob = P.dout + (long)b * P.do_sb + (long)h * P.do_sh;
  int qstart = 0;
  if (P.causal) qstart = max(0, (k0 - P.causal_off) / BQ * BQ);
  int qend = P.Sq;
  bool glob_blk;  // the block holds a valid global key: every query block sees it
  const int kwin = key_window(P, b, k0, key, kok, glob_blk);
  if (!glob_blk) band_range(P, k0, qstart, qend);
  if constexpr (LISTS) {
    // follow the key block's list of query blocks — the transpose of the key lists, repeats included
    int li, le;
    list_range(P, P.ql_ptr, h, (P.Sk + 63) / 64, (int)blockIdx.x, li, le);
    for (; li < le; ++li) {
      const int q0 = list_block(P.ql_idx, li, (P.Sq + 63) / 64);
      if (q0 < 0) continue;
#include "attn_f32_dkdv_block.h"
    }
  } else {
    for (int q0 = qstart; q0 < qend; q0 += BQ) {
      if (seg_apart(P, b, q0, k0)) continue;
#include "attn_f32_dkdv_block.h"
    }
  }
  // dk[dt][i] = dK[key = k0 + 16 w + 4 g + i][d = 16 dt + c]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int kr = k0 + 16 * w + 4 * g + i;
    if (kr >= P.Sk) continue;
    float* dkp = P.dk + (long)b * P.dk_sb + (long)kr * P.dk_ss + (long)h * P.dk_sh;
    float* dvp = P.dv + (long)b * P.dv_sb + (long)kr * P.dv_ss + (long)h * P.dv_sh;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      dkp[16 * dt + c] = dk[dt][i] * P.scale;
      dvp[16 * dt + c] = dv[dt][i];
    }
  }
}

}  // namespace

extern "C" int dllm_attn_f32_fwd(AttnF32Params* pp, hipStream_t st) {
  const AttnF32Params& P = *pp;
  // the binding checks it first: no cap with a bias LUT, segments, global keys or lists
  if (P.softcap > 0.f && (P.kl_ptr != nullptr || P.lut != nullptr || P.q_seg != nullptr || P.k_glob != nullptr)) return -2;
  dim3 grid((P.Sq + BQ - 1) / BQ, P.B * P.H);
  if (P.kl_ptr != nullptr) {  // the instantiations that follow block lists
    if (P.p_drop > 0.f) hipLaunchKernelGGL((attn_f32_fwd_kernel<true, true>), grid, dim3(NT), 0, st, P);
    else hipLaunchKernelGGL((attn_f32_fwd_kernel<false, true>), grid, dim3(NT), 0, st, P);
  } else if (P.softcap > 0.f) {  // the instantiations that cap the scores
    if (P.p_drop > 0.f) hipLaunchKernelGGL((attn_f32_fwd_kernel<true, false, true>), grid, dim3(NT), 0, st, P);
    else hipLaunchKernelGGL((attn_f32_fwd_kernel<false, false, true>), grid, dim3(NT), 0, st, P);
  } else if (P.p_drop > 0.f) hipLaunchKernelGGL(attn_f32_fwd_kernel<true>, grid, dim3(NT), 0, st, P);
  else hipLaunchKernelGGL(attn_f32_fwd_kernel<false>, grid, dim3(NT), 0, st, P);
  DLLM_CHECK_LAUNCH();
  return 0;
}

extern "C" int dllm_attn_f32_bwd(AttnF32Params* pp, hipStream_t st) {
  const AttnF32Params& P = *pp;
  if (P.softcap > 0.f && (P.kl_ptr != nullptr || P.lut != nullptr || P.q_seg != nullptr || P.k_glob != nullptr)) return -2;
  const long rows = (long)P.B * P.H * P.Sq;
  hipLaunchKernelGGL(attn_f32_delta_kernel, dim3((unsigned)((rows + NT / 16 - 1) / (NT / 16))), dim3(NT), 0, st, P);
  DLLM_CHECK_LAUNCH();
  dim3 gq((P.Sq + BQ - 1) / BQ, P.B * P.H), gk((P.Sk + BKY - 1) / BKY, P.B * P.H);
  if (P.kl_ptr != nullptr) {  // the instantiations that follow block lists
    if (P.p_drop > 0.f) {
      hipLaunchKernelGGL((attn_f32_dq_kernel<true, true>), gq, dim3(NT), 0, st, P);
      hipLaunchKernelGGL((attn_f32_dkdv_kernel<true, true>), gk, dim3(NT), 0, st, P);
    } else {
      hipLaunchKernelGGL((attn_f32_dq_kernel<false, true>), gq, dim3(NT), 0, st, P);
      hipLaunchKernelGGL((attn_f32_dkdv_kernel<false, true>), gk, dim3(NT), 0, st, P);
    }
  } else if (P.softcap > 0.f) {  // the instantiations that cap the scores
    if (P.p_drop > 0.f) {
      hipLaunchKernelGGL((attn_f32_dq_kernel<true, false, true>), gq, dim3(NT), 0, st, P);
      hipLaunchKernelGGL((attn_f32_dkdv_kernel<true, false, true>), gk, dim3(NT), 0, st, P);
    } else {
      hipLaunchKernelGGL((attn_f32_dq_kernel<false, false, true>), gq, dim3(NT), 0, st, P);
      hipLaunchKernelGGL((attn_f32_dkdv_kernel<false, false, true>), gk, dim3(NT), 0, st, P);
    }
  } else if (P.p_drop > 0.f) {
    hipLaunchKernelGGL(attn_f32_dq_kernel<true>, gq, dim3(NT), 0, st, P);
    hipLaunchKernelGGL(attn_f32_dkdv_kernel<true>, gk, dim3(NT), 0, st, P);
  } else {
    hipLaunchKernelGGL(attn_f32_dq_kernel<false>, gq, dim3(NT), 0, st, P);
    hipLaunchKernelGGL(attn_f32_dkdv_kernel<false>, gk, dim3(NT), 0, st, P);
  }
  DLLM_CHECK_LAUNCH();
  return 0;
}
