// Low-rank adapter (LoRA) kernels: y[:, c0:c0+n] += s * dropout(x) A^T B^T with rank r <= 64 (ops/lora.py).
// bf16 operands, fp32 accumulation on v_mfma_f32_16x16x32_bf16; r is padded to the MFMA shape inside the kernels
// (rows / columns past r are staged as zeros and never stored).  Dropout decisions are the row-Weyl hash of
// ops/rng.py rowwise_keep_mask (common.h rw_*), regenerated wherever they are needed: no mask and no dropped copy of
// x is ever written.  The mask only zeroes operand elements; the 1 / (1 - p) factor travels in `alpha` and is applied
// to the fp32 accumulator (one rounding).
//
//   down    t[N, r] = bf16(alpha * (keep . x)[N, K] A[r, K]^T).  x may be a column slice (row stride ldx): the
//           backward's dt = s * dY[:, c0:c0+n] B runs here with A = B^T.  One wave per 32 rows, x streamed once from
//           global memory in MFMA operand order (16 B per lane), A from L2.  No LDS, no barrier.
//   up      y[N, ld] columns [c0, c0+n) += alpha * (keep .) (t[N, r] M), M = [n, r] (the forward, M = B) or [r, n]
//           (kmajor: the backward's dx += keep . (dt A) / (1 - p)).  One read and one write of the slice, 16 B per
//           lane, 64 contiguous bytes per row and instruction.  M's fragments are loaded once per wave and reused
//           over 128 rows.  No LDS, no barrier.
//   wgrad   G (+)= alpha * Wide^T Small over tokens: Wide [N, wc] (row stride ldw, optionally masked: x), Small
//           [N, r]; G is [wc, r] (wide_major: dB += s * dY_s^T t) or [r, wc] (dA += dt^T dropout(x)).  Tokens are cut
//           into fixed splits; every (64-column strip, split) workgroup writes an fp32 partial, and a second kernel
//           sums the splits in ascending order into G (fp32 or bf16, beta = 1).  No atomics: bitwise reproducible.
//           Both operands are token-major, so the 64-token chunks are staged row-major in LDS and read through the
//           hardware-transposed ds_read_b64_tr_b16 (the key order of csrc/attn_hd.hip ld_tr2, the same for both).
#include "common.h"

using namespace dllm;

DLLM_SEED_STEP_TU(lora)

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8v;
typedef __attribute__((ext_vector_type(4))) short s16x4;

constexpr int kWgradRows = 2048;      // tokens per split of the weight-gradient reduction ...
constexpr int kWgradMaxSplits = 128;  // ... grown (in 64-token steps) where that would make more splits than this

DLLM_DEVICE f32x4 mma(bf16x8v a, bf16x8v b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
DLLM_DEVICE bf16x8v as_op(u16x8 v) { return __builtin_bit_cast(bf16x8v, v); }

// columns k .. k + 7 of a row of `len` valid columns (0: the row itself is out of range), zeros past the end.
// vec: len % 8 == 0 and the row is 16-B aligned (one 16-B load), else element loads.
DLLM_DEVICE u16x8 ld8(const uint16_t* row, int k, int len, bool vec) {
  u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (vec) {
    if (k < len) v = *reinterpret_cast<const u16x8*>(row + k);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (k + j < len) v[j] = row[k + j];
  }
  return v;
}

// zero the dropped ones of columns col .. col + 7 (col % 8 == 0) of the row with hash rh
DLLM_DEVICE u16x8 mask8(u16x8 v, uint32_t rh, uint32_t t2, uint32_t col) {
  u32x4 w = __builtin_bit_cast(u32x4, v);
  const uint32_t g = rw_gbase(rh, col >> 1);
#pragma unroll
  for (int q = 0; q < 4; ++q) w[q] &= ~rw_drop2(rw_pair_y(g + (uint32_t)q * RW_G), t2);
  return __builtin_bit_cast(u16x8, w);
}

// ---------------------------------------------------------------------------------------------------- down
template <int RT>  // 16-row tiles of A
__global__ __launch_bounds__(256) void lora_down_k(const uint16_t* __restrict__ x, long ldx,
                                                   const uint16_t* __restrict__ A, uint16_t* __restrict__ t, int N,
                                                   int K, int r, float alpha, uint32_t seed, uint32_t t2, int drop,
                                                   uint32_t row0) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const long tok0 = (long)blockIdx.x * 128 + w * 32;
  if (tok0 >= N) return;  // the whole wave: nothing below synchronises
  const long tok[2] = {tok0 + c, tok0 + 16 + c};
  uint32_t rh[2] = {0u, 0u};
  if (drop) {
    const uint32_t es = eff_seed(seed);
    rh[0] = mix32(es, row0 + (uint32_t)tok[0]);
    rh[1] = mix32(es, row0 + (uint32_t)tok[1]);
  }
  f32x4 acc[2][RT];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[m][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 32) {
    const int k = k0 + 8 * g;
    bf16x8v xf[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      u16x8 v = ld8(x + (tok[m] < N ? tok[m] : 0) * ldx, k, tok[m] < N ? K : 0, true);
      if (drop) v = mask8(v, rh[m], t2, (uint32_t)k);
      xf[m] = as_op(v);
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int rr = rt * 16 + c;
      const bf16x8v a = as_op(ld8(A + (long)(rr < r ? rr : 0) * K, k, rr < r ? K : 0, true));
      acc[0][rt] = mma(a, xf[0], acc[0][rt]);  // D[r index 4g + i][token c]
      acc[1][rt] = mma(a, xf[1], acc[1][rt]);
    }
  }
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    if (tok[m] >= N) continue;
    uint16_t* tp = t + tok[m] * r;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int rr = rt * 16 + 4 * g;
      if ((r & 3) == 0) {
        if (rr < r) Elem<uint16_t>::store4(tp + rr, acc[m][rt] * alpha);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (rr + i < r) tp[rr + i] = f2bf(acc[m][rt][i] * alpha);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- up
template <int KS>  // 32-wide steps over the padded rank
__global__ __launch_bounds__(256) void lora_up_k(const uint16_t* __restrict__ t, int r, const uint16_t* __restrict__ M,
                                                 int kmajor, uint16_t* __restrict__ y, long ld, int c0, int n, int N,
                                                 float alpha, uint32_t seed, uint32_t t2, int drop, uint32_t row0) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int j0 = blockIdx.y * 64;
  const long wtok0 = (long)blockIdx.x * 512 + w * 128;
  if (wtok0 >= N) return;  // the whole wave: nothing below synchronises
  // M fragments: tile 2u + e, operand row m = c <-> slice column j0 + 32u + 8 (c >> 2) + 4e + (c & 3), so that the
  // accumulators of the tile pair u hold 8 consecutive columns j0 + 32u + 8g .. + 7 of one row
  bf16x8v mf[4][KS];
  const bool vecM = !kmajor && (r & 7) == 0;
#pragma unroll
  for (int tl = 0; tl < 4; ++tl) {
    const int j = j0 + 32 * (tl >> 1) + 8 * (c >> 2) + 4 * (tl & 1) + (c & 3);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = 32 * ks + 8 * g;
      u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (j < n) {
        if (!kmajor) {
          v = ld8(M + (long)j * r, k, r, vecM);
        } else {
#pragma unroll
          for (int q = 0; q < 8; ++q)
            if (k + q < r) v[q] = M[(long)(k + q) * n + j];
        }
      }
      mf[tl][ks] = as_op(v);
    }
  }
  const bool vecT = (r & 7) == 0;
  const uint32_t es = drop ? eff_seed(seed) : 0u;
  for (int it = 0; it < 4; ++it) {
    const long tb = wtok0 + 32 * it;
    if (tb >= N) break;  // wave-uniform
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const long tok = tb + 16 * m + c;
      const bool live = tok < N;
      bf16x8v tf[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) tf[ks] = as_op(ld8(t + (live ? tok : 0) * r, 32 * ks + 8 * g, live ? r : 0, vecT));
      f32x4 acc[4];
#pragma unroll
      for (int tl = 0; tl < 4; ++tl) {
        acc[tl] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) acc[tl] = mma(mf[tl][ks], tf[ks], acc[tl]);
      }
      const uint32_t rh = drop ? mix32(es, row0 + (uint32_t)tok) : 0u;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int j = j0 + 32 * u + 8 * g;
        if (!live || j >= n) continue;
        uint16_t* yp = y + tok * ld + c0 + j;
        const u16x8 old = *reinterpret_cast<const u16x8*>(yp);
        f32x4 lo = acc[2 * u] * alpha, hi = acc[2 * u + 1] * alpha;
        if (drop) {
          const uint32_t gb = rw_gbase(rh, (uint32_t)j >> 1);
          const uint32_t d0 = rw_drop2(rw_pair_y(gb), t2), d1 = rw_drop2(rw_pair_y(gb + RW_G), t2);
          const uint32_t d2 = rw_drop2(rw_pair_y(gb + 2u * RW_G), t2), d3 = rw_drop2(rw_pair_y(gb + 3u * RW_G), t2);
          if (d0 & 0xFFFFu) lo.x = 0.f;
          if (d0 >> 16) lo.y = 0.f;
          if (d1 & 0xFFFFu) lo.z = 0.f;
          if (d1 >> 16) lo.w = 0.f;
          if (d2 & 0xFFFFu) hi.x = 0.f;
          if (d2 >> 16) hi.y = 0.f;
          if (d3 & 0xFFFFu) hi.z = 0.f;
          if (d3 >> 16) hi.w = 0.f;
        }
        u32x4 out;
        out.x = pack_bf16x2(bf2f(old[0]) + lo.x, bf2f(old[1]) + lo.y);
        out.y = pack_bf16x2(bf2f(old[2]) + lo.z, bf2f(old[3]) + lo.w);
        out.z = pack_bf16x2(bf2f(old[4]) + hi.x, bf2f(old[5]) + hi.y);
        out.w = pack_bf16x2(bf2f(old[6]) + hi.z, bf2f(old[7]) + hi.w);
        *reinterpret_cast<u32x4*>(yp) = out;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- wgrad
// MFMA operand whose reduction index is the tile row (token): for the lane (c, g), column c0 + c of rows
// rb + 4g + {0..3} (elements 0..3) and rb + 16 + 4g + {0..3} (elements 4..7); csrc/attn_hd.hip ld_tr2 with a runtime
// row stride.  EXEC must be full.
DLLM_DEVICE bf16x8v ld_tr(const uint16_t* img, int LD, int rb, int c0, int c, int g) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const uint16_t* p = img + (rb + 4 * g + (c >> 2)) * LD + c0 + 4 * (c & 3);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 16 * LD));
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  const s16x8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  return __builtin_bit_cast(bf16x8v, v);
}

template <int RT>  // 16-column tiles of Small
__global__ __launch_bounds__(256) void lora_wgrad_k(const uint16_t* __restrict__ Wd, long ldw, int wc,
                                                    const uint16_t* __restrict__ S, int r, float* __restrict__ part,
                                                    int N, int rows_per_split, int wide_major, uint32_t seed,
                                                    uint32_t t2, int drop, uint32_t row0) {
  constexpr int LW = 72, LS = 16 * RT + 8;  // row strides (elements): 16-B pad, 8-B aligned transposed reads
  __shared__ __attribute__((aligned(16))) uint16_t imgW[64 * LW];
  __shared__ __attribute__((aligned(16))) uint16_t imgS[64 * LS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  const int w0 = blockIdx.x * 64;
  const long t_begin = (long)blockIdx.y * rows_per_split;
  const long t_end = t_begin + rows_per_split < N ? t_begin + rows_per_split : N;
  const uint32_t es = drop ? eff_seed(seed) : 0u;
  const bool vecS = (r & 7) == 0;
  f32x4 acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long tb = t_begin; tb < t_end; tb += 64) {  // block-uniform bounds: the barriers stay matched
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int idx = tid + 256 * j, rr = idx >> 3, ch = idx & 7;
      const long tok = tb + rr;
      const int col = w0 + 8 * ch;
      u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (tok < t_end && col < wc) {
        v = *reinterpret_cast<const u16x8*>(Wd + tok * ldw + col);
        if (drop) v = mask8(v, mix32(es, row0 + (uint32_t)tok), t2, (uint32_t)col);
      }
      *reinterpret_cast<u16x8*>(imgW + rr * LW + 8 * ch) = v;
    }
    if (vecS) {
      for (int idx = tid; idx < 64 * 2 * RT; idx += 256) {
        const int rr = idx / (2 * RT), ch = idx % (2 * RT);
        const long tok = tb + rr;
        const u16x8 v = ld8(S + (tok < t_end ? tok : 0) * r, 8 * ch, tok < t_end ? r : 0, true);
        *reinterpret_cast<u16x8*>(imgS + rr * LS + 8 * ch) = v;
      }
    } else {
      for (int idx = tid; idx < 64 * 16 * RT; idx += 256) {
        const int rr = idx / (16 * RT), k = idx % (16 * RT);
        const long tok = tb + rr;
        imgS[rr * LS + k] = (tok < t_end && k < r) ? S[tok * r + k] : (uint16_t)0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const bf16x8v aw = ld_tr(imgW, LW, 32 * kk, 16 * w, c, g);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const bf16x8v as = ld_tr(imgS, LS, 32 * kk, 16 * rt, c, g);
        acc[rt] = wide_major ? mma(as, aw, acc[rt]) : mma(aw, as, acc[rt]);
      }
    }
  }
  float* out = part + (long)blockIdx.y * wc * r;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (wide_major) {  // D[small 4g + i][wide c] -> G[wide, small]
        const int wcol = w0 + 16 * w + c, rr = 16 * rt + 4 * g + i;
        if (wcol < wc && rr < r) out[(long)wcol * r + rr] = acc[rt][i];
      } else {  // D[wide 4g + i][small c] -> G[small, wide]
        const int wcol = w0 + 16 * w + 4 * g + i, rr = 16 * rt + c;
        if (wcol < wc && rr < r) out[(long)rr * wc + wcol] = acc[rt][i];
      }
    }
  }
}

// G (+)= alpha * sum over splits, in ascending split order
__global__ __launch_bounds__(256) void lora_wgrad_reduce_k(const float* __restrict__ part, int splits, long numel,
                                                           void* G, int g_bf16, float alpha, int beta) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= numel) return;
  float s = 0.f;
  for (int sp = 0; sp < splits; ++sp) s += part[(long)sp * numel + i];
  s *= alpha;
  if (g_bf16) {
    uint16_t* p = reinterpret_cast<uint16_t*>(G) + i;
    *p = f2bf(beta ? bf2f(*p) + s : s);
  } else {
    float* p = reinterpret_cast<float*>(G) + i;
    *p = beta ? *p + s : s;
  }
}

}  // namespace

extern "C" int dllm_lora_wgrad_rows() { return kWgradRows; }
extern "C" int dllm_lora_wgrad_max_splits() { return kWgradMaxSplits; }

// tokens per split for N tokens: kWgradRows, or more (a multiple of 64) where that keeps the splits <= kWgradMaxSplits
extern "C" int dllm_lora_wgrad_split_rows(long N) {
  long rows = kWgradRows;
  if ((N + rows - 1) / rows > kWgradMaxSplits) rows = ((N + kWgradMaxSplits - 1) / kWgradMaxSplits + 63) / 64 * 64;
  return (int)rows;
}

extern "C" int dllm_lora_down(const void* x, long ldx, const void* A, void* t, int N, int K, int r, float alpha, float p,
                              uint32_t seed, uint32_t row0, hipStream_t st) {
  if (N <= 0) return 0;
  const int drop = p > 0.f;
  const uint32_t t2 = rw_t2(drop_threshold(p));
  const dim3 grid((N + 127) / 128), block(256);
  const int RT = (r + 15) / 16;
#define DLLM_LORA_DOWN(R)                                                                                         \
  lora_down_k<R><<<grid, block, 0, st>>>((const uint16_t*)x, ldx, (const uint16_t*)A, (uint16_t*)t, N, K, r, alpha, \
                                         seed, t2, drop, row0)
  switch (RT) {
    case 1: DLLM_LORA_DOWN(1); break;
    case 2: DLLM_LORA_DOWN(2); break;
    case 3: DLLM_LORA_DOWN(3); break;
    case 4: DLLM_LORA_DOWN(4); break;
    default: return -1;
  }
#undef DLLM_LORA_DOWN
  DLLM_CHECK_LAUNCH();
  return 0;
}

extern "C" int dllm_lora_up(const void* t, int r, const void* M, int kmajor, void* y, long ld, int c0, int n, int N,
                            float alpha, float p, uint32_t seed, uint32_t row0, hipStream_t st) {
  if (N <= 0 || n <= 0) return 0;
  const int drop = p > 0.f;
  const uint32_t t2 = rw_t2(drop_threshold(p));
  const dim3 grid((N + 511) / 512, (n + 63) / 64), block(256);
  if (r < 1 || r > 64 || grid.y > 65535) return -1;
  if (r <= 32)
    lora_up_k<1><<<grid, block, 0, st>>>((const uint16_t*)t, r, (const uint16_t*)M, kmajor, (uint16_t*)y, ld, c0, n, N,
                                         alpha, seed, t2, drop, row0);
  else
    lora_up_k<2><<<grid, block, 0, st>>>((const uint16_t*)t, r, (const uint16_t*)M, kmajor, (uint16_t*)y, ld, c0, n, N,
                                         alpha, seed, t2, drop, row0);
  DLLM_CHECK_LAUNCH();
  return 0;
}

// part: fp32 scratch of splits * wc * r elements, splits = ceil(N / rows_per_split)
extern "C" int dllm_lora_wgrad(const void* Wd, long ldw, int wc, const void* S, int r, float* part, int N,
                               int rows_per_split, int wide_major, void* G, int g_bf16, float alpha, int beta, float p,
                               uint32_t seed, uint32_t row0, hipStream_t st) {
  if (N <= 0 || wc <= 0) return 0;
  const int drop = p > 0.f;
  const uint32_t t2 = rw_t2(drop_threshold(p));
  const int splits = (N + rows_per_split - 1) / rows_per_split;
  const dim3 grid((wc + 63) / 64, splits), block(256);
  if (splits > 65535) return -1;
  const int RT = (r + 15) / 16;
#define DLLM_LORA_WGRAD(R)                                                                                      \
  lora_wgrad_k<R><<<grid, block, 0, st>>>((const uint16_t*)Wd, ldw, wc, (const uint16_t*)S, r, part, N,           \
                                          rows_per_split, wide_major, seed, t2, drop, row0)
  switch (RT) {
    case 1: DLLM_LORA_WGRAD(1); break;
    case 2: DLLM_LORA_WGRAD(2); break;
    case 3: DLLM_LORA_WGRAD(3); break;
    case 4: DLLM_LORA_WGRAD(4); break;
    default: return -1;
  }
#undef DLLM_LORA_WGRAD
  DLLM_CHECK_LAUNCH();
  const long numel = (long)wc * r;
  lora_wgrad_reduce_k<<<dim3((unsigned)((numel + 255) / 256)), block, 0, st>>>(part, splits, numel, G, g_bf16, alpha,
                                                                              beta);
  DLLM_CHECK_LAUNCH();
  return 0;
}
