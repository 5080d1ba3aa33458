// NF4 (QLoRA) frozen base weights for gfx950 (MI355X / CDNA4): quantiser, dequantiser and the two projection GEMMs that
// read the 4-bit codes directly (ops/nf4.py states the contract; its torch composite is the oracle of this file).
//
// Storage (the only layout; read as it stands): W [N][K] as codes uint8 [N][K/2] (byte j of a row = element 2j in the
// high nibble, 2j+1 in the low one) and absmax fp32 [N][K/64] (one scale per 64 consecutive k of a row).  N, K % 64 == 0.
// deq(W)[n][k] = bf16(NF4[code] * absmax[n][k / 64]): one fp32 multiply, one rounding — the only rounding in front of
// the MFMA.  gfx950 has no matrix format with this code book (its MX fp4 is E2M1), so the codes become bf16 operands
// on the way through LDS.
//
//   quantize   16 lanes per 64-block (4 elements each): |w| max over the 16 lanes by shuffles, v = w / absmax (one
//              correctly rounded division), code = number of the 15 fp32 midpoints below v; 2 bytes stored per lane.
//   dequant    one thread per 8 codes (4 B in, 16 B out); serves the `dequant` route and merge_lora.
//   NT  Y[M][N] = X[M][K] . deq(W)[N][K]^T (+ bias)           forward
//   NN  dX[M][K] = dY[M][N] . deq(W)[N][K]  (reduction over N) input gradient
//
// The GEMMs.  256 threads = 4 waves as 2 x 2 over a BM x BN output tile, one tile per workgroup, reduction in steps of
// 64; fp32 accumulators of v_mfma_f32_16x16x32_bf16 with the WEIGHT fragment as the first operand, so a lane holds 4
// consecutive output columns of one row and stores them as 8 bytes.
// * Work split.  NT <128, 128>: training token counts, 64 x 64 per wave (4 x 4 accumulators, 64 fp32 per lane).
//   NT <64, 32>: the decode step's rows (M <= 64): the kernel is a weight stream there, so the tile is narrow in N —
//   N / 32 workgroups, 4x as many as the wide tile would give, each reading 32 rows of codes — and small enough
//   (24 KB of LDS) for several workgroups per CU.  NN <128>: 128 rows x 128 k-columns, 64 weight rows per step.
// * Global -> registers.  Per step a thread loads 16 B of codes = 32 codes (NT: half of a row's 64-deep step, whose
//   32 B and one scale two neighbouring lanes read; NN: a quarter of a weight row's 128 k-columns, two quantisation
//   blocks per row) plus the block's scale, and its 16-B pieces of the activation tile.  Rows past M, weight rows past
//   N (NT) and k-columns past K (NN) are loaded as zeros / scale 0; their outputs are never stored.
// * Registers -> LDS.  Each code indexes the 16-entry table held ACROSS THE LANES of one register (lane l holds
//   NF4[l & 15]; ds_bpermute_b32 fetches lane `code`: no LDS table, no bank conflicts), is scaled in fp32, and pairs
//   are rounded to bf16 by one v_cvt_pk_bf16_f32.  Every element of a tile is expanded ONCE per workgroup and then
//   serves, out of LDS, every MFMA row block of the tile: BM / 16 MFMAs read each expanded element (8 for the 128-row
//   tiles, 4 for the decode tile).
// * LDS images (two buffers of [activations | weights], step t in buffer t & 1).  Row-major [rows][64] bf16 images
//   (128-B rows: X, dY, the NT weights) store 16-B chunk c of row r at chunk c ^ ((r >> 1) & 7): the 16 lanes of a
//   ds_read_b128 fragment read (rows r0 .. r0+15, one chunk) then cover all 64 banks once.  The NN weight image is
//   [64 n][128 k] (256-B rows, reduction-major) with chunk c of row r at c ^ gsw(r) and is read through the
//   hardware-transposed ds_read_b64_tr_b16 (as csrc/gemm_w4.hip's k-major B operand): the 8 rows x 32 B a half wave
//   reads fall into 8 distinct 32-B bank groups.
// * Pipeline.  One barrier per step: the global loads of step t+1 are issued before the MFMAs of step t, their
//   expansion and LDS stores into the other buffer follow in program order and are free to overlap those MFMAs (no
//   dependence); the barrier closes the step.
// * Deterministic: no atomics, no split-K, a fixed reduction order per output element.
#include "common.h"

using namespace dllm;

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8v;
typedef __attribute__((ext_vector_type(4))) short s16x4;

constexpr int kDecodeRows = 64;  // NT: M <= this runs the <64, 32> tile

__constant__ const float kNF4[16] = {-1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f,
                                     -0.28444138169288635f, -0.18477343022823334f, -0.09105003625154495f, 0.0f,
                                     0.07958029955625534f, 0.16093020141124725f, 0.24611230194568634f,
                                     0.33791524171829224f, 0.44070982933044434f, 0.5626170039176941f,
                                     0.7229568362236023f, 1.0f};

DLLM_DEVICE f32x4 mma(bf16x8v a, bf16x8v b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// ------------------------------------------------------------------------------------------------ quantize / dequant
template <typename T>
__global__ __launch_bounds__(256) void nf4_quantize_k(const T* __restrict__ w, uint8_t* __restrict__ codes,
                                                      float* __restrict__ absmax, long quads) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;  // 4 elements per thread, 16 threads per block of 64
  const bool live = q < quads;                           // quads % 16 == 0: a 16-lane group is live as a whole
  const f32x4 v = live ? Elem<T>::load4(w + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
  float a = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) a = fmaxf(a, __shfl_xor(a, m, 64));
  uint32_t c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float x = __fdiv_rn(v[i], a);
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < 15; ++j) n += x > (kNF4[j] + kNF4[j + 1]) * 0.5f ? 1u : 0u;
    c[i] = a == 0.f ? 7u : n;
  }
  if (!live) return;
  *reinterpret_cast<uint16_t*>(codes + 2 * q) = (uint16_t)((c[0] << 4) | c[1] | (c[2] << 12) | (c[3] << 8));
  if ((q & 15) == 0) absmax[q >> 4] = a;
}

__global__ __launch_bounds__(256) void nf4_dequant_k(const uint8_t* __restrict__ codes, const float* __restrict__ absmax,
                                                     uint16_t* __restrict__ out, long octs) {
  const long o = (long)blockIdx.x * 256 + threadIdx.x;  // 8 elements per thread
  if (o >= octs) return;
  const uint32_t x = *reinterpret_cast<const uint32_t*>(codes + 4 * o);
  const float s = absmax[o >> 3];
  u32x4 r;
#pragma unroll
  for (int b = 0; b < 4; ++b) r[b] = pack_bf16x2(kNF4[(x >> (8 * b + 4)) & 15u] * s, kNF4[(x >> (8 * b)) & 15u] * s);
  *reinterpret_cast<u32x4*>(out + 8 * o) = r;
}

// -------------------------------------------------------------------------------------------------------- expansion
// 32 codes (16 B as loaded) -> 32 bf16 (16 packed pairs, element order): tab holds NF4[lane & 15], every lane of the
// wave must be active (the lookup reads lanes 0 .. 15)
DLLM_DEVICE void expand32(const u32x4& cw, float scale, float tab, uint32_t (&out)[16]) {
  const int t = __float_as_int(tab);
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t x = cw[w];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int ihi = (int)((x >> (8 * b + 2)) & 0x3Cu);  // 4 * high nibble of byte b: bpermute takes a byte address
      const int ilo = b == 0 ? (int)((x << 2) & 0x3Cu) : (int)((x >> (8 * b - 2)) & 0x3Cu);
      const float hi = __int_as_float(__builtin_amdgcn_ds_bpermute(ihi, t)) * scale;
      const float lo = __int_as_float(__builtin_amdgcn_ds_bpermute(ilo, t)) * scale;
      out[4 * w + b] = pack_bf16x2(hi, lo);
    }
  }
}

// byte offset of 16-B chunk ch of row r in a [rows][64] bf16 image
DLLM_DEVICE uint32_t off_rm(int r, int ch) { return (uint32_t)(r * 128 + ((ch ^ ((r >> 1) & 7)) << 4)); }

// [64][128] bf16 reduction-major image (256-B rows) of the NN weight tile (csrc/gemm_w4.hip's k-major swizzle)
DLLM_DEVICE int gsw(int r) { return ((r & 3) << 2) ^ (((r >> 3) & 1) << 1); }
DLLM_DEVICE uint32_t off_km(int r, int col) {
  return (uint32_t)((r << 8) + ((((col >> 3) ^ gsw(r)) << 3) + (col & 7)) * 2);
}
// operand from that image: lane l holds column cb + (l & 15), rows kk + 8 (l >> 4) + 0 .. 7.  EXEC must be full.
DLLM_DEVICE bf16x8v frag_km(const unsigned char* img, int kk, int cb, int lane) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const int i = lane & 15, r = kk + 8 * (lane >> 4) + (i >> 2), col = cb + 4 * (i & 3);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + off_km(r, col)));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + off_km(r + 4, col)));
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  const s16x8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  return __builtin_bit_cast(bf16x8v, v);
}

DLLM_DEVICE bf16x8v frag_rm(const unsigned char* img, int r, int ch) {
  return *reinterpret_cast<const bf16x8v*>(img + off_rm(r, ch));
}

// ---------------------------------------------------------------------------------------------------------------- NT
template <int BM, int BN>
__global__ __launch_bounds__(256) void gemm_nf4_nt_k(const uint16_t* __restrict__ X, long ldx,
                                                     const uint8_t* __restrict__ codes,
                                                     const float* __restrict__ absmax,
                                                     const uint16_t* __restrict__ bias, uint16_t* __restrict__ Y,
                                                     long ldy, int M, int N, int K) {
  constexpr int TM = BM / 32, TN = BN / 32;  // 16 x 16 accumulators per wave (2 x 2 waves)
  constexpr int XL = BM * 8 / 256;           // 16-B pieces of the X tile per thread
  constexpr int WL = (2 * BN + 255) / 256;   // 16-B code loads per thread; 2 BN < 256: the first 2 BN threads only
  static_assert(BM % 32 == 0 && BN % 32 == 0 && (2 * BN) % 64 == 0, "tile");
  constexpr uint32_t XB = BM * 128, BUF = (BM + BN) * 128;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BUF];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  const int wm = w >> 1, wn = w & 1;
  const long m0 = (long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const float tab = kNF4[lane & 15];
  const int nk = K / 64;
  const long cld = K / 2, sld = K / 64;  // row strides of codes (bytes) and absmax (elements)

  u16x8 xr[XL];
  u32x4 cr[WL];
  float sr[WL];
  auto gload = [&](int t) {
#pragma unroll
    for (int j = 0; j < XL; ++j) {
      const int idx = tid + 256 * j;
      const long row = m0 + (idx >> 3);
      xr[j] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (row < M) xr[j] = *reinterpret_cast<const u16x8*>(X + row * ldx + t * 64 + 8 * (idx & 7));
    }
#pragma unroll
    for (int j = 0; j < WL; ++j) {
      const int idx = tid + 256 * j;
      const int n = n0 + (idx >> 1);
      cr[j] = u32x4{0u, 0u, 0u, 0u};
      sr[j] = 0.f;
      if (idx < 2 * BN && n < N) {
        cr[j] = *reinterpret_cast<const u32x4*>(codes + n * cld + t * 32 + 16 * (idx & 1));
        sr[j] = absmax[n * sld + t];
      }
    }
  };
  auto lstore = [&](int b) {
    unsigned char* xs = smem + b * BUF;
    unsigned char* ws = xs + XB;
#pragma unroll
    for (int j = 0; j < XL; ++j) {
      const int idx = tid + 256 * j;
      *reinterpret_cast<u16x8*>(xs + off_rm(idx >> 3, idx & 7)) = xr[j];
    }
#pragma unroll
    for (int j = 0; j < WL; ++j) {
      const int idx = tid + 256 * j;
      if (2 * BN >= 256 || tid < 2 * BN) {  // whole waves: 2 BN % 64 == 0
        uint32_t o[16];
        expand32(cr[j], sr[j], tab, o);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<u32x4*>(ws + off_rm(idx >> 1, 4 * (idx & 1) + q)) =
              u32x4{o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
      }
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  gload(0);
  lstore(0);
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    const int b = t & 1;
    if (t + 1 < nk) gload(t + 1);
    const unsigned char* xs = smem + b * BUF;
    const unsigned char* ws = xs + XB;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8v xf[TM], wf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) xf[i] = frag_rm(xs, wm * (BM / 2) + 16 * i + c, 4 * kk + g);
#pragma unroll
      for (int j = 0; j < TN; ++j) wf[j] = frag_rm(ws, wn * (BN / 2) + 16 * j + c, 4 * kk + g);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mma(wf[j], xf[i], acc[i][j]);  // D[n 4g + r][m c]
    }
    if (t + 1 < nk) lstore(b ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const long row = m0 + wm * (BM / 2) + 16 * i + c;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = n0 + wn * (BN / 2) + 16 * j + 4 * g;
      if (row < M && col < N) {  // N % 4 == 0: the 4 columns are in range together
        f32x4 v = acc[i][j];
        if (bias != nullptr) v += Elem<uint16_t>::load4(bias + col);
        Elem<uint16_t>::store4(Y + row * ldy + col, v);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- NN
template <int BM>
__global__ __launch_bounds__(256) void gemm_nf4_nn_k(const uint16_t* __restrict__ dY, long ldy,
                                                     const uint8_t* __restrict__ codes,
                                                     const float* __restrict__ absmax, uint16_t* __restrict__ dX,
                                                     long ldx, int M, int N, int K) {
  constexpr int BKC = 128;         // output (k) columns of the tile
  constexpr int TM = BM / 32, TK = BKC / 32;
  constexpr int YL = BM * 8 / 256;  // 16-B pieces of the dY tile per thread
  constexpr uint32_t YB = BM * 128, BUF = YB + 64 * 256;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BUF];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  const int wm = w >> 1, wk = w & 1;
  const long m0 = (long)blockIdx.x * BM;
  const int kc0 = blockIdx.y * BKC;
  const float tab = kNF4[lane & 15];
  const int ns = N / 64;
  const long cld = K / 2, sld = K / 64;
  // this thread's 32 codes of a step: weight row n0 + wr, k-columns kc0 + 32 wq .. + 31 (one quantisation block's half)
  const int wr = tid >> 2, wq = tid & 3;
  const bool wok = kc0 + 32 * wq < K;  // K % 64 == 0: the 32 columns are in range together

  u16x8 yr[YL];
  u32x4 cr;
  float sr;
  auto gload = [&](int t) {
#pragma unroll
    for (int j = 0; j < YL; ++j) {
      const int idx = tid + 256 * j;
      const long row = m0 + (idx >> 3);
      yr[j] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (row < M) yr[j] = *reinterpret_cast<const u16x8*>(dY + row * ldy + t * 64 + 8 * (idx & 7));
    }
    cr = u32x4{0u, 0u, 0u, 0u};
    sr = 0.f;
    if (wok) {
      const long n = (long)t * 64 + wr;
      cr = *reinterpret_cast<const u32x4*>(codes + n * cld + (kc0 + 32 * wq) / 2);
      sr = absmax[n * sld + (kc0 + 32 * wq) / 64];
    }
  };
  auto lstore = [&](int b) {
    unsigned char* ys = smem + b * BUF;
    unsigned char* ws = ys + YB;
#pragma unroll
    for (int j = 0; j < YL; ++j) {
      const int idx = tid + 256 * j;
      *reinterpret_cast<u16x8*>(ys + off_rm(idx >> 3, idx & 7)) = yr[j];
    }
    uint32_t o[16];
    expand32(cr, sr, tab, o);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<u32x4*>(ws + off_km(wr, 32 * wq + 8 * q)) = u32x4{o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
  };

  f32x4 acc[TM][TK];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TK; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  gload(0);
  lstore(0);
  __syncthreads();
  for (int t = 0; t < ns; ++t) {
    const int b = t & 1;
    if (t + 1 < ns) gload(t + 1);
    const unsigned char* ys = smem + b * BUF;
    const unsigned char* ws = ys + YB;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8v yf[TM], wf[TK];
#pragma unroll
      for (int i = 0; i < TM; ++i) yf[i] = frag_rm(ys, wm * (BM / 2) + 16 * i + c, 4 * kk + g);
#pragma unroll
      for (int j = 0; j < TK; ++j) wf[j] = frag_km(ws, 32 * kk, wk * (BKC / 2) + 16 * j, lane);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TK; ++j) acc[i][j] = mma(wf[j], yf[i], acc[i][j]);  // D[k-column 4g + r][m c]
    }
    if (t + 1 < ns) lstore(b ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const long row = m0 + wm * (BM / 2) + 16 * i + c;
#pragma unroll
    for (int j = 0; j < TK; ++j) {
      const int col = kc0 + wk * (BKC / 2) + 16 * j + 4 * g;
      if (row < M && col < K) Elem<uint16_t>::store4(dX + row * ldx + col, acc[i][j]);
    }
  }
}

}  // namespace

extern "C" int dllm_nf4_decode_rows() { return kDecodeRows; }

// w [N][K] contiguous (bf16 or fp32), N * K % 64 == 0 with K % 64 == 0
extern "C" int dllm_nf4_quantize(const void* w, int is_bf16, uint8_t* codes, float* absmax, long N, long K,
                                 hipStream_t st) {
  const long quads = N * K / 4;
  if (quads <= 0) return 0;
  if (K % 64 || (quads + 255) / 256 > 0x7FFFFFFFL) return -1;
  const dim3 grid((unsigned)((quads + 255) / 256)), block(256);
  if (is_bf16) nf4_quantize_k<uint16_t><<<grid, block, 0, st>>>((const uint16_t*)w, codes, absmax, quads);
  else nf4_quantize_k<float><<<grid, block, 0, st>>>((const float*)w, codes, absmax, quads);
  DLLM_CHECK_LAUNCH();
  return 0;
}

extern "C" int dllm_nf4_dequant(const uint8_t* codes, const float* absmax, void* out, long N, long K, hipStream_t st) {
  const long octs = N * K / 8;
  if (octs <= 0) return 0;
  if (K % 64 || (octs + 255) / 256 > 0x7FFFFFFFL) return -1;
  nf4_dequant_k<<<dim3((unsigned)((octs + 255) / 256)), dim3(256), 0, st>>>(codes, absmax, (uint16_t*)out, octs);
  DLLM_CHECK_LAUNCH();
  return 0;
}

// nn = 0: out [M][N] = x [M][K] . deq(W)^T (+ bias [N]); nn = 1: out [M][K] = x [M][N] . deq(W).  W = [N][K] codes /
// absmax; x and out: bf16 rows of stride ldx / ldo elements, 16-B aligned rows.
extern "C" int dllm_gemm_nf4(const void* x, long ldx, const uint8_t* codes, const float* absmax, const void* bias,
                             void* out, long ldo, int M, int N, int K, int nn, hipStream_t st) {
  if (M <= 0) return 0;
  if (N <= 0 || K <= 0 || N % 64 || K % 64) return -1;
  const uint16_t* xp = (const uint16_t*)x;
  uint16_t* op = (uint16_t*)out;
  const dim3 block(256);
  if (nn) {
    const dim3 grid((M + 127) / 128, (K + 127) / 128);
    if (grid.y > 65535 || bias != nullptr) return -1;
    gemm_nf4_nn_k<128><<<grid, block, 0, st>>>(xp, ldx, codes, absmax, op, ldo, M, N, K);
  } else if (M <= kDecodeRows) {
    const dim3 grid(1, N / 32);
    if (grid.y > 65535) return -1;
    gemm_nf4_nt_k<64, 32><<<grid, block, 0, st>>>(xp, ldx, codes, absmax, (const uint16_t*)bias, op, ldo, M, N, K);
  } else {
    const dim3 grid((M + 127) / 128, (N + 127) / 128);
    if (grid.y > 65535) return -1;
    gemm_nf4_nt_k<128, 128><<<grid, block, 0, st>>>(xp, ldx, codes, absmax, (const uint16_t*)bias, op, ldo, M, N, K);
  }
  DLLM_CHECK_LAUNCH();
  return 0;
}
