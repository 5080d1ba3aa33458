// Adafactor (factored second moments, no first moment) over the flat parameter space, for gfx950.
// Semantics: transformers optimization.Adafactor with beta1=None, applied per unit (one transformers parameter: a flat
// segment, or one dim-0 slice of a fused one).  A device table (csrc/adafactor_params.h) describes every unit; each of
// the three tile passes covers all units in one launch, two small finalize kernels sit between them:
//   stats     g -> s = (coef g)^2 + eps1: row / column partial sums of s per tile (1-D units: V blended in place)
//   fin_stats R = b2t R + (1 - b2t) mean_cols(s), C = b2t C + (1 - b2t) mean_rows(s), mean(R) per unit
//   usum      u = g rsqrt(R_i / mean R) rsqrt(C_j) (1-D: g rsqrt(V)): sum u^2 per tile (+ sum w^2 with scale_parameter)
//   fin_clip  per unit: lr_t = rel (max(eps2, rms w) | 1), step = lr_t / max(1, rms(u) / clip), dec = wd lr_t
//   update    w -= dec w; w -= step u; master and (bf16, round to nearest even) parameters written
// No floating-point atomics: every partial sum goes to scratch and is added in a fixed order, so two runs on the same
// inputs agree bit for bit.  Longest sequential fp32 chains: column sums AF_RB rows per lane, then
// ceil(row blocks / AF_FIN_SLICES) partials per slice, a 2-step shuffle tree and 4 waves in order; row sums 4 elements
// per lane, a 6-step wave tree, 4 waves in order, then the column chunks in order.
#include "common.h"
#include "adafactor_params.h"

using namespace dllm;

namespace {

struct Tile {
  long off, rows, cols, rv, c, colpart, rowpart, nchunk, chunk, rb, r0;
  int nr, u, vec, decay;
};

DLLM_DEVICE Tile decode_tile(const long* __restrict__ tab, int U, long tile) {
  int lo = 0, hi = U;  // tab[U] holds the total tile count: the unit is the last one whose first tile is <= tile
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tab[(long)mid * AF_FIELDS + AF_TILE0] <= tile) lo = mid; else hi = mid;
  }
  const long* r = tab + (long)lo * AF_FIELDS;
  Tile t;
  t.u = lo;
  t.off = r[AF_OFF];
  t.rows = r[AF_ROWS];
  t.cols = r[AF_COLS];
  t.rv = r[AF_RV];
  t.c = r[AF_C];
  t.decay = (int)r[AF_DECAY];
  t.colpart = r[AF_COLPART];
  t.rowpart = r[AF_ROWPART];
  t.nchunk = r[AF_NCHUNK];
  t.vec = (int)r[AF_VEC];
  const long local = tile - r[AF_TILE0];
  t.rb = local / t.nchunk;
  t.chunk = local - t.rb * t.nchunk;
  t.r0 = t.rb * AF_RB;
  const long left = t.rows - t.r0;
  t.nr = (int)(left < AF_RB ? left : AF_RB);
  return t;
}

// the 4 columns of a lane inside its wave's AF_WC columns from cbase: 4 adjacent ones (16-byte access) or, on the scalar
// path, 4 strided by 64 so that a wave's accesses stay coalesced
template <bool VEC>
DLLM_DEVICE long colk(long cbase, int lane, int k) {
  return VEC ? cbase + 4 * lane + k : cbase + lane + 64 * k;
}

template <bool VEC, typename T>
DLLM_DEVICE void ld4(const T* __restrict__ base, long cbase, int lane, long cols, bool ok, float v[4]) {
  if constexpr (VEC) {
    const long c = cbase + 4 * lane;
    if (ok && c < cols) {
      const f32x4 x = Elem<T>::load4(base + c);
      v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
      v[0] = v[1] = v[2] = v[3] = 0.f;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long c = cbase + lane + 64 * k;
      v[k] = (ok && c < cols) ? Elem<T>::load(base + c) : 0.f;
    }
  }
}

template <bool VEC, typename T>
DLLM_DEVICE void st4(T* __restrict__ base, long cbase, int lane, long cols, const float v[4]) {
  if constexpr (VEC) {
    const long c = cbase + 4 * lane;
    if (c < cols) Elem<T>::store4(base + c, f32x4{v[0], v[1], v[2], v[3]});
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long c = cbase + lane + 64 * k;
      if (c < cols) Elem<T>::store(base + c, v[k]);
    }
  }
}

// ---------------------------------------------------------------------------------------------- pass 1: statistics
template <bool VEC>
DLLM_DEVICE void stats_tile(const Tile& t, const float* __restrict__ grad, float coef, float eps1, float b2t,
                            float* __restrict__ rv, float* __restrict__ colpart, float* __restrict__ rowpart,
                            float (*lrow)[AF_RB]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long cbase = t.chunk * AF_CC + (long)w * AF_WC;
  if (t.c < 0) {  // 1-D unit: V = b2t V + (1 - b2t) s, elementwise
    float g[4], v[4];
    ld4<VEC>(grad + t.off, cbase, lane, t.cols, true, g);
    ld4<VEC>(rv + t.rv, cbase, lane, t.cols, true, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gg = g[k] * coef;
      v[k] = b2t * v[k] + (1.f - b2t) * (gg * gg + eps1);
    }
    st4<VEC>(rv + t.rv, cbase, lane, t.cols, v);
    return;
  }
  bool cok[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) cok[k] = colk<VEC>(cbase, lane, k) < t.cols;
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
  const float* gbase = grad + t.off + t.r0 * t.cols;
  for (int r = 0; r < t.nr; r += 4) {
    float g[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = r + i < t.nr;
      ld4<VEC>(gbase + (ok ? (long)(r + i) * t.cols : 0), cbase, lane, t.cols, ok, g[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = r + i < t.nr;
      float rs = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float gg = g[i][k] * coef;
        const float s = (ok && cok[k]) ? gg * gg + eps1 : 0.f;
        cs[k] += s;
        rs += s;
      }
      rs = wave_sum(rs);
      if (lane == 0 && ok) lrow[w][r + i] = rs;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < t.nr) {
    const int x = threadIdx.x;
    rowpart[t.rowpart + (t.r0 + x) * t.nchunk + t.chunk] = ((lrow[0][x] + lrow[1][x]) + lrow[2][x]) + lrow[3][x];
  }
  st4<VEC>(colpart + t.colpart + t.rb * t.cols, cbase, lane, t.cols, cs);
  __syncthreads();  // lrow is rewritten by the workgroup's next tile
}

__global__ __launch_bounds__(256) void af_stats(const float* __restrict__ grad, const long* __restrict__ tab, int U,
                                                long n_tiles, const float* __restrict__ coef_p, float eps1, float b2t,
                                                const float* __restrict__ hyper, float* __restrict__ rv,
                                                float* __restrict__ colpart, float* __restrict__ rowpart) {
  __shared__ float lrow[4][AF_RB];
  const float coef = coef_p[0];
  if (hyper != nullptr) b2t = hyper[1];
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const Tile t = decode_tile(tab, U, tile);
    if (t.vec) stats_tile<true>(t, grad, coef, eps1, b2t, rv, colpart, rowpart, lrow);
    else stats_tile<false>(t, grad, coef, eps1, b2t, rv, colpart, rowpart, lrow);
  }
}

// grid (units, AF_FIN_Y).  y == 0 blends the unit's R and writes mean(R); every y blends the column groups y, y +
// AF_FIN_Y, ... of C.
__global__ __launch_bounds__(256) void af_fin_stats(const long* __restrict__ tab, float b2t,
                                                    const float* __restrict__ hyper, float* __restrict__ rv,
                                                    float* __restrict__ cst, const float* __restrict__ colpart,
                                                    const float* __restrict__ rowpart, float* __restrict__ scal) {
  __shared__ float red[4];
  __shared__ float lcol[4][AF_FIN_COLS];
  const long* r = tab + (long)blockIdx.x * AF_FIELDS;
  const long c_off = r[AF_C];
  if (c_off < 0) return;
  if (hyper != nullptr) b2t = hyper[1];
  const long rows = r[AF_ROWS], cols = r[AF_COLS], nchunk = r[AF_NCHUNK];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (blockIdx.y == 0) {
    float* R = rv + r[AF_RV];
    const float* rp = rowpart + r[AF_ROWPART];
    float acc = 0.f;
    for (long i = tid; i < rows; i += 256) {
      float s = 0.f;
      for (long k = 0; k < nchunk; ++k) s += rp[i * nchunk + k];
      const float v = b2t * R[i] + (1.f - b2t) * (s / (float)cols);
      R[i] = v;
      acc += v;
    }
    acc = block_sum<256>(acc, red);
    if (tid == 0) scal[r[AF_SCAL] * 4 + 0] = acc / (float)rows;
  }
  float* C = cst + c_off;
  const float* cp = colpart + r[AF_COLPART];
  const long nrb = (rows + AF_RB - 1) / AF_RB;
  const int cl = tid & (AF_FIN_COLS - 1);
  const int sl = (lane >> 4) + 4 * w;  // 0 .. AF_FIN_SLICES - 1
  for (long cg = blockIdx.y; cg * AF_FIN_COLS < cols; cg += AF_FIN_Y) {
    const long c = cg * AF_FIN_COLS + cl;
    float a = 0.f;
    if (c < cols)
      for (long rb = sl; rb < nrb; rb += AF_FIN_SLICES) a += cp[rb * cols + c];
    a += __shfl_xor(a, 16, 64);
    a += __shfl_xor(a, 32, 64);
    __syncthreads();
    if (lane < AF_FIN_COLS) lcol[w][lane] = a;
    __syncthreads();
    if (tid < AF_FIN_COLS && c < cols) {
      const float s = ((lcol[0][tid] + lcol[1][tid]) + lcol[2][tid]) + lcol[3][tid];
      C[c] = b2t * C[c] + (1.f - b2t) * (s / (float)rows);
    }
  }
}

// ------------------------------------------------------------------------------- passes 2 and 3: sum u^2, and update
// UPDATE false: sum of u^2 (and of w^2 when SP) of the tile -> tpart[tile], tpart[n_tiles + tile].
// UPDATE true:  w -= dec w; w -= step u.
template <bool VEC, bool UPDATE, bool SP, typename TP, bool MASTER>
DLLM_DEVICE void u_tile(const Tile& t, long tile, long n_tiles, TP* __restrict__ param, float* __restrict__ master,
                        const float* __restrict__ grad, float coef, const float* __restrict__ rv,
                        const float* __restrict__ cst, const float* __restrict__ scal, float* __restrict__ tpart,
                        float* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long cbase = t.chunk * AF_CC + (long)w * AF_WC;
  const bool factored = t.c >= 0;
  float cf[4];
  ld4<VEC>(factored ? cst + t.c : rv + t.rv, cbase, lane, t.cols, true, cf);
#pragma unroll
  for (int k = 0; k < 4; ++k) cf[k] = colk<VEC>(cbase, lane, k) < t.cols ? rsqrtf(cf[k]) * coef : 0.f;
  const float mean_r = factored ? scal[t.u * 4 + 0] : 1.f;
  float step = 0.f, dec = 0.f;
  if constexpr (UPDATE) {
    step = scal[t.u * 4 + 1];
    dec = scal[t.u * 4 + 2];
  }
  float acc = 0.f, wacc = 0.f;
  const long row0 = t.off + t.r0 * t.cols;
  for (int r = 0; r < t.nr; r += 4) {
    float g[4][4], wv[4][4], rf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = r + i < t.nr;
      const long ro = row0 + (ok ? (long)(r + i) * t.cols : 0);
      ld4<VEC>(grad + ro, cbase, lane, t.cols, ok, g[i]);
      if constexpr (UPDATE || SP) {
        if constexpr (MASTER) ld4<VEC>(master + ro, cbase, lane, t.cols, ok, wv[i]);
        else ld4<VEC>(param + ro, cbase, lane, t.cols, ok, wv[i]);
      }
      rf[i] = (factored && ok) ? rsqrtf(rv[t.rv + t.r0 + r + i] / mean_r) : 1.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (!UPDATE) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float u = g[i][k] * (rf[i] * cf[k]);
          acc += u * u;
          if constexpr (SP) wacc += wv[i][k] * wv[i][k];
        }
      } else {
        if (r + i < t.nr) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float u = g[i][k] * (rf[i] * cf[k]);
            const float x = fmaf(-dec, wv[i][k], wv[i][k]);  // one rounding each: w - dec w, then - step u
            wv[i][k] = fmaf(-step, u, x);
          }
          const long ro = row0 + (long)(r + i) * t.cols;
          if constexpr (MASTER) st4<VEC>(master + ro, cbase, lane, t.cols, wv[i]);
          st4<VEC>(param + ro, cbase, lane, t.cols, wv[i]);
        }
      }
    }
  }
  if constexpr (!UPDATE) {
    acc = block_sum<256>(acc, red);
    if constexpr (SP) wacc = block_sum<256>(wacc, red);
    if (threadIdx.x == 0) {
      tpart[tile] = acc;
      if constexpr (SP) tpart[n_tiles + tile] = wacc;
    }
  }
}

template <bool UPDATE, bool SP, typename TP, bool MASTER>
__global__ __launch_bounds__(256) void af_u(TP* __restrict__ param, float* __restrict__ master,
                                            const float* __restrict__ grad, const long* __restrict__ tab, int U,
                                            long n_tiles, const float* __restrict__ coef_p,
                                            const float* __restrict__ rv, const float* __restrict__ cst,
                                            const float* __restrict__ scal, float* __restrict__ tpart) {
  __shared__ float red[4];
  const float coef = coef_p[0];
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const Tile t = decode_tile(tab, U, tile);
    if (t.vec) u_tile<true, UPDATE, SP, TP, MASTER>(t, tile, n_tiles, param, master, grad, coef, rv, cst, scal, tpart, red);
    else u_tile<false, UPDATE, SP, TP, MASTER>(t, tile, n_tiles, param, master, grad, coef, rv, cst, scal, tpart, red);
  }
}

// one workgroup per unit: its tiles' partial sums in a fixed order -> the unit's step size and decay factor
__global__ __launch_bounds__(256) void af_fin_clip(const long* __restrict__ tab, long n_tiles,
                                                   const float* __restrict__ tpart, float rel,
                                                   const float* __restrict__ hyper, float eps2, float clip_thr, float wd,
                                                   int sp, float* __restrict__ scal) {
  __shared__ float red[4];
  const long* r = tab + (long)blockIdx.x * AF_FIELDS;
  const long t0 = r[AF_TILE0], t1 = r[AF_FIELDS + AF_TILE0];
  if (hyper != nullptr) rel = hyper[0];
  float su = 0.f, sw = 0.f;
  for (long i = t0 + threadIdx.x; i < t1; i += 256) {
    su += tpart[i];
    if (sp) sw += tpart[n_tiles + i];
  }
  su = block_sum<256>(su, red);
  sw = block_sum<256>(sw, red);
  if (threadIdx.x == 0) {
    const float numel = (float)(r[AF_ROWS] * r[AF_COLS]);
    const float lr_t = sp ? rel * fmaxf(eps2, sqrtf(sw / numel)) : rel;
    const float div = fmaxf(1.f, sqrtf(su / numel) / clip_thr);
    float* s = scal + r[AF_SCAL] * 4;
    s[1] = lr_t / div;
    s[2] = r[AF_DECAY] ? wd * lr_t : 0.f;
  }
}

}  // namespace

// One Adafactor step over every unit of `tab` ([U + 1, AF_FIELDS] int64 on the device, planned and bounds-checked by
// csrc/bind_optim.cpp).  `tpart` holds 2 * n_tiles floats, `scal` 4 * U.  is_bf16: bf16 parameters with an fp32 master; else
// fp32 parameters updated in place (master == nullptr).
extern "C" int dllm_adafactor_step(void* param, float* master, const float* grad, float* rv, float* cst,
                                   const long* tab, int U, long n_tiles, float* scal, float* colpart, float* rowpart,
                                   float* tpart, const float* coef, float rel, float b2t, float eps1, float eps2,
                                   float clip_thr, float wd, int scale_param, int is_bf16, const float* hyper,
                                   hipStream_t st) {
  if (U <= 0 || n_tiles <= 0) return -2;
  if ((is_bf16 != 0) != (master != nullptr)) return -3;
  const int G = (int)(n_tiles < AF_GRID_CAP ? n_tiles : AF_GRID_CAP);
  hipLaunchKernelGGL(af_stats, dim3(G), dim3(256), 0, st, grad, tab, U, n_tiles, coef, eps1, b2t, hyper, rv, colpart,
                     rowpart);
  hipLaunchKernelGGL(af_fin_stats, dim3(U, AF_FIN_Y), dim3(256), 0, st, tab, b2t, hyper, rv, cst, colpart, rowpart,
                     scal);
#define AF_U(UPD, SP)                                                                                                  \
  do {                                                                                                                 \
    if (is_bf16)                                                                                                       \
      hipLaunchKernelGGL((af_u<UPD, SP, uint16_t, true>), dim3(G), dim3(256), 0, st, (uint16_t*)param, master, grad,   \
                         tab, U, n_tiles, coef, rv, cst, scal, tpart);                                                 \
    else                                                                                                               \
      hipLaunchKernelGGL((af_u<UPD, SP, float, false>), dim3(G), dim3(256), 0, st, (float*)param, master, grad, tab,   \
                         U, n_tiles, coef, rv, cst, scal, tpart);                                                      \
  } while (0)
  if (scale_param) AF_U(false, true); else AF_U(false, false);
  hipLaunchKernelGGL(af_fin_clip, dim3(U), dim3(256), 0, st, tab, n_tiles, tpart, rel, hyper, eps2, clip_thr, wd,
                     scale_param, scal);
  AF_U(true, false);
#undef AF_U
  DLLM_CHECK_LAUNCH();
  return 0;
}
