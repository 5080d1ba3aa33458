// One sampling step on the LM-head logits, for gfx950 (models/generation.py _sample_step).
//
// transformers' sampling runs, per decode step, the repetition penalty, the logits processors, temperature, top-k (a
// top-k over [rows, V]) and top-p (a full sort of [rows, V], softmax, cumsum, scatter back), then a multinomial draw:
// ~20 launches and a sort.  Here one workgroup per row does it in one launch, re-reading the row (64 .. 1000 KB, L2
// resident) once per pass and never sorting:
//
//   * seen-token and ban bitmaps over the vocabulary in LDS, built from the row's decoder prefix (the n-gram bans as
//     csrc/beam.hip builds them); score(c) = logit -> penalty -> ban (-inf) -> / temperature is recomputed per pass;
//   * top-k threshold: radix select on an order-preserving 32-bit key of the score, 8 bits per pass, COUNT histograms;
//     ties with the k-th value survive.  The walk over the row is bound by VALU work per token (one CU per row), so
//     the row is cut coarsely first, on the keys BEFORE the temperature (no division per token): as soon as a radix
//     level leaves at most LIST_CAP candidates they are compacted into a small list, and the exact select and every
//     later pass walk the list instead of the row (2 - 3 passes over the row at top_k = 50, not 5+);
//   * top-p threshold: the same descent with MASS histograms (exp(x - max) per bin) over the survivors: the threshold
//     is the smallest value whose strictly-larger mass is < top_p * total (tied scores are kept or dropped together,
//     the maximum always stays);
//   * draw: Gumbel-max over x >= threshold with the counter-based uniforms of ops/rng.py sample_uniform; ties resolve
//     to the lower index.
//
// Histograms are replicated per lane (up to 32 copies, bin-major) so that the lanes of a wave that hit the same bin —
// the top byte of a float key takes a handful of values — land in different LDS banks instead of serialising.
// A forced token (BOS at step 1, EOS at the last step) is returned as it is.
#include "common.h"

using namespace dllm;

namespace {

constexpr int NT = 1024, NW = NT / 64, LIST_CAP = 4096;

struct SampleParams {
  const void* logits;  // [rows, V] with leading dimension ld (bf16 or fp32)
  long ld;
  const int64_t* seqs;  // [rows, lds] decoder prefix (positions 0 .. cur-1)
  long lds;
  int cur, ngram, ban_tok, force_tok, V, rows, top_k, copies;
  float penalty, temperature, top_p;
  uint32_t seed, step;
  int64_t* tok;   // [rows]
  float* thr;     // [rows, 2]: the top-k threshold (-inf: off) and the final threshold (kept: x >= it and x > -inf)
  float* list_v;  // [rows, LIST_CAP] workspace: survivors of top-k
  int* list_i;
};

template <typename T>
DLLM_DEVICE float ld1(const T* p, long i);
template <>
DLLM_DEVICE float ld1<float>(const float* p, long i) { return p[i]; }
template <>
DLLM_DEVICE float ld1<uint16_t>(const uint16_t* p, long i) { return bf2f(p[i]); }

// order-preserving key of a float (ascending), and back
DLLM_DEVICE uint32_t fkey(float x) {
  const uint32_t b = __float_as_uint(x);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
DLLM_DEVICE float fkey_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k); }

DLLM_DEVICE bool better(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

// f(raw logit, token, seen word, ban word) over the row: 16-B loads (8 bf16 / 4 fp32 per lane) when the row is 16-B
// aligned, the bitmap words read once per load (a load never straddles a 32-token word)
template <typename T, class F>
DLLM_DEVICE void row_each(const T* x, int V, int tid, const uint32_t* seen, const uint32_t* ban, bool pen, bool bans,
                          F f) {
  constexpr int VW = sizeof(T) == 2 ? 8 : 4;
  const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const int vend = vec ? V / VW * VW : 0;
  constexpr int U = 4;  // loads in flight per lane: one per trip leaves the walk bound by the load latency
  for (int cb = tid * VW; cb < vend; cb += NT * VW * U) {
    u32x4 raw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c0 = cb + u * NT * VW;
      if (c0 < vend) raw[u] = *reinterpret_cast<const u32x4*>(x + c0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c0 = cb + u * NT * VW;
      if (c0 >= vend) break;
      const uint32_t sw = pen ? seen[c0 >> 5] : 0u, bw = bans ? ban[c0 >> 5] : 0u;
      if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          f(bf2f((uint16_t)(raw[u][e] & 0xFFFFu)), c0 + 2 * e, sw, bw);
          f(bf2f((uint16_t)(raw[u][e] >> 16)), c0 + 2 * e + 1, sw, bw);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) f(__uint_as_float(raw[u][e]), c0 + e, sw, bw);
      }
    }
  }
  for (int c = vend + tid; c < V; c += NT) f(ld1<T>(x, c), c, pen ? seen[c >> 5] : 0u, bans ? ban[c >> 5] : 0u);
}

// sum the histogram's copies into tot[256]; thread t: bin t / 4, every 4th copy from t % 4
template <bool MASS>
DLLM_DEVICE void reduce_hist(const uint32_t* hist, uint32_t* tot, int C, int tid) {
  __syncthreads();
  const int bin = tid >> 2, q = tid & 3;
  if constexpr (MASS) {
    float s = 0.f;
    for (int i = q; i < C; i += 4) s += __uint_as_float(hist[bin * C + i]);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if (q == 0) tot[bin] = __float_as_uint(s);
  } else {
    uint32_t s = 0u;
    for (int i = q; i < C; i += 4) s += hist[bin * C + i];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if (q == 0) tot[bin] = s;
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(NT) void sample_step_kernel(SampleParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float red_v[NW];
  __shared__ int red_i[NW];
  __shared__ uint32_t sh_bin, sh_krem, sh_cnt, sh_n;
  __shared__ float sh_above, sh_total;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int row = blockIdx.x, V = P.V, nwords = (V + 31) >> 5, C = P.copies;
  if (P.force_tok >= 0) {  // forced token: after the bans, as transformers' ForcedBOS / ForcedEOS processors
    if (tid == 0) {
      P.tok[row] = P.force_tok;
      P.thr[2 * row] = -INFINITY;
      P.thr[2 * row + 1] = 0.f;
    }
    return;
  }
  uint32_t* seen = reinterpret_cast<uint32_t*>(smem);  // [nwords] tokens of the prefix
  uint32_t* ban = seen + nwords;                       // [nwords] banned tokens
  uint32_t* hist = ban + nwords;                       // [256 * C], bin-major
  uint32_t* tot = hist + 256 * C;                      // [256]
  const float r = P.penalty, Tm = P.temperature;
  const bool pen = r != 1.f, bans = P.ngram > 0 || P.ban_tok >= 0, useT = Tm != 1.f;
  const bool topk = P.top_k > 0 && P.top_k < V, topp = P.top_p < 1.f;
  const int64_t* s = P.seqs + (long)row * P.lds;

  // ---- bitmaps of this row
  if (pen || bans) {
    for (int i = tid; i < 2 * nwords; i += NT) seen[i] = 0u;
    __syncthreads();
    if (pen)
      for (int i = tid; i < P.cur; i += NT) {
        const int64_t t = s[i];
        if (t >= 0 && t < V) atomicOr(&seen[t >> 5], 1u << (t & 31));
      }
    if (tid == 0 && P.ban_tok >= 0 && P.ban_tok < V) atomicOr(&ban[P.ban_tok >> 5], 1u << (P.ban_tok & 31));
    const int n = P.ngram;
    if (n > 0 && P.cur >= n) {
      for (int i = tid; i <= P.cur - n; i += NT) {  // window i: tokens i .. i+n-1; prefix = last n-1 generated
        bool match = true;
        for (int q = 0; q < n - 1; ++q) match = match && s[i + q] == s[P.cur - n + 1 + q];
        const int64_t t = s[i + n - 1];
        if (match && t >= 0 && t < V) atomicOr(&ban[t >> 5], 1u << (t & 31));
      }
    }
    __syncthreads();
  }
  const T* x = reinterpret_cast<const T*>(P.logits) + (long)row * P.ld;
  // score = fin(pre(logit)): penalty and bans, then temperature (x / T: a division, as the composite's)
  auto pre = [&](float v, int c, uint32_t sw, uint32_t bw) -> float {
    if ((sw >> (c & 31)) & 1u) v = v < 0.f ? v * r : v / r;
    return ((bw >> (c & 31)) & 1u) ? -INFINITY : v;
  };
  auto fin = [&](float v) -> float {
    if (useT) v = v / Tm;
    return v == 0.f ? 0.f : v;  // -0 and +0 compare equal: one key
  };
  auto zero_hist = [&]() {
    __syncthreads();
    for (int i = tid; i < 256 * C; i += NT) hist[i] = 0u;
    __syncthreads();
  };
  const int copy = lane & (C - 1);
  float* lv = P.list_v + (long)row * LIST_CAP;
  int* li = P.list_i + (long)row * LIST_CAP;
  float m = -INFINITY;  // per-thread maximum of the scores
  uint32_t floor_key = 0u;
  bool use_list = false;
  int n_list = 0;
  // f(score, token) over the whole row / over the list
  auto row_x = [&](auto f) {
    row_each<T>(x, V, tid, seen, ban, pen, bans,
                [&](float v, int c, uint32_t sw, uint32_t bw) { f(fin(pre(v, c, sw, bw)), c); });
  };
  auto list_x = [&](auto f) {
    for (int i = tid; i < n_list; i += NT) f(lv[i], li[i]);
  };
  // wave 0, lane l: bins 4l .. 4l+3 of tot; the bin holding the krem-th largest -> sh_bin, sh_krem, sh_cnt
  auto select_count = [&](uint32_t krem) {
    if (tid < 64) {
      uint32_t v[4], lt = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = tot[4 * lane + j];
        lt += v[j];
      }
      uint32_t sfx = lt;  // inclusive suffix sum over lanes
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_down(sfx, o, 64);
        if (lane + o < 64) sfx += t;
      }
      uint32_t excl = sfx - lt;  // count in bins above this lane's
#pragma unroll
      for (int j = 3; j >= 0; --j) {
        const uint32_t incl = excl + v[j];
        if (incl >= krem && excl < krem) {
          sh_bin = 4 * lane + j;
          sh_krem = krem - excl;
          sh_cnt = v[j];
        }
        excl = incl;
      }
    }
    __syncthreads();
  };
  // radix select of the top_k-th largest key over a source, COUNT histograms: floor_key; returns the survivors
  auto radix_count = [&](auto src) -> uint32_t {
    uint32_t prefix = 0u, krem = (uint32_t)P.top_k;
    for (int L = 0; L < 4; ++L) {
      const int shift = 24 - 8 * L;
      zero_hist();
      src([&](float sc, int) {
        const uint32_t key = fkey(sc);
        if (L == 0) {
          m = fmaxf(m, sc);
          atomicAdd(&hist[(key >> 24) * C + copy], 1u);
        } else if ((key >> (shift + 8)) == prefix) {
          atomicAdd(&hist[((key >> shift) & 255u) * C + copy], 1u);
        }
      });
      reduce_hist<false>(hist, tot, C, tid);
      select_count(krem);
      prefix = (prefix << 8) | sh_bin;
      krem = sh_krem;
    }
    floor_key = prefix;
    return (uint32_t)P.top_k - krem + sh_cnt;  // above the k-th value + its ties
  };

  // ---- top-k
  if (topk) {
    // coarse cut on the scores before the temperature (no division per token): radix levels on their keys until few
    // enough tokens lie at or above the bin that holds the k-th largest.  x / T is monotone, so every survivor of
    // top-k lies there, or within rounding below the bin's edge (16 ulps taken): those tokens go to the list and the
    // exact select runs on the list
    uint32_t prefix = 0u, krem = (uint32_t)P.top_k;
    for (int L = 0; L < 4 && !use_list; ++L) {
      const int shift = 24 - 8 * L;
      zero_hist();
      row_each<T>(x, V, tid, seen, ban, pen, bans, [&](float v, int c, uint32_t sw, uint32_t bw) {
        const uint32_t key = fkey(pre(v, c, sw, bw));
        if (L == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[((key >> shift) & 255u) * C + copy], 1u);
      });
      reduce_hist<false>(hist, tot, C, tid);
      select_count(krem);
      prefix = (prefix << 8) | sh_bin;
      krem = sh_krem;
      const uint32_t cge = (uint32_t)P.top_k - krem + sh_cnt, lo = prefix << shift;
      if (lo < 0x01000000u || cge > (uint32_t)(LIST_CAP - 64)) continue;  // top byte 0 holds -inf: the banned tokens
      if (tid == 0) sh_n = 0u;
      __syncthreads();
      row_each<T>(x, V, tid, seen, ban, pen, bans, [&](float v, int c, uint32_t sw, uint32_t bw) {
        const float y = pre(v, c, sw, bw);
        if (fkey(y) >= lo - 16u) {
          const uint32_t pos = atomicAdd(&sh_n, 1u);
          if (pos < (uint32_t)LIST_CAP) {
            lv[pos] = fin(y);
            li[pos] = c;
          }
        }
      });
      __threadfence_block();
      __syncthreads();
      if (sh_n <= (uint32_t)LIST_CAP) {
        n_list = (int)sh_n;
        use_list = true;
      }
    }
    if (use_list) {
      radix_count(list_x);
    } else if (radix_count(row_x) <= (uint32_t)LIST_CAP) {  // compact the survivors: every later pass walks the list
      if (tid == 0) sh_n = 0u;
      __syncthreads();
      row_x([&](float sc, int c) {
        if (sc != -INFINITY && fkey(sc) >= floor_key) {
          const uint32_t pos = atomicAdd(&sh_n, 1u);
          if (pos < (uint32_t)LIST_CAP) {
            lv[pos] = sc;
            li[pos] = c;
          }
        }
      });
      __threadfence_block();
      __syncthreads();
      n_list = (int)min(sh_n, (uint32_t)LIST_CAP);
      use_list = true;
    }
  } else if (topp) {
    row_x([&](float sc, int) { m = fmaxf(m, sc); });
  }
  // f(score, token) over the survivors of top-k (never a banned token)
  auto each = [&](auto f) {
    auto g = [&](float sc, int c) {
      if (sc != -INFINITY && fkey(sc) >= floor_key) f(sc, c);
    };
    if (use_list) list_x(g);
    else row_x(g);
  };

  // ---- top-p: the same descent with MASS histograms: the smallest value whose strictly-larger mass is < top_p * total
  uint32_t thr_key = floor_key;
  if (topp) {
    const float M = block_max<NT>(m, red_v);
    uint32_t prefix = 0u;
    float above = 0.f, pS = 0.f;
    float* histf = reinterpret_cast<float*>(hist);
    for (int L = 0; L < 4; ++L) {
      const int shift = 24 - 8 * L;
      zero_hist();
      each([&](float sc, int) {
        const uint32_t key = fkey(sc);
        if (L == 0 || (key >> (shift + 8)) == prefix)  // FLT_MIN: a bin with a token in it never reads as empty
          atomicAdd(&histf[((key >> shift) & 255u) * C + copy], fmaxf(expf(sc - M), 1.17549435e-38f));
      });
      reduce_hist<true>(hist, tot, C, tid);
      if (tid < 64) {
        float v[4], lt = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = __uint_as_float(tot[4 * lane + j]);
          lt += v[j];
        }
        float sfx = lt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const float t = __shfl_down(sfx, o, 64);
          if (lane + o < 64) sfx += t;
        }
        if (L == 0) pS = P.top_p * __shfl(sfx, 0, 64);
        float excl = __shfl_down(sfx, 1, 64);  // mass in bins above this lane's
        if (lane == 63) excl = 0.f;
        int found = -1, top = -1;  // lowest kept bin of this lane; its highest non-empty bin
        float fex = 0.f, tex = 0.f;
#pragma unroll
        for (int j = 3; j >= 0; --j) {
          if (v[j] > 0.f) {
            if (top < 0) {
              top = 4 * lane + j;
              tex = excl;
            }
            if (above + excl < pS) {
              found = 4 * lane + j;
              fex = excl;
            }
          }
          excl += v[j];
        }
        const uint64_t ok = __ballot(found >= 0), any = __ballot(top >= 0);
        if (ok) {
          if (lane == __ffsll((unsigned long long)ok) - 1) {
            sh_bin = (uint32_t)found;
            sh_above = above + fex;
          }
        } else if (any) {  // rounding left no bin below the bound: the highest non-empty one (the maximum stays)
          if (lane == 63 - __clzll((unsigned long long)any)) {
            sh_bin = (uint32_t)top;
            sh_above = above + tex;
          }
        } else if (lane == 0) {  // nothing to draw from: every token is banned
          sh_bin = 0u;
          sh_above = above;
        }
        if (lane == 0) sh_total = pS;
      }
      __syncthreads();
      prefix = (prefix << 8) | sh_bin;
      above = sh_above;
      pS = sh_total;
    }
    thr_key = prefix > floor_key ? prefix : floor_key;
  }

  // ---- draw: Gumbel-max over the kept tokens, u from (seed, step, row, token)
  const uint32_t row_key = mix32(P.seed, P.step * (uint32_t)P.rows + (uint32_t)row);
  float bv = -INFINITY;
  int bi = 0x7FFFFFFF;
  each([&](float sc, int c) {
    if (fkey(sc) < thr_key) return;
    const uint32_t n = mix32(row_key, (uint32_t)c) >> 8;
    // t = -log(u), u = (n + 0.5) * 2^-24: above 1/2 through 1 - u, which fp32 holds exactly there (u itself rounds)
    const float t = n < (1u << 23) ? -logf(((float)n + 0.5f) * 5.9604644775390625e-8f)
                                   : -log1pf(-(((float)(16777216u - n) - 0.5f) * 5.9604644775390625e-8f));
    const float g = sc - logf(t);
    if (better(g, c, bv, bi)) {
      bv = g;
      bi = c;
    }
  });
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float v2 = __shfl_xor(bv, o, 64);
    const int i2 = __shfl_xor(bi, o, 64);
    if (better(v2, i2, bv, bi)) {
      bv = v2;
      bi = i2;
    }
  }
  __syncthreads();
  if (lane == 0) {
    red_v[w] = bv;
    red_i[w] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int q = 1; q < NW; ++q)
      if (better(red_v[q], red_i[q], bv, bi)) {
        bv = red_v[q];
        bi = red_i[q];
      }
    P.tok[row] = bi == 0x7FFFFFFF ? 0 : bi;
    P.thr[2 * row] = topk ? fkey_inv(floor_key) : -INFINITY;
    P.thr[2 * row + 1] = (topk || topp) ? fkey_inv(thr_key) : -INFINITY;
  }
}

template <typename T>
int launch(const SampleParams& p, size_t lds, hipStream_t st) {
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_step_kernel<T>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL((sample_step_kernel<T>), dim3(p.rows), dim3(NT), lds, st, p);
  DLLM_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// rows of the survivor workspace the caller allocates (list_v, list_i: [rows, this])
extern "C" int dllm_sample_list_cap() { return LIST_CAP; }

// returns -4 on unsupported arguments (V too large for the LDS bitmaps, options out of range)
extern "C" int dllm_sample_step(const void* logits, long ld, int is_bf16, const int64_t* seqs, long lds, int cur,
                                int ngram, int ban_tok, int force_tok, int rows, int V, float penalty,
                                float temperature, int top_k, float top_p, uint32_t seed, uint32_t step, int64_t* tok,
                                float* thr, float* list_v, int* list_i, hipStream_t st) {
  if (rows <= 0 || V <= 0 || cur < 0 || ngram < 0 || ban_tok >= V || force_tok >= V || !(penalty > 0.f) ||
      !(temperature > 0.f) || !(top_p > 0.f) || top_k < 0)
    return -4;
  static int lim = 0;  // LDS a workgroup may take (one device model per process)
  if (lim == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v <= 0)
      return -4;
    lim = v;
  }
  const size_t fixed = (size_t)((V + 31) / 32) * 8 + 256 * 4 + 256;  // bitmaps, totals, the kernel's static LDS
  int copies = 32;
  while (copies >= 1 && fixed + (size_t)copies * 1024 > (size_t)lim) copies >>= 1;
  if (copies < 1) return -4;
  SampleParams p{logits, ld,      seqs,        lds,   cur,  ngram, ban_tok, force_tok, V,      rows,  top_k,
                 copies, penalty, temperature, top_p, seed, step,  tok,     thr,       list_v, list_i};
  const size_t bytes = fixed - 256 + (size_t)copies * 1024;
  return is_bf16 ? launch<uint16_t>(p, bytes, st) : launch<float>(p, bytes, st);
}
