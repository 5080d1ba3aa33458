// Split-key flash-decoding attention for generate(): bf16 forward for the few query rows of a decode step against a
// long K/V — decoder self-attention on the cache (Sq = 1) and cross-attention on the encoder's K/V, shared by the nb
// beams of a batch entry (Sq = nb).  Contract: csrc/attn_params.h AttnDecodeParams.  The training forward kernels
// serve such a call with a 64- or 128-row query tile that holds 1 .. nb real rows and B * H workgroups that each walk
// every key alone; here the query rows are one MFMA tile and the key axis is split over workgroups.
//
//   rows     The R = Sq * G <= 16 query rows that read one K/V head (G = H / Hkv query heads per K/V head) are packed
//            as r = i * G + g into ONE 16-row tile, zero-padded: a K/V head is read once for its whole group and for
//            every beam, never repeated.
//   grid     (splits, Hkv, B), 256 threads.  Split s covers the keys [s L, min((s + 1) L, Sk)), L % 128 == 0.  Inside a
//            split wave w owns the 32-key steps w, w + 4, ...: each wave runs its own online softmax and keeps its own
//            (m, l, O^T), so the main loop has no workgroup barrier.
//   scores   S^T[16 keys][16 rows] = K Q^T on v_mfma_f32_16x16x32_bf16 (attn_mfma16.h): the K fragment of a lane is 8
//            consecutive head-dim elements of one key row, a plain 16-B global load straight into the A operand — K
//            never touches LDS.  Q^T is loaded once into registers as the B operand.
//   P V      the two 16-key accumulator tiles of a step pack (pack8) into the B operand of O^T[D][16 rows] += V^T P^T.
//            Only V goes through LDS: each wave stages its 32 x DP slab in a region of its own and reads it back
//            transposed (ds_read_b64_tr_b16, ld_tr2).  Same-wave LDS traffic is ordered, so no barrier.
//   overlap  the next step's K fragments are requested as soon as the score MFMAs have consumed the current ones (the
//            same registers), the next V slab and the next step's mask bytes / bias values go to registers at the same
//            point: all of them are in flight under the softmax and the P V product, and V reaches LDS at the top of
//            the next step.  The double buffer is the register copy; the LDS slab is single (the issue's design has two
//            slabs; with V passing through registers anyway the second one bought nothing and halves the workgroups
//            per CU at DP = 256).
//   masks    kpm and the bias LUT are read per key by the lane that holds the score (8 keys per lane and step): no
//            (row, key) LDS table.  Sequence length lives neither in LDS nor in registers: any Sk.
//   merge    the four waves merge (m, l, O^T) through LDS (the V slabs, reused).  With splits == 1 the workgroup
//            writes bf16 o; otherwise an unnormalised fp32 partial (m, l, O[R][D]) that attn_decode_merge_kernel
//            reduces over the splits in split order — no atomics, reruns are bit-identical.  A wave or split without
//            a visible key is (m = -inf, l = 0) and weighs exp2(-inf - mu) = 0 with mu = 0 when every m is -inf.
//
//   FP8      K/V as OCP e4m3fn codes with one fp32 scale per (batch entry, key, K/V head) (attn_params.h; template
//            parameter FP8, instantiations of their own): the same grid, row packing, softmax and merges on half the
//            bytes.  K: a lane loads 16 consecutive codes (16 B) of its key row straight into registers and widens them
//            to two bf16 A fragments there (v_cvt_pk_f32_fp8, then the high halves packed by v_perm: a code is exact in
//            bf16); the contraction order is free, so fragment 2 l + h holds the head-dim columns 64 l + 16 g + 8 h ..
//            + 7 and Q^T is loaded with the same permutation.  k_scale joins the score in fp32 where the lane holds
//            it (st * (scale2 * ks[key])), next to the mask byte and the bias.  V: 16-code chunks pass through half
//            the registers and are widened on the way into the slab, whose layout and transposed reads are those of
//            bf16 (ds_read_b64_tr_b16 kept: a slab of codes read by ds_read_b64_tr_b8 would feed an fp8 MFMA, and the
//            P operand would have to be rounded to fp8); v_scale multiplies P in fp32 ahead of pack8.
//   quantise attn_kv_quant_kernel writes that row format: D / 8 lanes of a row load 16 B each, the row max is a
//            shuffle reduction inside the lane group, the codes are v_cvt_pk_fp8_f32 of x / scale (a correctly rounded
//            fp32 divide, clamped to +-448): bit-equal to the torch composite of ops/attention.py quantize_kv.
//
// exp2 softmax with log2(e) folded into the scale; the cap is tanh_ex2, before the mask (template parameter CAP).
// Plain C++ and vector stores only.
#include <algorithm>

#include "common.h"
#include "attn_params.h"
#include "attn_small.h"
#include "attn_mfma16.h"

using namespace dllm;

namespace {

constexpr int STEP = 32;        // keys of one wave step: two 16-key MFMA tiles
constexpr int SPLIT_ALIGN = 128;  // 4 waves x STEP
// split choice (dllm_attn_decode_plan), from the sweep of tools/attn_decode_bench.py in profiles/attn_decode.txt
constexpr int FILL_PER_CU = 1;           // workgroups per CU to aim for
constexpr int SPLIT_FLOOR_BYTES = 65536;  // no split shorter than this many bytes of K: keys x padded head dim x
                                          // element size
// FP8 K/V, from the sweep in profiles/attn_decode_fp8.txt: half the bytes per step are in flight, so the FP8 kernels
// are fastest with every workgroup slot of a CU taken (3 / 2 / 1 at the padded head dims 64 / 128 / 256) and with
// bf16's floor in keys, which is half its bytes
constexpr int SPLIT_FLOOR_BYTES_FP8 = 32768;
constexpr int fill_per_cu_fp8(int dp) { return dp == 64 ? 3 : dp == 128 ? 2 : 1; }

// ordering of the wave's own LDS writes and (transposed) reads: nothing is emitted, the compiler keeps the order
DLLM_DEVICE void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// 8 e4m3fn codes (two dwords, ascending bytes) as 8 bf16: the fp32 value of a code has at most 4 significant bits, so
// its high half is the bf16 of the same value
DLLM_DEVICE uint32_t widen2(uint32_t w, bool hi) {
  const f32x2 f = hi ? __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true) : __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  return __builtin_amdgcn_perm(__float_as_uint(f.y), __float_as_uint(f.x), 0x07060302u);  // (x >> 16) | (y & ~0xFFFF)
}
DLLM_DEVICE u32x4 widen8(uint32_t lo, uint32_t hi) {
  return u32x4{widen2(lo, false), widen2(lo, true), widen2(hi, false), widen2(hi, true)};
}

template <int DP, bool CAP, bool FP8>
__global__ __launch_bounds__(NT) void attn_decode_kernel(AttnDecodeParams P) {
  constexpr int KS = DP / 32, DT = DP / 16, LD = Img<DP>::LD, CPR = Img<DP>::CPR, VPL = DP / 16;
  constexpr int KL = DP / 64;                 // FP8: 16-code loads of a lane per key row, two K fragments each
  constexpr int CPR8 = DP / 16, VPL8 = DP / 32;  // FP8: 16-code chunks per V row, and per lane and step
  constexpr int SLAB = STEP * LD;  // bf16 elements of a wave's V slab; as floats 16 DP + 128 >= the merge's 16 DP + 32
  __shared__ __attribute__((aligned(16))) uint16_t Vs[4 * SLAB];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int s = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int G = P.G, R = P.Sq * G;
  const bool row_ok = c < R;
  const int qi = row_ok ? c / G : 0, hq = hk * G + (row_ok ? c % G : 0);  // the lane's query index and query head

  bf16x8v qf[KS];
  const uint16_t* qrow = P.q + (long)b * P.q_sb + (long)qi * P.q_ss + (long)hq * P.q_sh;
  if constexpr (FP8) {  // the K fragments' column order: fragment 2 l + h = columns 64 l + 16 g + 8 h .. + 7
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int d0 = 64 * (ks >> 1) + 16 * g + 8 * (ks & 1);
      u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (d0 < P.D) v = *reinterpret_cast<const u16x8*>(qrow + d0);
      qf[ks] = __builtin_bit_cast(bf16x8v, v);
    }
  } else {
    load_row_frags<DP>(qrow, g, P.D, qf);
  }
  if (!row_ok) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = __builtin_bit_cast(bf16x8v, u16x8{0, 0, 0, 0, 0, 0, 0, 0});
  }
  const float scale2 = P.scale * LOG2E;
  const float capz2 = CAP ? P.scale / P.softcap * (2.f * LOG2E) : 0.f;
  const float capc2 = CAP ? P.softcap * LOG2E : 0.f;

  const int kbeg = s * P.L, kend = min(kbeg + P.L, P.Sk);
  const uint16_t* kb = P.k + (long)b * P.k_sb + (long)hk * P.k_sh;
  const uint16_t* vb = P.v + (long)b * P.v_sb + (long)hk * P.v_sh;
  const uint8_t* kpm = P.kpm ? P.kpm + (long)b * P.Sk : nullptr;
  // bias of (row, key j): lutp[j]
  const float* lutp = P.lut && row_ok ? P.lut + (long)hq * ((long)P.Sq + P.Sk - 1) + (P.Sq - 1 - qi) : nullptr;
  uint16_t* slab = Vs + w * SLAB;
  // FP8: the code bytes (strides in bytes) and the scales of the (batch entry, K/V head)
  const uint8_t* kb8 = reinterpret_cast<const uint8_t*>(P.k) + (long)b * P.k_sb + (long)hk * P.k_sh;
  const uint8_t* vb8 = reinterpret_cast<const uint8_t*>(P.v) + (long)b * P.v_sb + (long)hk * P.v_sh;
  const float* ksp = FP8 ? P.k_scale + (long)b * P.ks_sb + (long)hk * P.ks_sh : nullptr;
  const float* vsp = FP8 ? P.v_scale + (long)b * P.vs_sb + (long)hk * P.vs_sh : nullptr;

  bf16x8v kf[2][KS];  // the step's two K tiles: key k0 + 16 t + c, columns 32 ks + 8 g ..
  u16x8 vr[VPL];      // the step's V slab on its way to LDS: chunk lane + 64 j
  u32x4 kc[2][KL];    // FP8: the two K tiles as codes, columns 64 l + 16 g ..
  u32x4 vc[VPL8];     // FP8: the V slab as codes, 16-code chunk lane + 64 j
  uint8_t kp[2][4];   // visibility of the lane's keys k0 + 16 t + 4 g + i
  float lb[2][4];     // their bias, in log2 units
  float kq[2][4], vq[2][4];  // FP8: their k_scale and v_scale
  auto load_step = [&](int k0) {
    if constexpr (FP8) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int key = min(k0 + 16 * t + c, P.Sk - 1);  // past the end: a valid row, its score is masked below
#pragma unroll
        for (int l = 0; l < KL; ++l) {
          const int d0 = 64 * l + 16 * g;
          u32x4 v = {0u, 0u, 0u, 0u};  // code 0 is +0
          if (d0 < P.D) v = *reinterpret_cast<const u32x4*>(kb8 + (long)key * P.k_ss + d0);
          kc[t][l] = v;
        }
      }
#pragma unroll
      for (int j = 0; j < VPL8; ++j) {
        const int idx = lane + 64 * j, r = idx / CPR8, ch = idx % CPR8;
        u32x4 v = {0u, 0u, 0u, 0u};  // rows past the end and columns past D as zeros: 0 * P = 0
        if (k0 + r < kend && 16 * ch < P.D) v = *reinterpret_cast<const u32x4*>(vb8 + (long)(k0 + r) * P.v_ss + 16 * ch);
        vc[j] = v;
      }
    } else {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int key = min(k0 + 16 * t + c, P.Sk - 1);  // past the end: a valid row, its score is masked below
        load_row_frags<DP>(kb + (long)key * P.k_ss, g, P.D, kf[t]);
      }
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        const int idx = lane + 64 * j, r = idx / CPR, ch = idx % CPR;
        u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};  // rows past the end and columns past D as zeros: 0 * P = 0
        if (k0 + r < kend && 8 * ch < P.D) v = *reinterpret_cast<const u16x8*>(vb + (long)(k0 + r) * P.v_ss + 8 * ch);
        vr[j] = v;
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = k0 + 16 * t + 4 * g + i;
        const bool in = key < kend;
        kp[t][i] = in ? (kpm ? kpm[key] : (uint8_t)1) : (uint8_t)0;
        lb[t][i] = in && lutp ? lutp[key] * LOG2E : 0.f;
        if constexpr (FP8) {
          kq[t][i] = in ? ksp[(long)key * P.ks_ss] : 0.f;
          vq[t][i] = in ? vsp[(long)key * P.vs_ss] : 0.f;
        }
      }
    }
  };

  float m = -INFINITY, l = 0.f;
  f32x4 acc[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  int k0 = kbeg + STEP * w;  // uniform over the wave: EXEC stays full for the transposed reads
  if (k0 < kend) load_step(k0);
  for (; k0 < kend; k0 += 4 * STEP) {
    wave_lds_order();  // the previous step's slab reads come first
    if constexpr (FP8) {
#pragma unroll
      for (int j = 0; j < VPL8; ++j) {  // widened here: the slab is the bf16 one
        const int idx = lane + 64 * j, r = idx / CPR8, ch = idx % CPR8;
        *reinterpret_cast<u32x4*>(slab + r * LD + 16 * ch) = widen8(vc[j].x, vc[j].y);
        *reinterpret_cast<u32x4*>(slab + r * LD + 16 * ch + 8) = widen8(vc[j].z, vc[j].w);
      }
    } else {
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        const int idx = lane + 64 * j, r = idx / CPR, ch = idx % CPR;
        *reinterpret_cast<u16x8*>(slab + r * LD + 8 * ch) = vr[j];
      }
    }
    wave_lds_order();
    f32x4 st[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (FP8) {
#pragma unroll
        for (int l = 0; l < KL; ++l) {
          st[t] = mma(__builtin_bit_cast(bf16x8v, widen8(kc[t][l].x, kc[t][l].y)), qf[2 * l], st[t]);
          st[t] = mma(__builtin_bit_cast(bf16x8v, widen8(kc[t][l].z, kc[t][l].w)), qf[2 * l + 1], st[t]);
        }
      } else {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) st[t] = mma(kf[t][ks], qf[ks], st[t]);
      }
    }
    // st[t][i] = S[row c][key k0 + 16 t + 4 g + i]
    uint8_t vis[2][4];
    float bias[2][4], ksc[2][4], vsc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        vis[t][i] = kp[t][i];
        bias[t][i] = lb[t][i];
        if constexpr (FP8) {
          ksc[t][i] = kq[t][i];
          vsc[t][i] = vq[t][i];
        }
      }
    }
    if (k0 + 4 * STEP < kend) load_step(k0 + 4 * STEP);  // in flight under the softmax and P V
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float x;
        if constexpr (CAP && FP8) x = capc2 * tanh_ex2(st[t][i] * (capz2 * ksc[t][i]));
        else if constexpr (CAP) x = capc2 * tanh_ex2(st[t][i] * capz2);  // c tanh(scale s / c), in log2 units
        else if constexpr (FP8) x = st[t][i] * (scale2 * ksc[t][i]) + bias[t][i];
        else x = st[t][i] * scale2 + bias[t][i];
        if (!vis[t][i]) x = -INFINITY;
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
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pr = ex2(st[t][i] - mu);
        ls += pr;
        if constexpr (FP8) st[t][i] = pr * vsc[t][i];  // V's scale rides on P: the row sum stays that of P
        else st[t][i] = pr;
      }
    }
    ls = grp_sum(ls);
    l = l * alpha + ls;
    m = mn;
    const bf16x8v pb = pack8(st[0], st[1]);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] = mma(ld_tr2<DP>(slab, 0, 16 * dt, c, g), pb, acc[dt] * alpha);
  }
  // acc[dt][i] = O[row c][d = 16 dt + 4 g + i] of the wave's keys, unnormalised.  Merge the four waves through LDS:
  // every wave parks its state in its own slab (its reads of it are over), then wave w reduces the tiles dt = w, w + 4 ..
  wave_lds_order();
  float* mine = reinterpret_cast<float*>(slab);
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<f32x4*>(mine + (dt * 64 + lane) * 4) = acc[dt];
  if (g == 0) {
    mine[DT * 256 + c] = m;
    mine[DT * 256 + 16 + c] = l;
  }
  __syncthreads();
  const float* all = reinterpret_cast<const float*>(Vs);
  constexpr int SLABF = SLAB / 2;
  float f[4], M = -INFINITY, Ls = 0.f;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    f[x] = all[x * SLABF + DT * 256 + c];
    M = fmaxf(M, f[x]);
  }
  const float mu = M == -INFINITY ? 0.f : M;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    f[x] = ex2(f[x] - mu);
    Ls += all[x * SLABF + DT * 256 + 16 + c] * f[x];
  }
  const long bh = (long)b * P.Hkv + hk;
  if (P.splits > 1 && w == 0 && g == 0) {
    float* ml = P.part_ml + (bh * P.splits + s) * 32;
    ml[c] = M;
    ml[16 + c] = Ls;
  }
  const float inv = Ls > 0.f ? 1.f / Ls : 0.f;
  for (int dt = w; dt < DT; dt += 4) {
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int x = 0; x < 4; ++x) o += *reinterpret_cast<const f32x4*>(all + x * SLABF + (dt * 64 + lane) * 4) * f[x];
    const int d0 = 16 * dt + 4 * g;
    if (row_ok && d0 < P.D) {
      if (P.splits > 1)
        *reinterpret_cast<f32x4*>(P.part_o + ((bh * P.splits + s) * R + c) * P.D + d0) = o;
      else
        st4(P.o + (long)b * P.o_sb + (long)qi * P.o_ss + (long)hq * P.o_sh + d0, o * inv);
    }
  }
}

// o[b][i][h][d0 .. d0 + 3] from the splits' partials, one thread per 4 head-dim elements of a row; the splits are
// reduced in ascending order by one thread: no atomics, the same bits on every run
__global__ __launch_bounds__(NT) void attn_decode_merge_kernel(AttnDecodeParams P) {
  const int D4 = P.D / 4, R = P.Sq * P.G;
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  if (idx >= (long)P.B * P.Hkv * R * D4) return;
  const int d0 = 4 * (int)(idx % D4), r = (int)(idx / D4 % R);
  const long bh = idx / D4 / R;
  const float* ml = P.part_ml + bh * P.splits * 32;
  float M = -INFINITY;
  for (int s = 0; s < P.splits; ++s) M = fmaxf(M, ml[s * 32 + r]);
  const float mu = M == -INFINITY ? 0.f : M;
  float Ls = 0.f;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < P.splits; ++s) {
    const float f = ex2(ml[s * 32 + r] - mu);
    Ls += ml[s * 32 + 16 + r] * f;
    o += *reinterpret_cast<const f32x4*>(P.part_o + ((bh * P.splits + s) * R + r) * P.D + d0) * f;
  }
  const int b = (int)(bh / P.Hkv), hk = (int)(bh % P.Hkv), qi = r / P.G, hq = hk * P.G + r % P.G;
  st4(P.o + (long)b * P.o_sb + (long)qi * P.o_ss + (long)hq * P.o_sh + d0, o * (Ls > 0.f ? 1.f / Ls : 0.f));
}

int cu_count() {
  static int n = 0;
  if (n == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      v = 256;
    n = v;
  }
  return n;
}

template <int DP, bool FP8>
void launch_as(const AttnDecodeParams& P, hipStream_t st) {
  const dim3 grid(P.splits, P.Hkv, P.B);
  if (P.softcap > 0.f) hipLaunchKernelGGL((attn_decode_kernel<DP, true, FP8>), grid, dim3(NT), 0, st, P);
  else hipLaunchKernelGGL((attn_decode_kernel<DP, false, FP8>), grid, dim3(NT), 0, st, P);
}
template <int DP>
void launch(const AttnDecodeParams& P, hipStream_t st) {
  if (P.k_scale != nullptr) launch_as<DP, true>(P, st);
  else launch_as<DP, false>(P, st);
}

// Rows of D bf16 to D e4m3fn codes and one fp32 scale (attn_params.h AttnDecodeParams, FP8 K/V).  LG lanes serve a row
// (LG: D / 8 rounded up to a power of two; the lanes past D / 8 idle), 64 / LG rows a wave: one 16-B load, the row's
// max by xor shuffles inside the group, four v_cvt_pk_fp8_f32, one 8-B store per lane and one scale store per row.
__global__ __launch_bounds__(NT) void attn_kv_quant_kernel(const uint16_t* kv, long row_stride, uint8_t* codes,
                                                           float* scales, long rows, int D, int LG) {
  const int sub = threadIdx.x % LG;
  const long row = ((long)blockIdx.x * NT + threadIdx.x) / LG;
  const bool on = row < rows && 8 * sub < D;  // a group is never split over two waves: the shuffles below stay inside
  float x[8];
  float amax = 0.f;
  if (on) {
    const u16x8 v = *reinterpret_cast<const u16x8*>(kv + row * row_stride + 8 * sub);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      x[i] = bf2f(v[i]);
      amax = fmaxf(amax, fabsf(x[i]));
    }
  }
  for (int m = LG >> 1; m >= 1; m >>= 1) amax = fmaxf(amax, __shfl_xor(amax, m, 64));
  if (!on) return;
  const float scale = amax == 0.f ? 1.f : amax / 448.f;  // IEEE divide (no fast-math): the composite's bits
  uint32_t w[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    float y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = fminf(fmaxf(x[4 * i + j] / scale, -448.f), 448.f);
    int c = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
    c = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], c, true);
    w[i] = (uint32_t)c;
  }
  *reinterpret_cast<uint2*>(codes + row * D + 8 * sub) = make_uint2(w[0], w[1]);
  if (sub == 0) scales[row] = scale;
}

}  // namespace

extern "C" int dllm_attn_decode_plan(AttnDecodeParams* pp) {
  AttnDecodeParams& P = *pp;
  const bool fp8 = P.k_scale != nullptr;
  if (P.D < 32 || P.D > 256 || P.D % (fp8 ? 16 : 8)) return -1;
  if (fp8 != (P.v_scale != nullptr)) return -9;
  if (P.Hkv <= 0 || P.H % P.Hkv) return -2;
  if (P.B <= 0 || P.Sq <= 0 || P.Sk <= 0 || P.B > 65535 || P.Hkv > 65535) return -3;
  P.G = P.H / P.Hkv;
  if ((long)P.Sq * P.G > 16) return -4;
  if (P.softcap < 0.f || (P.softcap > 0.f && P.lut != nullptr)) return -5;
  if (P.splits < 0) return -6;
  long want = P.splits;
  if (want == 0) {
    // enough workgroups to fill the chip, no split below the floor; 1 once B * Hkv alone fills it
    const int dp = P.D <= 64 ? 64 : P.D <= 128 ? 128 : 256;
    const long bh = (long)P.B * P.Hkv, target = (long)(fp8 ? fill_per_cu_fp8(dp) : FILL_PER_CU) * cu_count();
    const long floor_keys = fp8 ? SPLIT_FLOOR_BYTES_FP8 / dp : SPLIT_FLOOR_BYTES / (dp * 2);
    want = std::max(1L, std::min((target + bh - 1) / bh, (long)P.Sk / floor_keys));
  }
  const long per = (P.Sk + want - 1) / want;
  const long L = std::min<long>((per + SPLIT_ALIGN - 1) / SPLIT_ALIGN * SPLIT_ALIGN, 0x40000000L);
  P.L = (int)L;
  P.splits = (int)((P.Sk + L - 1) / L);
  return 0;
}

extern "C" int dllm_attn_decode(const AttnDecodeParams* pp, hipStream_t st) {
  const AttnDecodeParams P = *pp;
  if (P.L <= 0 || P.L % SPLIT_ALIGN || P.G <= 0 || P.splits != (P.Sk + P.L - 1) / P.L) return -7;  // not planned
  if (P.splits > 1 && (P.part_o == nullptr || P.part_ml == nullptr)) return -8;
  if ((P.k_scale != nullptr) != (P.v_scale != nullptr) || (P.k_scale != nullptr && P.D % 16)) return -9;
  if (P.D <= 64) launch<64>(P, st);
  else if (P.D <= 128) launch<128>(P, st);
  else launch<256>(P, st);
  if (P.splits > 1) {
    const long n = (long)P.B * P.Hkv * P.Sq * P.G * (P.D / 4);
    hipLaunchKernelGGL(attn_decode_merge_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, P);
  }
  DLLM_CHECK_LAUNCH();
  return 0;
}

extern "C" int dllm_kv_quant_fp8(const void* kv, long row_stride, uint8_t* codes, float* scales, long rows, int D,
                                 hipStream_t st) {
  if (D < 32 || D > 256 || D % 16 || rows < 0 || row_stride < D || row_stride % 8) return -1;
  if (rows == 0) return 0;
  int LG = 4;
  while (LG < D / 8) LG *= 2;  // 4 .. 32: a divisor of 64
  const long blocks = (rows * LG + NT - 1) / NT;
  if (blocks > 0x7FFFFFFFL) return -2;
  hipLaunchKernelGGL(attn_kv_quant_kernel, dim3((unsigned)blocks), dim3(NT), 0, st, static_cast<const uint16_t*>(kv),
                     row_stride, codes, scales, rows, D, LG);
  DLLM_CHECK_LAUNCH();
  return 0;
}
