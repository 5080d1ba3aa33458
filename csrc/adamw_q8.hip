// 8-bit AdamW (Dettmers et al. 2022, block-wise dynamic quantisation) over the flat parameter space, for gfx950: the
// two moments live as one uint8 code per element plus one fp32 scale (absmax) per 64-element block and state; the fp32
// master, the gradient and the decay mask are those of csrc/adamw.hip.  The contract — code books, midpoint rule, the
// order of operations — is ops/q8.py's; the recurrence is adamw8_kernel's of csrc/adamw.hip, in fp32.
//
// One launch, grid-stride over 64-blocks, no atomics, no barrier after the table staging:
//   * a wave covers 256 consecutive elements = 4 blocks: one 16-lane group (a DPP row) per block, 4 consecutive
//     elements per lane.  The 4 codes of a state are one 32-bit load, gradient and master 16-byte loads, the bf16
//     parameter one 8-byte store, the decay mask one 32-bit load; every load of an iteration is issued before any math
//     (the side-store loads excepted: they wait for the block's slot);
//   * the two code books and their 255 midpoints each are staged in LDS once per workgroup (4 KiB, from the `tables`
//     operand: T_signed | T_unsigned | mid_signed | mid_unsigned, 256 floats each).  Dequantisation is one lookup and
//     one multiply.  Requantisation is the midpoint rule itself: code = #{i : mid[i] < x}, x = value / absmax (one
//     correctly rounded division), found by an 8-step branch-free binary search over the LDS midpoints; the 8 searches
//     of a lane (4 elements x 2 states) run interleaved, 8 independent LDS reads per step;
//   * the new block maxima are xor-butterflies inside the DPP row (quad_perm x 2, row_half_mirror, row_mirror): 4 VALU
//     steps per state, no LDS, no barrier;
//   * a group whose block has a slot >= 0 keeps fp32 moments: it reads and writes 64 floats at slot * 64 of the side
//     store per state instead of codes and skips the searches; the divergence is per group.  A slot >= nslots touches
//     nothing (the block is skipped): a table the kernel cannot trust must not become an address.
// Bytes per parameter (bf16 + master): grad 4, master 4 + 4, param 2, codes 1 + 1 + 1 + 1, scales and slot 20 / 64,
// mask 1: 18.3 without the mask, against 31 of the fp32 step.
#include "common.h"

using namespace dllm;

namespace {

constexpr int Q8_BLOCK = 64;                  // elements per quantisation block
constexpr int Q8_WG_BLOCKS = 16;              // blocks per workgroup and iteration: 4 waves x 4 groups
constexpr int Q8_GRID_CAP = 2048;             // 8 workgroups per CU
constexpr int Q8_TABLE_FLOATS = 1024;

template <int CTRL>
DLLM_DEVICE float dpp_f(float v) {
  const int i = __float_as_int(v);
  return __int_as_float(__builtin_amdgcn_update_dpp(i, i, CTRL, 0xF, 0xF, false));
}
// max over the 16 lanes of a DPP row, in every lane of the row (v >= 0)
DLLM_DEVICE float row16_max(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));   // quad_perm [1, 0, 3, 2]: lane ^ 1
  v = fmaxf(v, dpp_f<0x4E>(v));   // quad_perm [2, 3, 0, 1]: lane ^ 2
  v = fmaxf(v, dpp_f<0x141>(v));  // row_half_mirror: the other quad of the half (quads are uniform by now)
  v = fmaxf(v, dpp_f<0x140>(v));  // row_mirror: the other half of the row
  return v;
}

template <typename TP, bool MASTER>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void adamw_q8_kernel(
    TP* __restrict__ param, float* __restrict__ master, const float* __restrict__ grad, uint8_t* __restrict__ code_m,
    uint8_t* __restrict__ code_v, float* __restrict__ absmax_m, float* __restrict__ absmax_v,
    const int* __restrict__ slots, float* __restrict__ side_m, float* __restrict__ side_v, int nslots,
    const uint8_t* __restrict__ wd_mask, const float* __restrict__ tables, const float* __restrict__ coef_p, long nblk,
    float lr, float b1, float b2, float eps, float wd, float step_size, float inv_sqrt_bc2,
    const float* __restrict__ hyper) {
  __shared__ float lut[Q8_TABLE_FLOATS];
  for (int i = threadIdx.x; i < Q8_TABLE_FLOATS; i += 256) lut[i] = tables[i];
  __syncthreads();
  const float* t_s = lut;            // signed code book (exp_avg)
  const float* t_u = lut + 256;      // unsigned code book (exp_avg_sq)
  const float* mid_s = lut + 512;    // 255 midpoints each (+ one pad)
  const float* mid_u = lut + 768;

  const float coef = coef_p[0];
  if (hyper != nullptr) {  // graph-replayed steps: lr / bias corrections computed on the device (ops/optim.py)
    lr = hyper[0];
    step_size = hyper[1];
    inv_sqrt_bc2 = hyper[2];
  }
  const float dec = lr * wd;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane >> 4, l16 = lane & 15;
  const long nquad = (nblk + 3) / 4;  // wave iterations: 4 blocks each, the last one possibly partial
  for (long q = blockIdx.x * 4L + wave; q < nquad; q += (long)gridDim.x * 4) {  // wave-uniform
    const long blk = q * 4 + grp;
    const bool in = blk < nblk;
    const long o = blk * Q8_BLOCK + l16 * 4;
    f32x4 g = {0.f, 0.f, 0.f, 0.f}, w = g, mm = g, vv = g;
    uint32_t mk = 0x01010101u, cm = 0, cv = 0;
    float am = 0.f, av = 0.f;
    int slot = -1;
    if (in) {
      slot = slots[blk];
      g = *reinterpret_cast<const f32x4*>(grad + o);
      w = MASTER ? *reinterpret_cast<const f32x4*>(master + o) : Elem<TP>::load4(param + o);
      cm = *reinterpret_cast<const uint32_t*>(code_m + o);
      cv = *reinterpret_cast<const uint32_t*>(code_v + o);
      am = absmax_m[blk];
      av = absmax_v[blk];
      if (wd_mask != nullptr) mk = *reinterpret_cast<const uint32_t*>(wd_mask + o);
    }
    const bool act = in && slot < nslots;  // the block is updated
    const bool side = act && slot >= 0;    // ... with fp32 moments from the side store
    const long so = (long)(side ? slot : 0) * Q8_BLOCK + l16 * 4;
    if (side) {
      mm = *reinterpret_cast<const f32x4*>(side_m + so);
      vv = *reinterpret_cast<const f32x4*>(side_v + so);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        mm[k] = t_s[(cm >> (8 * k)) & 0xFFu] * am;
        vv[k] = t_u[(cv >> (8 * k)) & 0xFFu] * av;
      }
    }
    float mxm = 0.f, mxv = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gk = g[k] * coef;
      const float d = ((mk >> (8 * k)) & 0xFFu) ? dec : 0.f;
      float wk = w[k] * (1.f - d);
      const float mk2 = mm[k] + (1.f - b1) * (gk - mm[k]);
      const float vk = b2 * vv[k] + (1.f - b2) * gk * gk;
      wk -= step_size * mk2 / (sqrtf(vk) * inv_sqrt_bc2 + eps);
      w[k] = wk;
      mm[k] = mk2;
      vv[k] = vk;
      mxm = fmaxf(mxm, fabsf(mk2));
      mxv = fmaxf(mxv, vk);
    }
    mxm = row16_max(mxm);  // outside the divergent part: a row's 16 lanes are always together
    mxv = row16_max(mxv);
    if (act) {
      if (MASTER) *reinterpret_cast<f32x4*>(master + o) = w;
      Elem<TP>::store4(param + o, w);
    }
    if (side) {
      *reinterpret_cast<f32x4*>(side_m + so) = mm;
      *reinterpret_cast<f32x4*>(side_v + so) = vv;
    } else if (act) {
      // x = value / absmax (an all-zero block: 0), code = #{midpoints < x}: lower_bound over 255 sorted midpoints
      float x[8];
      int pos[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        x[k] = mxm > 0.f ? __fdiv_rn(mm[k], mxm) : 0.f;
        x[4 + k] = mxv > 0.f ? __fdiv_rn(vv[k], mxv) : 0.f;
        pos[k] = pos[4 + k] = 0;
      }
#pragma unroll
      for (int step = 128; step >= 1; step >>= 1) {
        float md[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) md[j] = (j < 4 ? mid_s : mid_u)[pos[j] + step - 1];
#pragma unroll
        for (int j = 0; j < 8; ++j) pos[j] += md[j] < x[j] ? step : 0;
      }
      const uint32_t ncm = (uint32_t)pos[0] | ((uint32_t)pos[1] << 8) | ((uint32_t)pos[2] << 16) |
                           ((uint32_t)pos[3] << 24);
      const uint32_t ncv = (uint32_t)pos[4] | ((uint32_t)pos[5] << 8) | ((uint32_t)pos[6] << 16) |
                           ((uint32_t)pos[7] << 24);
      *reinterpret_cast<uint32_t*>(code_m + o) = ncm;
      *reinterpret_cast<uint32_t*>(code_v + o) = ncv;
      if (l16 == 0) {
        absmax_m[blk] = mxm;
        absmax_v[blk] = mxv;
      }
    }
  }
}

}  // namespace

extern "C" int dllm_adamw_q8_wg_elems() { return Q8_WG_BLOCKS * Q8_BLOCK; }
extern "C" int dllm_adamw_q8_grid_cap() { return Q8_GRID_CAP; }

// n % 64 == 0; bf16 parameters come with an fp32 master, fp32 parameters without one; fp32 gradients.  codes: n bytes
// per state, absmax: n / 64 floats per state, slots: n / 64 ints (-1: quantised, else the block's place in the side
// stores of nslots * 64 floats each), tables: 1024 floats (file header).
extern "C" int dllm_adamw_q8(void* param, float* master, const float* grad, uint8_t* code_m, uint8_t* code_v,
                             float* absmax_m, float* absmax_v, const int* slots, float* side_m, float* side_v,
                             int nslots, const uint8_t* wd_mask, const float* tables, const float* coef, long n,
                             float lr, float b1, float b2, float eps, float wd, float bc1, float bc2, int is_bf16,
                             const float* hyper, hipStream_t st) {
  if (n <= 0 || n % Q8_BLOCK) return -2;
  if ((is_bf16 != 0) != (master != nullptr)) return -3;
  if (nslots < 0 || (nslots > 0 && (side_m == nullptr || side_v == nullptr))) return -4;
  const long nblk = n / Q8_BLOCK;
  const long wgs = (nblk + Q8_WG_BLOCKS - 1) / Q8_WG_BLOCKS;
  const int G = (int)(wgs < Q8_GRID_CAP ? wgs : Q8_GRID_CAP);
  const float step_size = lr / bc1;
  const float inv_sqrt_bc2 = 1.f / sqrtf(bc2);
#define Q8(TP, MS)                                                                                                      \
  hipLaunchKernelGGL((adamw_q8_kernel<TP, MS>), dim3(G), dim3(256), 0, st, (TP*)param, master, grad, code_m, code_v,   \
                     absmax_m, absmax_v, slots, side_m, side_v, nslots, wd_mask, tables, coef, nblk, lr, b1, b2, eps,  \
                     wd, step_size, inv_sqrt_bc2, hyper)
  if (is_bf16) Q8(uint16_t, true);
  else Q8(float, false);
#undef Q8
  DLLM_CHECK_LAUNCH();
  return 0;
}
