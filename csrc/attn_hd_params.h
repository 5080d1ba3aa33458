// Parameter block for the bf16 attention kernels of any head dim 32 .. 128 (csrc/attn_hd.hip), filled by the host
// binding (csrc/bind.cpp).  Tensors are [B, S, H, D] bf16 views with the head dim contiguous, D % 8 == 0 and every
// stride a multiple of 8 elements (16-B row starts); strides in elements.
#pragma once
#include <stdint.h>

struct AttnHdParams {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  const uint16_t* o;     // bwd: forward output
  const uint16_t* dout;  // bwd: output gradient
  uint16_t* o_out;       // fwd output
  float* lse;            // [B, H, Sq], log2 units, +inf = row without a valid key: fwd writes, bwd reads
  float* delta;          // [B, H, Sq]: rowsum(dO * O), written by the bwd pre-pass
  uint16_t* dq;
  uint16_t* dk;
  uint16_t* dv;
  float* dlut;           // [H, Sq + Sk - 1] (bwd, accumulated with atomics; zeroed by the host)
  const uint8_t* kpm;    // [B, Sk] 1 = attend
  const float* lut;      // [H, Sq + Sk - 1] additive bias by relative position (key - row + Sq - 1)
  long q_sb, q_ss, q_sh;
  long k_sb, k_ss, k_sh;
  long v_sb, v_ss, v_sh;
  long o_sb, o_ss, o_sh;
  long do_sb, do_ss, do_sh;
  long dq_sb, dq_ss, dq_sh;
  long dk_sb, dk_ss, dk_sh;
  long dv_sb, dv_ss, dv_sh;
  int B, H, Sq, Sk;
  int D;           // real head dim (32 .. 128, % 8 == 0); the kernels are instantiated for D rounded up to 32
  float scale;
  int causal;
  int causal_off;  // Sk - Sq
  float p_drop;
  uint32_t seed;
  uint32_t thr;    // 16-bit keep threshold (ops/rng.py threshold16)
};
