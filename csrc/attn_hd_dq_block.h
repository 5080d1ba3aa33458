// One 64-key block of the dQ walk of csrc/attn_hd.hip (attn_hd_dq_kernel): K and V staged, S^T and dP^T, dS, dQ^T +=
// K^T dS^T, the bias gradient's diagonal sums.  A fragment, not a header, as csrc/attn_hd_fwd_block.h: included inside
// the kernel, in place in the head dim 32 loop and in the lambda of the other head dims.
    __syncthreads();
    stage<DP>(kb, P.k_ss, k0, P.Sk, P.D, Ks, tid);
    stage<DP>(vb, P.v_ss, k0, P.Sk, P.D, Vs, tid);
    stage_bias(P, h, q0, k0, Ls, tid, LOG2E);
    if (tid < BKY) {
      Mk[tid] = DP != 32 ? key_byte(P, b, k0 + tid) : (uint8_t)key_ok(P, b, k0 + tid);  // no global keys at DP = 32
      if (P.q_seg) Sg[tid] = seg_at(P.k_seg, b, P.Sk, k0 + tid);
    }
    __syncthreads();
    // key valid and of the row's segment (low half); key global (high half)
    const uint32_t vis = key_bits(P, Mk, Sg, qsg, g) | (DP != 32 ? glob_bits(P, Mk, g) : 0u);
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
      const uint32_t kb4 = DROP ? keep4(rh, k0 + 16 * t + 4 * g, P.thr) : 0xFu;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = k0 + 16 * t + 4 * g + i;
        const int di = key - row - (k0 - q0 - 63);
        float x, dtanh = 1.f;  // dtanh = 1 - tanh^2, the cap's derivative
        if constexpr (CAP) {
          const float th = tanh_ex2(st[t][i] * capz2);
          x = capc2 * th;
          dtanh = 1.f - th * th;
        } else {
          x = st[t][i] * scale2;
        }
        if (P.lut) x += Ls[di];
        const bool msk =
            hidden(vis, t, i) || (P.causal && key > row + P.causal_off) ||
            (DP != 32 ? off_band(P, row, key, vis, t, i) : off_band(P, row, key));
        const float pr = msk ? 0.f : ex2(x - lse);
        const float dpk = DROP ? (((kb4 >> i) & 1u) ? dpt[t][i] * dscale : 0.f) : dpt[t][i];
        const float ds = CAP ? pr * (dpk - dlt) * dtanh : pr * (dpk - dlt);
        st[t][i] = ds;
        if (want_dlut) Ds[(16 * w + c) * (BKY + 1) + 16 * t + 4 * g + i] = ds;  // 0 for rows >= Sq (lse = inf)
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bf16x8v sb = pack8(st[2 * u], st[2 * u + 1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) acc[dt] = mma(ld_tr2<DP>(Ks, 32 * u, 16 * dt, c, g), sb, acc[dt]);
    }
    if (want_dlut) {
      __syncthreads();  // the block's dS tile is complete
      dlut_add_diagonals(P, h, q0, k0, Ds, tid);
    }
