// One 64-query block of the dK / dV walk of csrc/attn_hd.hip (attn_hd_dkdv_kernel): Q and dO staged with the rows' LSE,
// delta and dropout hashes, S and dP, dV^T += dO^T P_kept, dK^T += Q^T dS.  A fragment, not a header, as
// csrc/attn_hd_fwd_block.h: included inside the kernel, in place in the head dim 32 loop and in the lambda of the other
// head dims, where q0 and the kernel's locals are in scope.
    __syncthreads();
    stage<DP>(qb, P.q_ss, q0, P.Sq, P.D, Qs, tid);
    stage<DP>(ob, P.do_ss, q0, P.Sq, P.D, Os, tid);
    stage_bias(P, h, q0, k0, Ls, tid, LOG2E);
    if (tid < BQ) {
      const int r = q0 + tid;
      const bool ok = r < P.Sq;
      Rl[tid] = ok ? P.lse[(long)bh * P.Sq + r] : INFINITY;
      Rd[tid] = ok ? P.delta[(long)bh * P.Sq + r] : 0.f;
      if (DROP) Rh[tid] = mix32(seed, (uint32_t)((long)bh * P.Sq + min(r, P.Sq - 1)));
      if (P.q_seg) Rs[tid] = seg_at(P.q_seg, b, P.Sq, r);
    }
    __syncthreads();
    const uint32_t vis = kok ? seg_bits(P, Rs, ksg, g) : 0u;  // key valid and of the rows' segments
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
    // sc[t][i] = S[row = q0 + 16 t + 4 g + i][key]; pd = kept P, sc <- dS
    f32x4 pd[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int rl = 16 * t + 4 * g + i, row = q0 + rl;
        float x, dtanh = 1.f;  // dtanh = 1 - tanh^2, the cap's derivative
        if constexpr (CAP) {
          const float th = tanh_ex2(sc[t][i] * capz2);
          x = capc2 * th;
          dtanh = 1.f - th * th;
        } else {
          x = sc[t][i] * scale2;
        }
        if (P.lut) x += Ls[key - row - (k0 - q0 - 63)];
        const bool msk = hidden(vis, t, i) || (P.causal && key > row + P.causal_off) ||
                         (DP == 32 ? off_band(P, row, key) : (P.window >= 0 && off_band_w(kwin, row, key)));
        const float pr = msk ? 0.f : ex2(x - Rl[rl]);
        const bool kp = DROP ? keep_key(Rh[rl], key, P.thr) : true;
        const float dpk = kp ? dp[t][i] * dscale : 0.f;
        pd[t][i] = kp ? pr * dscale : 0.f;
        sc[t][i] = CAP ? pr * (dpk - Rd[rl]) * dtanh : pr * (dpk - Rd[rl]);
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
