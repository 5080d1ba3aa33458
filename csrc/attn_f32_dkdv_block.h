// One 64-query block of the dK / dV walk of csrc/attn_f32.hip (attn_f32_dkdv_kernel): Q and dO staged (row-major and
// transposed) with the rows' LSE, delta and dropout hashes, S and dP, dV += P_kept^T dO, dK += dS^T Q.  A fragment, not
// a header, as csrc/attn_hd_fwd_block.h: included inside the kernel's loops, where q0 and the kernel's locals are in
// scope.
    __syncthreads();
    stage<true, true>(qb, P.q_ss, q0, P.Sq, Qs, Qt, tid);
    stage<true, true>(ob, P.do_ss, q0, P.Sq, Os, Ot, tid);
    stage_bias(P, h, q0, k0, Ls, tid, 1.f);
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
      float qf[16], of[16];
      rd_row16(Qs, 16 * t + c, g, qf);
      rd_row16(Os, 16 * t + c, g, of);
      sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        sc[t] = mma(qf[s], kf[s], sc[t]);
        dp[t] = mma(of[s], vf[s], dp[t]);
      }
    }
    // sc[t][i] = S[row = q0 + 16 t + 4 g + i][key]; pd = kept P, sc <- dS
    f32x4 pd[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int rl = 16 * t + 4 * g + i, row = q0 + rl;
        float x = sc[t][i] * P.scale, dtanh = 1.f;  // dtanh = 1 - tanh^2, the cap's derivative
        if constexpr (CAP) {
          const float th = tanhf(x * capinv);
          x = P.softcap * th;
          dtanh = 1.f - th * th;
        }
        if (P.lut) x += Ls[key - row - (k0 - q0 - 63)];
        const bool msk = hidden(vis, t, i) || (P.causal && key > row + P.causal_off) ||
                         (P.window >= 0 && off_band_w(kwin, row, key));
        const float pr = msk ? 0.f : __expf(x - Rl[rl]);
        const bool kp = DROP ? keep_key(Rh[rl], key, P.thr) : true;
        const float dpk = kp ? dp[t][i] * dscale : 0.f;
        pd[t][i] = kp ? pr * dscale : 0.f;
        sc[t][i] = CAP ? pr * (dpk - Rd[rl]) * dtanh : pr * (dpk - Rd[rl]);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const f32x4 oa = rd_col4(Ot, 16 * dt + c, 16 * t + 4 * g);
        const f32x4 qa = rd_col4(Qt, 16 * dt + c, 16 * t + 4 * g);
        dv[dt] = mma(pd[t][0], oa.x, dv[dt]);
        dv[dt] = mma(pd[t][1], oa.y, dv[dt]);
        dv[dt] = mma(pd[t][2], oa.z, dv[dt]);
        dv[dt] = mma(pd[t][3], oa.w, dv[dt]);
        dk[dt] = mma(sc[t][0], qa.x, dk[dt]);
        dk[dt] = mma(sc[t][1], qa.y, dk[dt]);
        dk[dt] = mma(sc[t][2], qa.z, dk[dt]);
        dk[dt] = mma(sc[t][3], qa.w, dk[dt]);
      }
    }
