// One 64-key block of the forward walk of csrc/attn_hd.hip (attn_hd_fwd_kernel): K and V staged, S^T = K Q^T, online
// softmax + dropout in registers, O^T += V^T P^T.  A fragment, not a header: included inside the kernel, where k0 and
// the kernel's locals are in scope — twice, once in place in the head dim 32 loop and once in the lambda the other
// head dims expand into their two loops (the kernel says why).
    __syncthreads();  // the previous block's LDS reads are done
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
    f32x4 st[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) st[t] = mma(ld_row<DP>(Ks, 16 * t + c, ks, g), qf[ks], st[t]);
    }
    // st[t][i] = S[row][key = k0 + 16 t + 4 g + i]
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = k0 + 16 * t + 4 * g + i;
        float x;
        if constexpr (CAP) x = capc2 * tanh_ex2(st[t][i] * capz2);  // c tanh(scale s / c), in log2 units
        else x = st[t][i] * scale2;
        if (P.lut) x += Ls[key - row - (k0 - q0 - 63)];
        if (hidden(vis, t, i) || (P.causal && key > row + P.causal_off) ||
            (DP != 32 ? off_band(P, row, key, vis, t, i) : off_band(P, row, key)))
          x = -INFINITY;
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
    for (int t = 0; t < 4; ++t) {
      const uint32_t kb4 = DROP ? keep4(rh, k0 + 16 * t + 4 * g, P.thr) : 0xFu;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pr = ex2(st[t][i] - mu);
        ls += pr;
        st[t][i] = DROP ? (((kb4 >> i) & 1u) ? pr * dscale : 0.f) : pr;
      }
    }
    ls = grp_sum(ls);
    l = l * alpha + ls;
    m = mn;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] *= alpha;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bf16x8v pb = pack8(st[2 * u], st[2 * u + 1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) acc[dt] = mma(ld_tr2<DP>(Vs, 32 * u, 16 * dt, c, g), pb, acc[dt]);
    }
