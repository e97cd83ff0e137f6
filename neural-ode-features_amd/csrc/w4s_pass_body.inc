// The body of a GroupNorm / transform pass (kernels_w4s.hip), included as TEXT into k_w4s_pass and k_w4s_pass_rider.  In scope where
// it is included: HEAD, TAIL, Q (compile-time), the kernel's W4sArgs `a`, and `block`, the workgroup's index in the pass's grid
// (w4s_grid).  Text and not a device function on purpose: behind a function boundary -- even a force-inlined one -- the compiler
// pairs these multiplies and adds into packed instructions differently and contracts four fewer of them per pass, which changes the
// last bit of a solve's results (measured on the instruction counts of every instantiation).
  __shared__ float s_red[Q == 4 ? W4Q_RED : 1];
  __shared__ float s_tiles[Q == 4 ? W4Q_TILES : 1];
  W4Wave<Q> wv;
  w4s_place(wv, a.C, s_red, s_tiles, block);
  const int lane = wv.lane, CB = a.C >> 4, n = wv.n, cb = wv.cb, t = wv.t, c = wv.c;
  const int cpg = a.cpg, G = a.C / cpg, grp = c / cpg;
  const float inv_m = 1.0f / (float)(64 * Q * cpg);
  const size_t f4 = ((size_t)wv.nv * CB + cb) * 256 + lane;   // float4 index of tile row 0 in a W4S tensor (rows 64 apart)
  const bool stat_lane = t == 0 && wv.q == 0 && c % cpg == 0;   // the one lane of the launch that owns (sample, group)

  float v[4][4];     // the conv input whose transform leaves at the end
  float hx[4][4];    // HEAD 1: xhat of the head's GroupNorm
  float ho[4][4];    // the head's output (a stage derivative)
  float hrstd = 0.f;

  if (HEAD == 1) {
    const W4sHead& h = a.h;
    float z[4][4];
    w4s_out_transform(w4s_m_ptr(h.M, wv, a.C), z);
    const float tval = eval_time(h.et), bv = h.bias[c];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 tm = w4s_ld4(h.tmapS, ((size_t)wv.q * CB + cb) * 256 + i * 64 + lane);
      z[i][0] += fmaf(tval, tm.x, bv); z[i][1] += fmaf(tval, tm.y, bv); z[i][2] += fmaf(tval, tm.z, bv); z[i][3] += fmaf(tval, tm.w, bv);
    }
    float mean;
    w4s_gn_stats(z, cpg, inv_m, a.eps, wv, mean, hrstd);
    const float gam = h.gamma[c], bet = h.beta[c];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        hx[i][j] = (z[i][j] - mean) * hrstd;
        float vv = fmaf(hx[i][j], gam, bet);
        if (h.relu) vv = fmaxf(vv, 0.f);
        ho[i][j] = h.osign * vv;
      }
    if (h.out_s) {
#pragma unroll
      for (int i = 0; i < 4; ++i) w4s_st4(h.out_s, f4 + i * 64, ho[i]);
    }
    if (h.out_nhwc) w4s_store_nhwc(h.out_nhwc, wv, a.C, ho);
    if (h.xhat_s) {
#pragma unroll
      for (int i = 0; i < 4; ++i) w4s_st4(h.xhat_s, f4 + i * 64, hx[i]);
    }
    if (h.rstd && stat_lane) h.rstd[(size_t)n * G + grp] = hrstd;
    if (TAIL == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = ho[i][j];
    }
  }
  if (HEAD == 2) {
    const W4sHead& h = a.h;
    float4 xq[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xq[i] = w4s_ld4(h.xhat_s, f4 + i * 64);
    const float gam = h.gamma[c], bet = h.beta[c], rs = h.rstd[(size_t)n * G + grp];
    float g[4][4], xh[4][4];
    w4s_out_transform(w4s_m_ptr(h.M, wv, a.C), g);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xh[i][0] = xq[i].x; xh[i][1] = xq[i].y; xh[i][2] = xq[i].z; xh[i][3] = xq[i].w;
#pragma unroll
      for (int j = 0; j < 4; ++j) g[i][j] = fmaf(xh[i][j], gam, bet) > 0.f ? g[i][j] : 0.f;   // ReLU mask of this layer's output
    }
    w4s_gn_bwd(g, xh, gam, rs, cpg, inv_m, h.osign, wv, a.C, h.gpart, ho);
    if (h.out_s) {
#pragma unroll
      for (int i = 0; i < 4; ++i) w4s_st4(h.out_s, f4 + i * 64, ho[i]);
    }
    if (h.out_nhwc) w4s_store_nhwc(h.out_nhwc, wv, a.C, ho);
    if (h.spart) w4s_colsums(ho, wv, h.spart, a.C);
    if (a.gstat != nullptr && (h.z_out != nullptr || (TAIL == 0 && a.V != nullptr))) w4s_record_max(ho, a.gstat, a.z_exp != nullptr ? a.z_exp : (TAIL == 0 ? a.v_exp : nullptr));
    if (h.z_out) {
      if (a.z_exp != nullptr) w4s_emit_zh(ho, w4s_vh_ptr(h.z_out, wv, a.C), (size_t)4 * a.Nv * a.C, ldexpf(1.f, *a.z_exp), (wv.c15 & 1) != 0);
      else w4s_emit_z(ho, wv.nv, a.Nv, a.C, c, t, h.z_out);
    }
    if (TAIL == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = ho[i][j];
    }
  }

  if (TAIL != 0) {
    const W4sTail& tl = a.t;
    const float scale = comb_scale(tl.comb, a.ctrl);
    float cf[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) cf[j] = scale * tl.comb.coef[j];
    float y[4][4];
    if (HEAD == 1 && TAIL == 1) {
      if (tl.self) w4s_comb_any<true>(tl.comb, cf, f4, ho, y);
      else w4s_comb_any<false>(tl.comb, cf, f4, ho, y);
    } else {
      w4s_comb_any<false>(tl.comb, cf, f4, ho, y);
    }
    if (tl.y_out) {
#pragma unroll
      for (int i = 0; i < 4; ++i) w4s_st4(tl.y_out, f4 + i * 64, y[i]);
    }
    if (TAIL == 1) {   // GroupNorm-1 -> ReLU (model.py:341-342)
      float mean, rstd;
      w4s_gn_stats(y, cpg, inv_m, a.eps, wv, mean, rstd);
      const float gam = tl.gamma[c], bet = tl.beta[c];
      float xh[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          xh[i][j] = (y[i][j] - mean) * rstd;
          v[i][j] = fmaxf(fmaf(xh[i][j], gam, bet), 0.f);
        }
      if (tl.act_nhwc) w4s_store_nhwc(tl.act_nhwc, wv, a.C, v);
      if (tl.xhat_s) {
#pragma unroll
        for (int i = 0; i < 4; ++i) w4s_st4(tl.xhat_s, f4 + i * 64, xh[i]);
      }
      if (tl.rstd && stat_lane) tl.rstd[(size_t)n * G + grp] = rstd;
    } else {   // cotangent g = csign * (adjoint combine) through GroupNorm-3's backward (xhat-3, 1/sigma-3 from the head)
      float g[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) g[i][j] = tl.csign * y[i][j];
      w4s_gn_bwd(g, hx, a.h.gamma[c], hrstd, cpg, inv_m, 1.f, wv, a.C, tl.gpart, v);
      if (tl.act_nhwc) w4s_store_nhwc(tl.act_nhwc, wv, a.C, v);
      if (tl.spart) w4s_colsums(v, wv, tl.spart, a.C);
      if (a.gstat != nullptr) w4s_record_max(v, a.gstat, a.z_exp != nullptr ? a.z_exp : a.v_exp);
      if (tl.z_out) {
        if (a.z_exp != nullptr) w4s_emit_zh(v, w4s_vh_ptr(tl.z_out, wv, a.C), (size_t)4 * a.Nv * a.C, ldexpf(1.f, *a.z_exp), (wv.c15 & 1) != 0);
        else w4s_emit_z(v, wv.nv, a.Nv, a.C, c, t, tl.z_out);
      }
    }
  }

  if (a.V != nullptr) w4s_put_v(v, wv, a.V, a.C, a.Nv, a.v_exp);
