// GroupNorm as a pointwise pass, for the geometries whose convolution does not carry it in its epilogue: the Butcher-tableau stage
// combine fused with GroupNorm + ReLU (k_combine_gn) and its backward (k_gn_bwd).  HBM-bound.
#include "pointwise_common.h"

namespace node {

// ============================================================================
// Stage combine + GroupNorm + ReLU
//   y_i  = y + scale * sum_j coef_j k_j                  (Butcher row)
//   act  = relu(GN(y_i) * gamma + beta)                   (model.py:341-342)
// One workgroup owns (sample n, a slab of whole groups): the combined values stay
// in LDS between the statistics pass and the normalise pass, so y_i is never
// written to HBM unless the caller asks for it (last stage -> y1).
// ============================================================================
// y + sum_j cf[j] * k[j] at TWO offsets of the same thread, every request issued before the first use.  Written as a
// loop over a run-time term count the compiler waits for each tensor's load before it requests the next: (1 + nk) x 2
// dependent round trips at the head of every combine (12 for the last dopri5 stage).  Same summation order as the
// generic loops below.
template <int NK>
__device__ __forceinline__ void comb_pair(const Comb& c, const float* cf, size_t off0, size_t off1, float4& r0, float4& r1) {
  float4 y0 = ld4(c.y + off0), y1 = ld4(c.y + off1);
  float4 k0[NK > 0 ? NK : 1], k1[NK > 0 ? NK : 1];
#pragma unroll
  for (int j = 0; j < NK; ++j) { k0[j] = ld4(c.k[j] + off0); k1[j] = ld4(c.k[j] + off1); }
  if (NK > 0) {
    float4 s0, s1;
    s0.x = cf[0] * k0[0].x; s0.y = cf[0] * k0[0].y; s0.z = cf[0] * k0[0].z; s0.w = cf[0] * k0[0].w;
    s1.x = cf[0] * k1[0].x; s1.y = cf[0] * k1[0].y; s1.z = cf[0] * k1[0].z; s1.w = cf[0] * k1[0].w;
#pragma unroll
    for (int j = 1; j < NK; ++j) {
      s0.x += cf[j] * k0[j].x; s0.y += cf[j] * k0[j].y; s0.z += cf[j] * k0[j].z; s0.w += cf[j] * k0[j].w;
      s1.x += cf[j] * k1[j].x; s1.y += cf[j] * k1[j].y; s1.z += cf[j] * k1[j].z; s1.w += cf[j] * k1[j].w;
    }
    y0.x += s0.x; y0.y += s0.y; y0.z += s0.z; y0.w += s0.w;
    y1.x += s1.x; y1.y += s1.y; y1.z += s1.z; y1.w += s1.w;
  }
  r0 = y0;
  r1 = y1;
}
__device__ __forceinline__ void comb_pair_any(const Comb& c, const float* cf, size_t off0, size_t off1, float4& r0, float4& r1) {
  switch (c.nk) {
    case 0: comb_pair<0>(c, cf, off0, off1, r0, r1); break;
    case 1: comb_pair<1>(c, cf, off0, off1, r0, r1); break;
    case 2: comb_pair<2>(c, cf, off0, off1, r0, r1); break;
    case 3: comb_pair<3>(c, cf, off0, off1, r0, r1); break;
    case 4: comb_pair<4>(c, cf, off0, off1, r0, r1); break;
    case 5: comb_pair<5>(c, cf, off0, off1, r0, r1); break;
    case 6: comb_pair<6>(c, cf, off0, off1, r0, r1); break;
    default: comb_pair<7>(c, cf, off0, off1, r0, r1); break;
  }
}

__global__ __launch_bounds__(256) void k_combine_gn(CombineGnArgs a, Dims d) {
  if (a.ctrl->done) return;   // a step enqueued past the end of the interval (see Ctrl)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x, c0 = blockIdx.y * d.cs;
  const int csl = min(d.cs, d.C - c0);
  const int cs4 = csl >> 2;
  const int nvec = d.HW * cs4;
  float* tile = smem;                      // [HW][csl]
  float* smean = smem + d.HW * d.cs;       // [cs/cpg]
  float* srstd = smean + d.cs;             // generous

  const float scale = comb_scale(a.comb, a.ctrl);
  float cf[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) cf[j] = scale * a.comb.coef[j];

  if ((nvec & 511) == 0) {   // two units per thread and round, all their requests in flight together
    for (int v = tid; v < nvec; v += 512) {
      const int p0 = v / cs4, q0 = v - p0 * cs4, p1 = (v + 256) / cs4, q1 = (v + 256) - p1 * cs4;
      const size_t off0 = ((size_t)(n * d.HW + p0)) * d.C + c0 + 4 * q0, off1 = ((size_t)(n * d.HW + p1)) * d.C + c0 + 4 * q1;
      float4 y0, y1;
      comb_pair_any(a.comb, cf, off0, off1, y0, y1);
      st4(tile + p0 * csl + 4 * q0, y0);
      st4(tile + p1 * csl + 4 * q1, y1);
      if (a.y_out) { st4(a.y_out + off0, y0); st4(a.y_out + off1, y1); }
    }
  } else
  for (int v = tid; v < nvec; v += 256) {
    const int p = v / cs4, q = v - p * cs4;
    const size_t off = ((size_t)(n * d.HW + p)) * d.C + c0 + 4 * q;
    float4 yv = ld4(a.comb.y + off);
    if (a.comb.nk > 0) {
      float4 s;
      {
        float4 kv = ld4(a.comb.k[0] + off);
        s.x = cf[0] * kv.x; s.y = cf[0] * kv.y; s.z = cf[0] * kv.z; s.w = cf[0] * kv.w;
      }
      for (int j = 1; j < a.comb.nk; ++j) {
        float4 kv = ld4(a.comb.k[j] + off);
        s.x += cf[j] * kv.x; s.y += cf[j] * kv.y; s.z += cf[j] * kv.z; s.w += cf[j] * kv.w;
      }
      yv.x += s.x; yv.y += s.y; yv.z += s.z; yv.w += s.w;
    }
    st4(tile + p * csl + 4 * q, yv);
    if (a.y_out) st4(a.y_out + off, yv);
  }
  __syncthreads();

  const int ngs = csl / d.cpg;
  const int m = d.HW * d.cpg;
  const float inv_m = 1.0f / (float)m;
  for (int gi = wave; gi < ngs; gi += 4) {
    float s = 0.f;
    for (int e = lane; e < m; e += 64) {
      const int p = e / d.cpg, cc = e - p * d.cpg;
      s += tile[p * csl + gi * d.cpg + cc];
    }
    const float mean = wave_sum(s) * inv_m;
    float s2 = 0.f;
    for (int e = lane; e < m; e += 64) {
      const int p = e / d.cpg, cc = e - p * d.cpg;
      const float dv = tile[p * csl + gi * d.cpg + cc] - mean;
      s2 += dv * dv;
    }
    const float var = wave_sum(s2) * inv_m;
    const float rstd = 1.0f / sqrtf(var + d.eps);
    if (lane == 0) {
      smean[gi] = mean;
      srstd[gi] = rstd;
      if (a.rstd_out) a.rstd_out[(size_t)n * d.G + c0 / d.cpg + gi] = rstd;
    }
  }
  __syncthreads();

  for (int v = tid; v < nvec; v += 256) {
    const int p = v / cs4, q = v - p * cs4;
    const size_t off = ((size_t)(n * d.HW + p)) * d.C + c0 + 4 * q;
    const float4 xv = ld4(tile + p * csl + 4 * q);
    const float4 gm = ld4(a.gamma + c0 + 4 * q);
    const float4 bt = ld4(a.beta + c0 + 4 * q);
    float x[4] = {xv.x, xv.y, xv.z, xv.w};
    float g[4] = {gm.x, gm.y, gm.z, gm.w};
    float b[4] = {bt.x, bt.y, bt.z, bt.w};
    float xh[4], o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gl = (4 * q + i) / d.cpg;
      xh[i] = (x[i] - smean[gl]) * srstd[gl];
      float vv = xh[i] * g[i] + b[i];
      if (a.relu) vv = fmaxf(vv, 0.f);
      o[i] = a.osign * vv;
    }
    if (a.act_out) st4(a.act_out + off, make_float4(o[0], o[1], o[2], o[3]));
    if (a.xhat_out) st4(a.xhat_out + off, make_float4(xh[0], xh[1], xh[2], xh[3]));
  }
}

void launch_combine_gn(const Dims& d, const CombineGnArgs& a, hipStream_t s) {
  size_t lds = ((size_t)d.HW * d.cs + 2 * (size_t)d.cs) * sizeof(float);
  hipLaunchKernelGGL(k_combine_gn, dim3(d.N, d.nslab), dim3(256), lds, s, a, d);
}

// ============================================================================
// Top of the backward chain: combine the adjoint state, negate it into the
// cotangent and push it through GroupNorm-3's backward.
//   g   = csign * (a + scale * sum coef_j k^a_j)
//   dz  = rstd * (g*gamma - mean(g*gamma) - xhat * mean(g*gamma*xhat))
//   per-sample partials of dgamma = sum g*xhat, dbeta = sum g
// ============================================================================
__global__ __launch_bounds__(256) void k_gn_bwd(GnBwdArgs a, Dims d) {
  if (a.ctrl->done) return;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x, c0 = blockIdx.y * d.cs;
  const int csl = min(d.cs, d.C - c0);
  const int cs4 = csl >> 2;
  const int nvec = d.HW * cs4;
  float* gt = smem;                           // [HW][csl]   g
  float* xt = gt + d.HW * d.cs;               // [HW][csl]   xhat
  float* sm1 = xt + d.HW * d.cs;              // [cs]
  float* sm2 = sm1 + d.cs;                    // [cs]
  unsigned char* flg = reinterpret_cast<unsigned char*>(sm2 + d.cs);   // [HW] border flags (rounded up to 16 B)
  float* cred = sm2 + d.cs + ((d.HW + 15) / 16) * 4;   // [256][2] channel partials
  float* red9 = cred + 512;                   // [9 * 256] masked column sums across pixel groups
  if (a.spart)
    for (int p = tid; p < d.HW; p += 256) {
      const int h = p / d.W, x = p - h * d.W;
      flg[p] = (unsigned char)((h == 0 ? 1 : 0) | (h == d.H - 1 ? 2 : 0) | (x == 0 ? 4 : 0) | (x == d.W - 1 ? 8 : 0));
    }

  const float scale = comb_scale(a.comb, a.ctrl);
  float cf[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) cf[j] = scale * a.comb.coef[j];

  if ((nvec & 511) == 0) {   // two units per thread and round, all their requests in flight together
    for (int v = tid; v < nvec; v += 512) {
      const int p0 = v / cs4, q0 = v - p0 * cs4, p1 = (v + 256) / cs4, q1 = (v + 256) - p1 * cs4;
      const size_t off0 = ((size_t)(n * d.HW + p0)) * d.C + c0 + 4 * q0, off1 = ((size_t)(n * d.HW + p1)) * d.C + c0 + 4 * q1;
      const float4 x0 = ld4(a.xhat + off0), x1 = ld4(a.xhat + off1);
      float4 m0 = make_float4(1.f, 1.f, 1.f, 1.f), m1 = m0;
      if (a.mask_act) { m0 = ld4(a.mask_act + off0); m1 = ld4(a.mask_act + off1); }
      float4 a0, a1;
      comb_pair_any(a.comb, cf, off0, off1, a0, a1);
      if (a.a_out) { st4(a.a_out + off0, a0); st4(a.a_out + off1, a1); }
      float4 g0 = make_float4(a.csign * a0.x, a.csign * a0.y, a.csign * a0.z, a.csign * a0.w);
      float4 g1 = make_float4(a.csign * a1.x, a.csign * a1.y, a.csign * a1.z, a.csign * a1.w);
      g0.x = m0.x > 0.f ? g0.x : 0.f; g0.y = m0.y > 0.f ? g0.y : 0.f; g0.z = m0.z > 0.f ? g0.z : 0.f; g0.w = m0.w > 0.f ? g0.w : 0.f;
      g1.x = m1.x > 0.f ? g1.x : 0.f; g1.y = m1.y > 0.f ? g1.y : 0.f; g1.z = m1.z > 0.f ? g1.z : 0.f; g1.w = m1.w > 0.f ? g1.w : 0.f;
      st4(gt + p0 * csl + 4 * q0, g0);
      st4(gt + p1 * csl + 4 * q1, g1);
      st4(xt + p0 * csl + 4 * q0, x0);
      st4(xt + p1 * csl + 4 * q1, x1);
    }
  } else
  for (int v = tid; v < nvec; v += 256) {
    const int p = v / cs4, q = v - p * cs4;
    const size_t off = ((size_t)(n * d.HW + p)) * d.C + c0 + 4 * q;
    float4 av = ld4(a.comb.y + off);
    if (a.comb.nk > 0) {
      float4 s;
      {
        float4 kv = ld4(a.comb.k[0] + off);
        s.x = cf[0] * kv.x; s.y = cf[0] * kv.y; s.z = cf[0] * kv.z; s.w = cf[0] * kv.w;
      }
      for (int j = 1; j < a.comb.nk; ++j) {
        float4 kv = ld4(a.comb.k[j] + off);
        s.x += cf[j] * kv.x; s.y += cf[j] * kv.y; s.z += cf[j] * kv.z; s.w += cf[j] * kv.w;
      }
      av.x += s.x; av.y += s.y; av.z += s.z; av.w += s.w;
    }
    if (a.a_out) st4(a.a_out + off, av);
    float4 gq = make_float4(a.csign * av.x, a.csign * av.y, a.csign * av.z, a.csign * av.w);
    if (a.mask_act) {
      const float4 mk = ld4(a.mask_act + off);
      gq.x = mk.x > 0.f ? gq.x : 0.f; gq.y = mk.y > 0.f ? gq.y : 0.f;
      gq.z = mk.z > 0.f ? gq.z : 0.f; gq.w = mk.w > 0.f ? gq.w : 0.f;
    }
    st4(gt + p * csl + 4 * q, gq);
    st4(xt + p * csl + 4 * q, ld4(a.xhat + off));
  }
  __syncthreads();

  // per-channel partial sums over the sample's pixels (dgamma, dbeta)
  {
    const int npg = csl <= 256 ? 256 / csl : 1;
    for (int cbase = 0; cbase < csl; cbase += 256) {
      const int cl = cbase + (tid % min(csl, 256));
      const int pg = tid / min(csl, 256);
      float dg = 0.f, db = 0.f;
      if (pg < npg && cl < csl) {
        for (int p = pg; p < d.HW; p += npg) {
          const float g = gt[p * csl + cl];
          dg += g * xt[p * csl + cl];
          db += g;
        }
      }
      cred[tid * 2] = dg;
      cred[tid * 2 + 1] = db;
      __syncthreads();
      if (pg == 0 && cl < csl) {
        const int stride = min(csl, 256);
        for (int r = 1; r < npg; ++r) {
          dg += cred[(r * stride + (tid % stride)) * 2];
          db += cred[(r * stride + (tid % stride)) * 2 + 1];
        }
        a.gpart[((size_t)n * 2 + 0) * d.C + c0 + cl] = dg;
        a.gpart[((size_t)n * 2 + 1) * d.C + c0 + cl] = db;
      }
      __syncthreads();
    }
  }

  const int ngs = csl / d.cpg;
  const int m = d.HW * d.cpg;
  const float inv_m = 1.0f / (float)m;
  for (int gi = wave; gi < ngs; gi += 4) {
    float s1 = 0.f, s2 = 0.f;
    for (int e = lane; e < m; e += 64) {
      const int p = e / d.cpg, cc = e - p * d.cpg;
      const int col = gi * d.cpg + cc;
      const float dxh = gt[p * csl + col] * a.gamma[c0 + col];
      s1 += dxh;
      s2 += dxh * xt[p * csl + col];
    }
    s1 = wave_sum(s1) * inv_m;
    s2 = wave_sum(s2) * inv_m;
    if (lane == 0) { sm1[gi] = s1; sm2[gi] = s2; }
  }
  __syncthreads();

  for (int v = tid; v < nvec; v += 256) {
    const int p = v / cs4, q = v - p * cs4;
    const size_t off = ((size_t)(n * d.HW + p)) * d.C + c0 + 4 * q;
    const float4 gv = ld4(gt + p * csl + 4 * q);
    const float4 xv = ld4(xt + p * csl + 4 * q);
    const float4 gm = ld4(a.gamma + c0 + 4 * q);
    float g[4] = {gv.x, gv.y, gv.z, gv.w};
    float x[4] = {xv.x, xv.y, xv.z, xv.w};
    float w[4] = {gm.x, gm.y, gm.z, gm.w};
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gl = (4 * q + i) / d.cpg;
      const float r = a.rstd[(size_t)n * d.G + c0 / d.cpg + gl];
      o[i] = a.osign * (r * (g[i] * w[i] - sm1[gl] - x[i] * sm2[gl]));
    }
    st4(a.dz_out + off, make_float4(o[0], o[1], o[2], o[3]));
    if (a.spart) st4(gt + p * csl + 4 * q, make_float4(o[0], o[1], o[2], o[3]));   // dz tile for the column sums below
  }
  if (a.spart) {   // masked column sums of this sample's dz slab while it is still in LDS (replaces a k_colsum launch)
    __syncthreads();
    for (int cbase = 0; cbase < csl; cbase += 256) {
      const int ncols = min(csl - cbase, 256);
      masked_colsum_tile(gt + cbase, csl, d.HW, flg, ncols, max(1, 256 / ncols), tid, red9,
                         a.spart + (size_t)n * 9 * d.C + c0 + cbase, d.C);
    }
  }
}

void launch_gn_bwd(const Dims& d, const GnBwdArgs& a, hipStream_t s) {
  size_t lds = (2 * (size_t)d.HW * d.cs + 2 * (size_t)d.cs + 512 + 9 * 256) * sizeof(float) + (size_t)d.HW + 16;
  hipLaunchKernelGGL(k_gn_bwd, dim3(d.N, d.nslab), dim3(256), lds, s, a, d);
}

}  // namespace node
