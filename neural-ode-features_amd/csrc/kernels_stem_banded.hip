// GroupNorm + ReLU passes of the residual stem for (sample, channel block) blocks that do not fit the LDS -- 64 x 64 images:
// 62 x 62 = 3844 pixels behind the first layer, where the resident backward of kernels_stem.hip would need 2 x 3844 x 8 x 4 B.
//   reference: model.py:284-310 (`relu(norm(x))` in front of every convolution of ResBlock), model.py:268-271 (GroupNorm(min(32, C), C)).
// A workgroup takes (sample, band of band_px consecutive pixels, CB channels) and keeps nothing of the tensor: at C = 64 = CB a band
// is ONE contiguous piece of band_px x 256 bytes, read with 16-byte requests, eight in flight per thread.  Each pass is two launches
// of the same grid N x bands x (C / CB); no workgroup waits for another one, nothing is added atomically, every sum has one order:
//   forward   k_stem_gnb_stats   per (band, group): mean and centred second moment of the band's cpg x pixels values (two reads of the
//                                band: sums, then squares around the band's own mean) -> fpart
//             k_stem_gnb_norm    every workgroup merges its groups' band partials with Chan's formula in band order (the same code on
//                                the same numbers in every workgroup of a sample: the same bits), band 0 writes `stats`; then
//                                relu(GN(h)) of its band -> triples
//   backward  k_stem_gnb_bsum    per (band, channel): sum dy and sum dy xhat, the ReLU mask recomputed from h and `stats` -> bpart
//             k_stem_gnb_dh      every workgroup adds its channels' band partials in band order, band 0 writes gpart; group sums
//                                s1, s2; dh of its band as fp32 and / or triples
// The pre-activation y = fma(xhat, gamma, beta) is ONE function (gnb_pre) for the forward's ReLU and both backward launches' masks.
// LDS: 4 - 9 KB per workgroup, whatever the image.  The second read of a band comes from L2 / Infinity Cache (supposed, not traced).
#include "stem.h"
#include "stem_split.h"

namespace node {

namespace {

constexpr int GNB_NB = 8;      // 16-byte requests in flight per thread
__device__ __forceinline__ int gnb_log2(int v) { return 31 - __clz(v); }
__device__ __forceinline__ float gnb_xhat(float h, float mean, float rstd) { return (h - mean) * rstd; }
__device__ __forceinline__ float gnb_pre(float xh, float gam, float bet) { return __builtin_fmaf(xh, gam, bet); }

struct GnbBlock { int n, band, c0, px0, npx; };
// blockIdx.x = (n * nbands + band) * (C / CB) + channel block
__device__ __forceinline__ GnbBlock gnb_block(const SGnBandArgs& a) {
  GnbBlock w;
  const int nblk = a.g.C / a.CB;
  int b = blockIdx.x;
  const int cb = b % nblk;
  b /= nblk;
  w.n = b / a.nbands;
  w.band = b - w.n * a.nbands;
  w.c0 = cb * a.CB;
  w.px0 = w.band * a.band_px;
  w.npx = min(a.band_px, a.g.HW - w.px0);      // >= 1: nbands = ceil(HW / band_px)
  return w;
}

// red [PL][CB] holds every thread's four channel sums (thread (pl, q) at red[pl * CB + 4 q]): chs[c] <- sum over pl in order, then
// grp[g] <- sum of the group's channels in order.  Three barriers; red, chs may be rewritten behind them.
__device__ __forceinline__ void gnb_group_sums(const float4& s, float* red, float* chs, float* grp, int CB, int PL, int cpg, int t) {
  *reinterpret_cast<float4*>(red + 4 * t) = s;
  __syncthreads();
  if (t < CB) {
    float v = 0.f;
    for (int j = 0; j < PL; ++j) v += red[j * CB + t];
    chs[t] = v;
  }
  __syncthreads();
  if (t < CB / cpg) {
    float v = 0.f;
    for (int k = 0; k < cpg; ++k) v += chs[t * cpg + k];
    grp[t] = v;
  }
  __syncthreads();
}

// thread -> four channels 4 q .. 4 q + 3 of the block (fixed), pixels pl, pl + PL, ... of the band
__global__ __launch_bounds__(256) void k_stem_gnb_stats(const SGnBandArgs a) {
  __shared__ __align__(16) float red[1024];
  __shared__ float chs[128];
  __shared__ float gsum[32];
  __shared__ float gsq[32];
  const int t = threadIdx.x;
  const GnbBlock w = gnb_block(a);
  const int CB = a.CB, C = a.g.C, lcb = gnb_log2(CB), lcpg = gnb_log2(a.g.cpg);
  const int q = t & ((CB >> 2) - 1), pl = t >> (lcb - 2), PL = 1024 >> lcb;
  const float* src = a.g.h + ((size_t)w.n * a.g.HW + w.px0) * C + w.c0 + 4 * q;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k0 = pl; k0 < w.npx; k0 += GNB_NB * PL) {
    float4 r[GNB_NB];
#pragma unroll
    for (int u = 0; u < GNB_NB; ++u) r[u] = *reinterpret_cast<const float4*>(src + (size_t)min(k0 + u * PL, w.npx - 1) * C);
#pragma unroll
    for (int u = 0; u < GNB_NB; ++u)
      if (k0 + u * PL < w.npx) { s.x += r[u].x; s.y += r[u].y; s.z += r[u].z; s.w += r[u].w; }
  }
  gnb_group_sums(s, red, chs, gsum, CB, PL, a.g.cpg, t);
  const float inv_m = 1.f / (float)(a.g.cpg * w.npx);
  const float m0 = gsum[(4 * q) >> lcpg] * inv_m, m1 = gsum[(4 * q + 1) >> lcpg] * inv_m, m2 = gsum[(4 * q + 2) >> lcpg] * inv_m,
              m3 = gsum[(4 * q + 3) >> lcpg] * inv_m;
  float4 s2 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k0 = pl; k0 < w.npx; k0 += GNB_NB * PL) {
    float4 r[GNB_NB];
#pragma unroll
    for (int u = 0; u < GNB_NB; ++u) r[u] = *reinterpret_cast<const float4*>(src + (size_t)min(k0 + u * PL, w.npx - 1) * C);
#pragma unroll
    for (int u = 0; u < GNB_NB; ++u)
      if (k0 + u * PL < w.npx) {
        const float d0 = r[u].x - m0, d1 = r[u].y - m1, d2 = r[u].z - m2, d3 = r[u].w - m3;
        s2.x = __builtin_fmaf(d0, d0, s2.x);
        s2.y = __builtin_fmaf(d1, d1, s2.y);
        s2.z = __builtin_fmaf(d2, d2, s2.z);
        s2.w = __builtin_fmaf(d3, d3, s2.w);
      }
  }
  gnb_group_sums(s2, red, chs, gsq, CB, PL, a.g.cpg, t);
  if (t < (CB >> lcpg)) {
    const int G = C >> lcpg;
    float* part = a.fpart + (((size_t)w.n * a.nbands + w.band) * G + (w.c0 >> lcpg) + t) * 2;
    part[0] = gsum[t] * inv_m;
    part[1] = gsq[t];
  }
}

// thread -> eight channels 8 q .. 8 q + 7 of the block (fixed), pixels t / (CB / 8), + 256 / (CB / 8), ... of the band
__global__ __launch_bounds__(256) void k_stem_gnb_norm(const SGnBandArgs a) {
  __shared__ float gmean[32];
  __shared__ float grstd[32];
  const int t = threadIdx.x;
  const GnbBlock w = gnb_block(a);
  const int CB = a.CB, C = a.g.C, HW = a.g.HW, lcb = gnb_log2(CB), lcpg = gnb_log2(a.g.cpg);
  const int G = C >> lcpg;
  if (t < (CB >> lcpg)) {
    // Chan's merge of the bands' (count, mean, M2) in band order; a band's count is cpg x its pixels
    const float* part = a.fpart + ((size_t)w.n * a.nbands * G + (w.c0 >> lcpg) + t) * 2;
    float cnt = 0.f, mean = 0.f, M2 = 0.f;
    for (int b0 = 0; b0 < a.nbands; b0 += GNB_NB) {
      float mb[GNB_NB], qb[GNB_NB];
#pragma unroll
      for (int u = 0; u < GNB_NB; ++u) {
        const float* p = part + (size_t)min(b0 + u, a.nbands - 1) * G * 2;
        mb[u] = p[0];
        qb[u] = p[1];
      }
#pragma unroll
      for (int u = 0; u < GNB_NB; ++u)
        if (b0 + u < a.nbands) {
          const float nb = (float)(a.g.cpg * min(a.band_px, HW - (b0 + u) * a.band_px));
          const float tot = cnt + nb, d = mb[u] - mean, f = nb / tot;
          mean += d * f;
          M2 += qb[u] + d * d * cnt * f;
          cnt = tot;
        }
    }
    const float rs = rsqrtf(M2 * (1.f / (float)(a.g.cpg * HW)) + a.g.eps);
    gmean[t] = mean;
    grstd[t] = rs;
    if (w.band == 0) {
      float* st = a.g.stats + ((size_t)w.n * G + (w.c0 >> lcpg) + t) * 2;
      st[0] = mean;
      st[1] = rs;
    }
  }
  __syncthreads();
  const int lq8 = lcb - 3, q = t & ((1 << lq8) - 1), pstep = 256 >> lq8;
  float gm[8], gr[8], ga[8], be[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int cc = 8 * q + k, g = cc >> lcpg;
    gm[k] = gmean[g];
    gr[k] = grstd[g];
    ga[k] = a.g.gamma[w.c0 + cc];
    be[k] = a.g.beta[w.c0 + cc];
  }
  const size_t row0 = (size_t)w.n * HW + w.px0;
  const float* src = a.g.h + row0 * C + w.c0 + 8 * q;
  bf16_t* dst = a.g.a3 + row0 * C + w.c0 + 8 * q;
  constexpr int NP = GNB_NB / 2;
  for (int k0 = t >> lq8; k0 < w.npx; k0 += NP * pstep) {
    float4 r0[NP], r1[NP];
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const float* p = src + (size_t)min(k0 + u * pstep, w.npx - 1) * C;
      r0[u] = *reinterpret_cast<const float4*>(p);
      r1[u] = *reinterpret_cast<const float4*>(p + 4);
    }
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const int px = k0 + u * pstep;
      if (px >= w.npx) continue;
      float v[8] = {r0[u].x, r0[u].y, r0[u].z, r0[u].w, r1[u].x, r1[u].y, r1[u].z, r1[u].w};
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = fmaxf(gnb_pre(gnb_xhat(v[k], gm[k], gr[k]), ga[k], be[k]), 0.f);
      u32x4 hh, mm, ll;
      split8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), hh, mm, ll);
      bf16_t* d = dst + (size_t)px * C;
      *reinterpret_cast<u32x4*>(d) = hh;
      *reinterpret_cast<u32x4*>(d + a.g.a_plane) = mm;
      *reinterpret_cast<u32x4*>(d + 2 * a.g.a_plane) = ll;
    }
  }
}

// backward: da = dL/d relu(GN(h)).  dy = da where the pre-activation is positive; dgamma_c = sum dy xhat, dbeta_c = sum dy;
// dh = rstd (dy gamma - (s1 + xhat s2) / m) with s1 = sum_group gamma dbeta, s2 = sum_group gamma dgamma  (as k_stem_gn_bwd)
__global__ __launch_bounds__(256) void k_stem_gnb_bsum(const SGnBandArgs a) {
  __shared__ __align__(16) float redA[1024];
  __shared__ __align__(16) float redB[1024];
  __shared__ float gmean[32];
  __shared__ float grstd[32];
  const int t = threadIdx.x;
  const GnbBlock w = gnb_block(a);
  const int CB = a.CB, C = a.g.C, lcb = gnb_log2(CB), lcpg = gnb_log2(a.g.cpg);
  const int G = C >> lcpg;
  if (t < (CB >> lcpg)) {
    const float* st = a.g.stats + ((size_t)w.n * G + (w.c0 >> lcpg) + t) * 2;
    gmean[t] = st[0];
    grstd[t] = st[1];
  }
  __syncthreads();
  const int q = t & ((CB >> 2) - 1), pl = t >> (lcb - 2), PL = 1024 >> lcb;
  float gm[4], gr[4], ga[4], be[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int cc = 4 * q + k, g = cc >> lcpg;
    gm[k] = gmean[g];
    gr[k] = grstd[g];
    ga[k] = a.g.gamma[w.c0 + cc];
    be[k] = a.g.beta[w.c0 + cc];
  }
  const size_t off = ((size_t)w.n * a.g.HW + w.px0) * C + w.c0 + 4 * q;
  const float* sh = a.g.h + off;
  const float* sd = a.g.da + off;
  float sA[4] = {0.f, 0.f, 0.f, 0.f}, sB[4] = {0.f, 0.f, 0.f, 0.f};
  constexpr int NP = GNB_NB / 2;
  for (int k0 = pl; k0 < w.npx; k0 += NP * PL) {
    float4 rh[NP], rd[NP];
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const size_t o = (size_t)min(k0 + u * PL, w.npx - 1) * C;
      rh[u] = *reinterpret_cast<const float4*>(sh + o);
      rd[u] = *reinterpret_cast<const float4*>(sd + o);
    }
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      if (k0 + u * PL >= w.npx) continue;
      const float hv[4] = {rh[u].x, rh[u].y, rh[u].z, rh[u].w}, dv[4] = {rd[u].x, rd[u].y, rd[u].z, rd[u].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float xh = gnb_xhat(hv[k], gm[k], gr[k]);
        const float dy = gnb_pre(xh, ga[k], be[k]) > 0.f ? dv[k] : 0.f;
        sA[k] += dy;
        sB[k] = __builtin_fmaf(dy, xh, sB[k]);
      }
    }
  }
  *reinterpret_cast<float4*>(redA + 4 * t) = make_float4(sA[0], sA[1], sA[2], sA[3]);      // red[pl * CB + 4 q]
  *reinterpret_cast<float4*>(redB + 4 * t) = make_float4(sB[0], sB[1], sB[2], sB[3]);
  __syncthreads();
  if (t < CB) {
    float A = 0.f, B = 0.f;
    for (int j = 0; j < PL; ++j) { A += redA[j * CB + t]; B += redB[j * CB + t]; }
    float* part = a.bpart + ((size_t)w.n * a.nbands + w.band) * 2 * C + w.c0 + t;
    part[0] = B;      // towards dgamma
    part[C] = A;      // towards dbeta
  }
}

__global__ __launch_bounds__(256) void k_stem_gnb_dh(const SGnBandArgs a) {
  __shared__ float chA[128];
  __shared__ float chB[128];
  __shared__ float gmean[32];
  __shared__ float grstd[32];
  __shared__ float gs1[32];
  __shared__ float gs2[32];
  const int t = threadIdx.x;
  const GnbBlock w = gnb_block(a);
  const int CB = a.CB, C = a.g.C, HW = a.g.HW, lcb = gnb_log2(CB), lcpg = gnb_log2(a.g.cpg);
  const int G = C >> lcpg, ngrp = CB >> lcpg;
  if (t < CB) {
    // the channel's band partials in band order
    const float* part = a.bpart + (size_t)w.n * a.nbands * 2 * C + w.c0 + t;
    float A = 0.f, B = 0.f;
    for (int b0 = 0; b0 < a.nbands; b0 += GNB_NB) {
      float xa[GNB_NB], xb[GNB_NB];
#pragma unroll
      for (int u = 0; u < GNB_NB; ++u) {
        const float* p = part + (size_t)min(b0 + u, a.nbands - 1) * 2 * C;
        xb[u] = p[0];
        xa[u] = p[C];
      }
#pragma unroll
      for (int u = 0; u < GNB_NB; ++u)
        if (b0 + u < a.nbands) { A += xa[u]; B += xb[u]; }
    }
    if (w.band == 0) {
      a.g.gpart[((size_t)w.n * 2 + 0) * C + w.c0 + t] = B;      // dgamma
      a.g.gpart[((size_t)w.n * 2 + 1) * C + w.c0 + t] = A;      // dbeta
    }
    const float gam = a.g.gamma[w.c0 + t];
    chA[t] = A * gam;
    chB[t] = B * gam;
  }
  if (t < ngrp) {
    const float* st = a.g.stats + ((size_t)w.n * G + (w.c0 >> lcpg) + t) * 2;
    gmean[t] = st[0];
    grstd[t] = st[1];
  }
  __syncthreads();
  if (t < ngrp) {
    float s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < a.g.cpg; ++k) { s1 += chA[t * a.g.cpg + k]; s2 += chB[t * a.g.cpg + k]; }
    gs1[t] = s1;
    gs2[t] = s2;
  }
  __syncthreads();
  const float inv_m = 1.f / (float)(a.g.cpg * HW);
  const int lq8 = lcb - 3, q = t & ((1 << lq8) - 1), pstep = 256 >> lq8;
  float gm[8], gr[8], ga[8], be[8], g1[8], g2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int cc = 8 * q + k, g = cc >> lcpg;
    gm[k] = gmean[g];
    gr[k] = grstd[g];
    ga[k] = a.g.gamma[w.c0 + cc];
    be[k] = a.g.beta[w.c0 + cc];
    g1[k] = gs1[g];
    g2[k] = gs2[g];
  }
  const size_t off = ((size_t)w.n * HW + w.px0) * C + w.c0 + 8 * q;
  const float* sh = a.g.h + off;
  const float* sd = a.g.da + off;
  constexpr int NP = GNB_NB / 4;
  for (int k0 = t >> lq8; k0 < w.npx; k0 += NP * pstep) {
    float4 rh[NP][2], rd[NP][2];
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const size_t o = (size_t)min(k0 + u * pstep, w.npx - 1) * C;
      rh[u][0] = *reinterpret_cast<const float4*>(sh + o);
      rh[u][1] = *reinterpret_cast<const float4*>(sh + o + 4);
      rd[u][0] = *reinterpret_cast<const float4*>(sd + o);
      rd[u][1] = *reinterpret_cast<const float4*>(sd + o + 4);
    }
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const int px = k0 + u * pstep;
      if (px >= w.npx) continue;
      const float hv[8] = {rh[u][0].x, rh[u][0].y, rh[u][0].z, rh[u][0].w, rh[u][1].x, rh[u][1].y, rh[u][1].z, rh[u][1].w};
      const float dv[8] = {rd[u][0].x, rd[u][0].y, rd[u][0].z, rd[u][0].w, rd[u][1].x, rd[u][1].y, rd[u][1].z, rd[u][1].w};
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float xh = gnb_xhat(hv[k], gm[k], gr[k]);
        const float dy = gnb_pre(xh, ga[k], be[k]) > 0.f ? dv[k] : 0.f;
        v[k] = gr[k] * (dy * ga[k] - (g1[k] + xh * g2[k]) * inv_m);
      }
      const size_t o = off + (size_t)px * C;
      const float4 p0 = make_float4(v[0], v[1], v[2], v[3]), p1 = make_float4(v[4], v[5], v[6], v[7]);
      if (a.g.dh) {
        *reinterpret_cast<float4*>(a.g.dh + o) = p0;
        *reinterpret_cast<float4*>(a.g.dh + o + 4) = p1;
      }
      if (a.g.dh3) {
        u32x4 hh, mm, ll;
        split8(p0, p1, hh, mm, ll);
        *reinterpret_cast<u32x4*>(a.g.dh3 + o) = hh;
        *reinterpret_cast<u32x4*>(a.g.dh3 + o + a.g.dh_plane) = mm;
        *reinterpret_cast<u32x4*>(a.g.dh3 + o + 2 * a.g.dh_plane) = ll;
      }
    }
  }
}

}  // namespace

// The banded passes' channel block: 64 channels = one 256-byte line of every pixel, or one whole group where a group is wider
// (filters = 4096: 128 channels per group).  C and cpg are powers of two, C >= 64 (the stem's plan admits nothing else), so the block
// divides C, holds whole groups -- at most 32 of them -- and the kernels' index arithmetic is shifts.
int stem_gn_band_cb(int C, int cpg) {
  int cb = 64;
  while (cb < cpg) cb *= 2;
  return cb;
}

void launch_stem_gn_banded_fwd(const SGnBandArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)a.g.N * a.nbands * (a.g.C / a.CB));
  hipLaunchKernelGGL(k_stem_gnb_stats, grid, dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_stem_gnb_norm, grid, dim3(256), 0, s, a);
}
void launch_stem_gn_banded_bwd(const SGnBandArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)a.g.N * a.nbands * (a.g.C / a.CB));
  hipLaunchKernelGGL(k_stem_gnb_bsum, grid, dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_stem_gnb_dh, grid, dim3(256), 0, s, a);
}

}  // namespace node
