// Kernels of the `minimal` stem (ministem.h): 24-channel convolutions and GroupNorm(24, 24) passes in fp32 on NHWC tensors of
// channel pitch 24.  Register tiles: a thread owns one pixel and 8 to 32 channels of the tensor it writes -- few enough that a
// batch of 128 fills the chip with waves -- and the filter block sits in LDS, read as wave-uniform 16-byte words.  Every sum
// has a fixed order: no atomics, the same bits run to run.
#include "ministem.h"

namespace node {

namespace {

constexpr int C = MINI_C;
constexpr int COB = MINI_COB;
constexpr int FCO = MINI_FCO;                 // output channels per thread of the forward 4x4 convolution
constexpr int CQ = C / 4;                    // 16-byte channel quads of a pixel

// sum over the 256 threads of a workgroup, per component, as a fixed tree; every thread gets the same bits
__device__ inline float4 block_sum4(float4* red, float4 v) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      const float4 a = red[t], b = red[t + w];
      red[t] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
    __syncthreads();
  }
  return red[0];
}

// first layer: thread = one output pixel x its 24 channels; the filter [9 Cin][24] and the bias in LDS
__global__ __launch_bounds__(256) void k_mini_conv0_fwd(const float* __restrict__ x, const float* __restrict__ w0, const float* __restrict__ b0,
                                                        float* __restrict__ h0, int R, int Cin, int H, int W) {
  __shared__ float4 ws[28 * CQ];
  float* wsf = reinterpret_cast<float*>(ws);
  const int t = threadIdx.x, K = 9 * Cin;
  for (int idx = t; idx < 28 * C; idx += 256) {
    const int k = idx / C, c = idx - k * C;
    wsf[idx] = k < K ? w0[c * K + k] : (k == 27 ? b0[c] : 0.f);
  }
  __syncthreads();
  const int r = blockIdx.x * 256 + t;
  if (r >= R) return;
  const int H0 = H - 2, W0 = W - 2, HW0 = H0 * W0, n = r / HW0, p = r - n * HW0, y = p / W0, xx = p - y * W0;
  float acc[C];
#pragma unroll
  for (int q = 0; q < CQ; ++q) {
    const float4 b = ws[27 * CQ + q];
    acc[q * 4] = b.x; acc[q * 4 + 1] = b.y; acc[q * 4 + 2] = b.z; acc[q * 4 + 3] = b.w;
  }
  const float* xp = x + ((size_t)n * Cin * H + y) * W + xx;
  for (int ci = 0; ci < Cin; ++ci)
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float v = xp[((size_t)ci * H + k / 3) * W + k % 3];
      const float4* wr = ws + (ci * 9 + k) * CQ;
#pragma unroll
      for (int q = 0; q < CQ; ++q) {
        const float4 ww = wr[q];
        acc[q * 4 + 0] += v * ww.x;
        acc[q * 4 + 1] += v * ww.y;
        acc[q * 4 + 2] += v * ww.z;
        acc[q * 4 + 3] += v * ww.w;
      }
    }
  float4* op = reinterpret_cast<float4*>(h0 + (size_t)r * C);
#pragma unroll
  for (int q = 0; q < CQ; ++q) op[q] = make_float4(acc[q * 4], acc[q * 4 + 1], acc[q * 4 + 2], acc[q * 4 + 3]);
}

// GroupNorm(24, 24) + ReLU: one workgroup per (sample, channel quad); two-pass statistics of the four planes, then the apply
__global__ __launch_bounds__(256) void k_mini_gn_fwd(const float* __restrict__ h, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float* __restrict__ a, float* __restrict__ stats, int HW, float eps) {
  __shared__ float4 red[256];
  const int n = blockIdx.x, q = blockIdx.y, t = threadIdx.x;
  const float* hn = h + (size_t)n * HW * C + 4 * q;
  float* an = a + (size_t)n * HW * C + 4 * q;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = t; p < HW; p += 256) {
    const float4 v = *reinterpret_cast<const float4*>(hn + (size_t)p * C);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  const float4 S = block_sum4(red, s);
  const float inv = 1.0f / (float)HW;
  const float4 mean = make_float4(S.x * inv, S.y * inv, S.z * inv, S.w * inv);
  s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = t; p < HW; p += 256) {
    const float4 v = *reinterpret_cast<const float4*>(hn + (size_t)p * C);
    const float dx = v.x - mean.x, dy = v.y - mean.y, dz = v.z - mean.z, dw = v.w - mean.w;
    s.x += dx * dx; s.y += dy * dy; s.z += dz * dz; s.w += dw * dw;
  }
  const float4 Q = block_sum4(red, s);
  const float4 rstd = make_float4(1.0f / sqrtf(Q.x * inv + eps), 1.0f / sqrtf(Q.y * inv + eps), 1.0f / sqrtf(Q.z * inv + eps),
                                  1.0f / sqrtf(Q.w * inv + eps));
  if (t == 0) {
    float* st = stats + ((size_t)n * C + 4 * q) * 2;
    st[0] = mean.x; st[1] = rstd.x; st[2] = mean.y; st[3] = rstd.y; st[4] = mean.z; st[5] = rstd.z; st[6] = mean.w; st[7] = rstd.w;
  }
  const float4 g = *reinterpret_cast<const float4*>(gamma + 4 * q), b = *reinterpret_cast<const float4*>(beta + 4 * q);
  for (int p = t; p < HW; p += 256) {
    const float4 v = *reinterpret_cast<const float4*>(hn + (size_t)p * C);
    float4 o;
    o.x = fmaxf((v.x - mean.x) * rstd.x * g.x + b.x, 0.f);
    o.y = fmaxf((v.y - mean.y) * rstd.y * g.y + b.y, 0.f);
    o.z = fmaxf((v.z - mean.z) * rstd.z * g.z + b.z, 0.f);
    o.w = fmaxf((v.w - mean.w) * rstd.w * g.w + b.w, 0.f);
    *reinterpret_cast<float4*>(an + (size_t)p * C) = o;
  }
}

// its backward, in place on d (the activation's gradient in, the gradient of h out); same workgroups
__global__ __launch_bounds__(256) void k_mini_gn_bwd(const float* __restrict__ h, const float* __restrict__ a, const float* __restrict__ gamma,
                                                     const float* __restrict__ stats, float* __restrict__ d, float* __restrict__ gpart,
                                                     float* __restrict__ bpart, int HW) {
  __shared__ float4 red[256];
  const int n = blockIdx.x, q = blockIdx.y, t = threadIdx.x;
  const size_t base = (size_t)n * HW * C + 4 * q;
  const float* hn = h + base;
  const float* an = a + base;
  float* dn = d + base;
  const float* st = stats + ((size_t)n * C + 4 * q) * 2;
  const float4 mean = make_float4(st[0], st[2], st[4], st[6]), rstd = make_float4(st[1], st[3], st[5], st[7]);
  float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
  for (int p = t; p < HW; p += 256) {
    const float4 hv = *reinterpret_cast<const float4*>(hn + (size_t)p * C), av = *reinterpret_cast<const float4*>(an + (size_t)p * C);
    float4 g = *reinterpret_cast<const float4*>(dn + (size_t)p * C);
    g.x = av.x > 0.f ? g.x : 0.f; g.y = av.y > 0.f ? g.y : 0.f; g.z = av.z > 0.f ? g.z : 0.f; g.w = av.w > 0.f ? g.w : 0.f;
    s1.x += g.x; s1.y += g.y; s1.z += g.z; s1.w += g.w;
    s2.x += g.x * ((hv.x - mean.x) * rstd.x); s2.y += g.y * ((hv.y - mean.y) * rstd.y);
    s2.z += g.z * ((hv.z - mean.z) * rstd.z); s2.w += g.w * ((hv.w - mean.w) * rstd.w);
  }
  const float4 S1 = block_sum4(red, s1);
  const float4 S2 = block_sum4(red, s2);
  if (t == 0) {
    *reinterpret_cast<float4*>(gpart + (size_t)n * 2 * C + 4 * q) = S2;          // dgamma
    *reinterpret_cast<float4*>(gpart + (size_t)n * 2 * C + C + 4 * q) = S1;      // dbeta
  }
  const float inv = 1.0f / (float)HW;
  const float4 gm = *reinterpret_cast<const float4*>(gamma + 4 * q);
  const float4 k = make_float4(gm.x * rstd.x, gm.y * rstd.y, gm.z * rstd.z, gm.w * rstd.w);
  const float4 m1 = make_float4(S1.x * inv, S1.y * inv, S1.z * inv, S1.w * inv), m2 = make_float4(S2.x * inv, S2.y * inv, S2.z * inv, S2.w * inv);
  float4 sb = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = t; p < HW; p += 256) {
    const float4 hv = *reinterpret_cast<const float4*>(hn + (size_t)p * C), av = *reinterpret_cast<const float4*>(an + (size_t)p * C);
    float4 g = *reinterpret_cast<const float4*>(dn + (size_t)p * C);
    g.x = av.x > 0.f ? g.x : 0.f; g.y = av.y > 0.f ? g.y : 0.f; g.z = av.z > 0.f ? g.z : 0.f; g.w = av.w > 0.f ? g.w : 0.f;
    float4 o;
    o.x = k.x * (g.x - m1.x - ((hv.x - mean.x) * rstd.x) * m2.x);
    o.y = k.y * (g.y - m1.y - ((hv.y - mean.y) * rstd.y) * m2.y);
    o.z = k.z * (g.z - m1.z - ((hv.z - mean.z) * rstd.z) * m2.z);
    o.w = k.w * (g.w - m1.w - ((hv.w - mean.w) * rstd.w) * m2.w);
    *reinterpret_cast<float4*>(dn + (size_t)p * C) = o;
    sb.x += o.x; sb.y += o.y; sb.z += o.z; sb.w += o.w;
  }
  const float4 SB = block_sum4(red, sb);
  if (t == 0) *reinterpret_cast<float4*>(bpart + (size_t)n * C + 4 * q) = SB;
}

// ----------------------------------------------------------------------------------------------------------------
// Conv2d(24, Cout, 4, 2, 1): thread = one output pixel x 32 output channels; filter block [16][24][32] in LDS
// ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mini_conv4_fwd(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ out, int R, int IH, int IW, int OH, int OW, int Cout, int nchw) {
  __shared__ float4 ws[16 * C * FCO / 4];
  float* wsf = reinterpret_cast<float*>(ws);
  const int t = threadIdx.x, co0 = blockIdx.y * FCO;      // (Cout % FCO == 0: 24, and the powers of two from 64)
  for (int idx = t; idx < 16 * C * FCO; idx += 256) {
    const int j = idx % FCO, ci = (idx / FCO) % C, tap = idx / (FCO * C);
    wsf[idx] = w[((size_t)(co0 + j) * C + ci) * 16 + tap];
  }
  __syncthreads();
  const int r = blockIdx.x * 256 + t;
  if (r >= R) return;
  const int OHW = OH * OW, n = r / OHW, p = r - n * OHW, oy = p / OW, ox = p - oy * OW;
  float acc[FCO];
#pragma unroll
  for (int j = 0; j < FCO; ++j) acc[j] = bias[co0 + j];
  for (int ky = 0; ky < 4; ++ky) {
    const int iy = 2 * oy - 1 + ky;
    if (iy < 0 || iy >= IH) continue;
    for (int kx = 0; kx < 4; ++kx) {
      const int ix = 2 * ox - 1 + kx;
      if (ix < 0 || ix >= IW) continue;
      const float4* ip = reinterpret_cast<const float4*>(in + (((size_t)n * IH + iy) * IW + ix) * C);
      const float4* wt = ws + (ky * 4 + kx) * C * FCO / 4;
#pragma unroll
      for (int q = 0; q < CQ; ++q) {
        const float4 v4 = ip[q];
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float4* wr = wt + (q * 4 + e) * FCO / 4;
#pragma unroll
          for (int j4 = 0; j4 < FCO / 4; ++j4) {
            const float4 ww = wr[j4];
            acc[j4 * 4 + 0] += v[e] * ww.x;
            acc[j4 * 4 + 1] += v[e] * ww.y;
            acc[j4 * 4 + 2] += v[e] * ww.z;
            acc[j4 * 4 + 3] += v[e] * ww.w;
          }
        }
      }
    }
  }
  if (nchw) {
#pragma unroll
    for (int j = 0; j < FCO; ++j) out[((size_t)n * Cout + co0 + j) * OHW + p] = acc[j];
  } else {     // pitch 24: Cout == 24
    float4* op = reinterpret_cast<float4*>(out + (size_t)r * C + co0);
#pragma unroll
    for (int q = 0; q < FCO / 4; ++q) op[q] = make_float4(acc[q * 4], acc[q * 4 + 1], acc[q * 4 + 2], acc[q * 4 + 3]);
  }
}

// data gradient: thread = one pixel of the convolution's INPUT x eight of its 24 channels (blockIdx.y: which eight); of the 16
// taps the four of the pixel's (row parity, column parity) class reach it.  The reduction over Cout runs in blocks of 32 through
// LDS [16][32][8] (+ 8 floats a tap: the four taps a wave reads at once lie in different banks)
constexpr int DCI = 8;
constexpr int DG_TAP = COB * DCI + 8;
__global__ __launch_bounds__(256) void k_mini_conv4_dgrad(const MiniDy dy, const float* __restrict__ w, float* __restrict__ d_in, int R,
                                                          int IH, int IW, int OH, int OW, int Cout) {
  __shared__ float4 ws[16 * DG_TAP / 4];
  float* wsf = reinterpret_cast<float*>(ws);
  const int t = threadIdx.x, ci0 = blockIdx.y * DCI;
  const int r = blockIdx.x * 256 + t;
  const bool valid = r < R;
  const int IHW = IH * IW, n = valid ? r / IHW : 0, p = valid ? r - n * IHW : 0, iy = p / IW, ix = p - iy * IW;
  // taps ky = ky0, ky0 + 2 with oy = (iy + 1 - ky) / 2
  const int ky0 = (iy + 1) & 1, kx0 = (ix + 1) & 1;
  float acc[DCI];
#pragma unroll
  for (int i = 0; i < DCI; ++i) acc[i] = 0.f;
  for (int c0 = 0; c0 < Cout; c0 += COB) {
    __syncthreads();
    for (int idx = t; idx < 16 * COB * DCI; idx += 256) {
      const int ci = idx % DCI, j = (idx / DCI) % COB, tap = idx / (DCI * COB), co = c0 + j;
      wsf[tap * DG_TAP + j * DCI + ci] = co < Cout ? w[((size_t)co * C + ci0 + ci) * 16 + tap] : 0.f;
    }
    __syncthreads();
    if (!valid) continue;
    const int nco = Cout - c0 < COB ? Cout - c0 : COB;
    for (int a = 0; a < 2; ++a) {
      const int ky = ky0 + 2 * a, oy = (iy + 1 - ky) / 2;
      if (iy + 1 - ky < 0 || oy >= OH) continue;
      for (int b = 0; b < 2; ++b) {
        const int kx = kx0 + 2 * b, ox = (ix + 1 - kx) / 2;
        if (ix + 1 - kx < 0 || ox >= OW) continue;
        const float* gp = dy.p + (size_t)n * dy.sn + (size_t)c0 * dy.sc + (size_t)(oy * OW + ox) * dy.sp;
        const float4* wt = ws + (ky * 4 + kx) * DG_TAP / 4;
        // the block's 32 output gradients first, as independent loads in flight (past Cout: channel 0 again, against zero filters)
        float gv[COB];
#pragma unroll
        for (int j = 0; j < COB; ++j) gv[j] = gp[(size_t)(j < nco ? j : 0) * dy.sc];
#pragma unroll
        for (int j = 0; j < COB; ++j) {
          const float g = gv[j];
          const float4 w0 = wt[j * 2], w1 = wt[j * 2 + 1];
          acc[0] += g * w0.x; acc[1] += g * w0.y; acc[2] += g * w0.z; acc[3] += g * w0.w;
          acc[4] += g * w1.x; acc[5] += g * w1.y; acc[6] += g * w1.z; acc[7] += g * w1.w;
        }
      }
    }
  }
  if (!valid) return;
  float4* op = reinterpret_cast<float4*>(d_in + (size_t)r * C + ci0);
  op[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
  op[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

// weight gradient: thread = one (tap, input channel) x 32 output channels, over the rows of one split; the rows' output
// gradients go through LDS 32 at a time with the rows' gather bases
constexpr int WG_RC = 32;
__global__ __launch_bounds__(384) void k_mini_conv4_wgrad(const MiniDy dy, const float* __restrict__ in, float* __restrict__ slab, int R,
                                                          int IH, int IW, int OH, int OW, int Cout, int rps) {
  __shared__ float4 gt[WG_RC * COB / 4];
  __shared__ int rbase[WG_RC];
  __shared__ unsigned rmask[WG_RC];
  float* gtf = reinterpret_cast<float*>(gt);
  const int t = threadIdx.x, tap = t / C, ci = t - tap * C, ky = tap >> 2, kx = tap & 3;
  const int co0 = blockIdx.y * COB, OHW = OH * OW;
  const int r0 = blockIdx.x * rps, r1 = r0 + rps < R ? r0 + rps : R;
  const int toff = (ky * IW + kx) * C + ci;
  float acc[COB];
#pragma unroll
  for (int j = 0; j < COB; ++j) acc[j] = 0.f;
  for (int rc = r0; rc < r1; rc += WG_RC) {
    __syncthreads();
    for (int idx = t; idx < WG_RC * COB; idx += 384) {
      int rr, j;
      if (dy.sc == 1) { j = idx % COB; rr = idx / COB; } else { rr = idx % WG_RC; j = idx / WG_RC; }
      const int r = rc + rr, co = co0 + j;
      float v = 0.f;
      if (r < r1 && co < Cout) {
        const int n = r / OHW, p = r - n * OHW;
        v = dy.p[(size_t)n * dy.sn + (size_t)co * dy.sc + (size_t)p * dy.sp];
      }
      gtf[rr * COB + j] = v;
    }
    if (t < WG_RC) {
      const int r = rc + t;
      unsigned m = 0;
      int base = 0;
      if (r < r1) {
        const int n = r / OHW, p = r - n * OHW, oy = p / OW, ox = p - oy * OW;
        base = ((n * IH + 2 * oy - 1) * IW + 2 * ox - 1) * C;
        for (int a = 0; a < 4; ++a)
          for (int b = 0; b < 4; ++b) {
            const int iy = 2 * oy - 1 + a, ix = 2 * ox - 1 + b;
            if (iy >= 0 && iy < IH && ix >= 0 && ix < IW) m |= 1u << (a * 4 + b);
          }
      }
      rbase[t] = base;
      rmask[t] = m;
    }
    __syncthreads();
    const int nr = r1 - rc < WG_RC ? r1 - rc : WG_RC;
    for (int rr = 0; rr < nr; ++rr) {
      if (!((rmask[rr] >> tap) & 1u)) continue;
      const float v = in[rbase[rr] + toff];
      const float4* gr = gt + rr * COB / 4;
#pragma unroll
      for (int j4 = 0; j4 < COB / 4; ++j4) {
        const float4 g = gr[j4];
        acc[j4 * 4 + 0] += v * g.x;
        acc[j4 * 4 + 1] += v * g.y;
        acc[j4 * 4 + 2] += v * g.z;
        acc[j4 * 4 + 3] += v * g.w;
      }
    }
  }
  float* sl = slab + (size_t)blockIdx.x * Cout * C * 16;
#pragma unroll
  for (int j = 0; j < COB; ++j)
    if (co0 + j < Cout) sl[((size_t)(co0 + j) * C + ci) * 16 + tap] = acc[j];
}

// ----------------------------------------------------------------------------------------------------------------
// the first layer's gradients
// ----------------------------------------------------------------------------------------------------------------
// weight gradient per (sample, kernel row ky): thread = (pixel slot, output channel) with the row's 3 Cin taps as accumulators;
// the ten slots are added in slot order
constexpr int W0_SLOTS = 10;
__global__ __launch_bounds__(256) void k_mini_conv0_wgrad(const float* __restrict__ x, const float* __restrict__ dh0, float* __restrict__ slab,
                                                          int Cin, int H, int W) {
  __shared__ float red[W0_SLOTS * 9 * C];
  const int n = blockIdx.x, ky = blockIdx.y, t = threadIdx.x, co = t % C, slot = t / C;
  const int K = 9 * Cin, H0 = H - 2, W0 = W - 2, HW0 = H0 * W0;
  const float* xn = x + (size_t)n * Cin * H * W + (size_t)ky * W;
  const float* dn = dh0 + (size_t)n * HW0 * C + co;
  float acc[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) acc[i] = 0.f;
  if (slot < W0_SLOTS) {
    for (int p = slot; p < HW0; p += W0_SLOTS) {
      const int y = p / W0, xx = p - y * W0;
      const float d = dn[(size_t)p * C];
      const float* xp = xn + y * W + xx;
#pragma unroll
      for (int ci = 0; ci < 3; ++ci)
        if (ci < Cin) {
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) acc[ci * 3 + kx] += d * xp[(size_t)ci * H * W + kx];
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) red[(slot * 9 + i) * C + co] = acc[i];
  }
  __syncthreads();
  if (t < 9 * C) {
    const int i = t / C, c = t - i * C, ci = i / 3, kx = i - ci * 3;
    if (ci < Cin) {
      float s = 0.f;
      for (int k = 0; k < W0_SLOTS; ++k) s += red[(k * 9 + i) * C + c];
      slab[((size_t)n * C + c) * K + ci * 9 + ky * 3 + kx] = s;
    }
  }
}

__global__ __launch_bounds__(256) void k_mini_conv0_dgrad(const float* __restrict__ dh0, const float* __restrict__ w0, float* __restrict__ dx,
                                                          int R, int Cin, int H, int W) {
  __shared__ float4 ws[9 * C];      // [tap][co] -> (ci 0, 1, 2, -)
  const int t = threadIdx.x;
  for (int idx = t; idx < 9 * C; idx += 256) {
    const int tap = idx / C, co = idx - tap * C;
    float v[3];
    for (int ci = 0; ci < 3; ++ci) v[ci] = ci < Cin ? w0[((size_t)co * Cin + ci) * 9 + tap] : 0.f;
    ws[idx] = make_float4(v[0], v[1], v[2], 0.f);
  }
  __syncthreads();
  const int r = blockIdx.x * 256 + t;
  if (r >= R) return;
  const int HW = H * W, H0 = H - 2, W0 = W - 2, n = r / HW, p = r - n * HW, y = p / W, xx = p - y * W;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int ky = 0; ky < 3; ++ky) {
    const int yy = y - ky;
    if (yy < 0 || yy >= H0) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int xs = xx - kx;
      if (xs < 0 || xs >= W0) continue;
      const float4* dp = reinterpret_cast<const float4*>(dh0 + (((size_t)n * H0 + yy) * W0 + xs) * C);
      const float4* wt = ws + (ky * 3 + kx) * C;
#pragma unroll
      for (int q = 0; q < C / 4; ++q) {
        const float4 d4 = dp[q];
        const float d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float4 ww = wt[q * 4 + e];
          a0 += d[e] * ww.x;
          a1 += d[e] * ww.y;
          a2 += d[e] * ww.z;
        }
      }
    }
  }
  float* o = dx + (size_t)n * Cin * HW + p;
  o[0] = a0;
  if (Cin > 1) o[HW] = a1;
  if (Cin > 2) o[2 * (size_t)HW] = a2;
}

// ----------------------------------------------------------------------------------------------------------------
// sums
// ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mini_chansum(const float* __restrict__ g, float* __restrict__ db, int N, int Cn, int HW) {
  __shared__ float red[256];
  const int c = blockIdx.x, t = threadIdx.x, total = N * HW;
  float s = 0.f;
  for (int i = t; i < total; i += 256) {
    const int n = i / HW, p = i - n * HW;
    s += g[((size_t)n * Cn + c) * HW + p];
  }
  red[t] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) db[c] = red[0];
}

__global__ __launch_bounds__(256) void k_mini_sums(const MiniSumArgs a) {
  const MiniSumJob j = a.job[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= j.count) return;
  float s = 0.f;
  for (int k = 0; k < j.ns; ++k) s += j.src[(size_t)k * j.stride + i];
  j.out[i] = s;
}

}  // namespace

void launch_mini_conv0_fwd(const float* x, const float* w0, const float* b0, float* h0, int N, int Cin, int H, int W, hipStream_t s) {
  const int R = N * (H - 2) * (W - 2);
  hipLaunchKernelGGL(k_mini_conv0_fwd, dim3((R + 255) / 256), dim3(256), 0, s, x, w0, b0, h0, R, Cin, H, W);
}
void launch_mini_gn_fwd(const float* h, const float* gamma, const float* beta, float* a, float* stats, int N, int HW, float eps, hipStream_t s) {
  hipLaunchKernelGGL(k_mini_gn_fwd, dim3(N, CQ), dim3(256), 0, s, h, gamma, beta, a, stats, HW, eps);
}
void launch_mini_conv4_fwd(const float* in, const float* w, const float* bias, float* out, int N, int IH, int IW, int OH, int OW, int Cout,
                           int nchw, hipStream_t s) {
  const int R = N * OH * OW;
  hipLaunchKernelGGL(k_mini_conv4_fwd, dim3((R + 255) / 256, Cout / FCO), dim3(256), 0, s, in, w, bias, out, R, IH, IW, OH, OW,
                     Cout, nchw);
}
void launch_mini_conv4_dgrad(MiniDy dy, const float* w, float* d_in, int N, int IH, int IW, int OH, int OW, int Cout, hipStream_t s) {
  const int R = N * IH * IW;
  hipLaunchKernelGGL(k_mini_conv4_dgrad, dim3((R + 255) / 256, C / DCI), dim3(256), 0, s, dy, w, d_in, R, IH, IW, OH, OW, Cout);
}
void launch_mini_conv4_wgrad(MiniDy dy, const float* in, float* slab, int N, int IH, int IW, int OH, int OW, int Cout, int nsplit,
                             int rows_per_split, hipStream_t s) {
  hipLaunchKernelGGL(k_mini_conv4_wgrad, dim3(nsplit, (Cout + COB - 1) / COB), dim3(384), 0, s, dy, in, slab, N * OH * OW, IH, IW, OH, OW,
                     Cout, rows_per_split);
}
void launch_mini_gn_bwd(const float* h, const float* a, const float* gamma, const float* stats, float* d, float* gpart, float* bpart,
                        int N, int HW, hipStream_t s) {
  hipLaunchKernelGGL(k_mini_gn_bwd, dim3(N, CQ), dim3(256), 0, s, h, a, gamma, stats, d, gpart, bpart, HW);
}
void launch_mini_conv0_wgrad(const float* x, const float* dh0, float* slab, int N, int Cin, int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(k_mini_conv0_wgrad, dim3(N, 3), dim3(256), 0, s, x, dh0, slab, Cin, H, W);
}
void launch_mini_conv0_dgrad(const float* dh0, const float* w0, float* dx, int N, int Cin, int H, int W, hipStream_t s) {
  const int R = N * H * W;
  hipLaunchKernelGGL(k_mini_conv0_dgrad, dim3((R + 255) / 256), dim3(256), 0, s, dh0, w0, dx, R, Cin, H, W);
}
void launch_mini_chansum(const float* g, float* db, int N, int Cn, int HW, hipStream_t s) {
  hipLaunchKernelGGL(k_mini_chansum, dim3(Cn), dim3(256), 0, s, g, db, N, Cn, HW);
}
void launch_mini_sums(const MiniSumArgs& a, hipStream_t s) {
  int most = 1;
  for (int i = 0; i < a.njobs; ++i) most = a.job[i].count > most ? a.job[i].count : most;
  hipLaunchKernelGGL(k_mini_sums, dim3((most + 255) / 256, a.njobs), dim3(256), 0, s, a);
}

}  // namespace node
