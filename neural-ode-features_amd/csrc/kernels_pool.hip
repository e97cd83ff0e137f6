// The hand-off between the two solves of the `ode` stem -- `ODEDownsample.maxpool`, nn.MaxPool2d(4, 2, 1) of model.py:181-196 --
// and the per-slice plane means of the stem's trajectory in feature extraction (model.py:36, `fi.mean(-1).mean(-1)`), NCHW fp32
// in and out:
//
//   pooled[q][oh][ow]  = max_{kh,kw} x[T-1][q][2 oh - 1 + kh][2 ow - 1 + kw]        (q = (n, c); outside the image: -inf)
//   argmax[q][oh][ow]  = the winning tap kh 4 + kw.  ATen's scan: row-major over the window, `val > max || isnan(val)` -- ties go
//                        to the first tap, a NaN wins and the last NaN of a window is the one named; a window of -inf alone
//                        names its first tap inside the image.
//   means[t][q]        = sum_{h,w} x[t][q][h][w] / (H W)
//   d_x[q][h][w]       = sum of grad_y[q][oh][ow] over the (at most 2 x 2) windows whose argmax names (h, w), in ascending
//                        (oh, ow) order starting from 0 -- the order of ATen's CPU backward, so the bits are its bits.
//
// Both kernels are streams: every byte is wanted once from HBM and nothing is computed that a load does not wait for.  A WAVE
// owns a plane, lanes run over the plane's items, waves stride over the planes: all index arithmetic is 32-bit and inside one
// plane, the sums have one fixed order (lane-strided partial sums, then a butterfly over the 64 lanes), no LDS, no atomics.
//
//   k_pool_fwd<VEC>   W % 4 == 0 and 16-byte planes: the mean reads the plane as float4 (1 KiB per wave instruction); a lane
//                     owns the output pair (oh, 2 j), (oh, 2 j + 1), whose windows are the columns 4 j - 1 .. 4 j + 4 of four
//                     rows: one float4 and two scalars per row, the results one float2 and one uchar2 store.  The pool's reads
//                     follow the mean's reads of the same KiB and hit the cache.  Otherwise (scalar): a lane per element of the
//                     sum and per output of the pool, 16 bounds-checked loads.
//   k_pool_bwd<VEC>   a gather: a lane owns four consecutive pixels of a row (one float4 store); they lie in the windows
//                     ow = 2 j - 1 .. 2 j + 2 of two output rows: 8 argmax bytes and 8 gradients.  Scalar: a lane per pixel, its
//                     2 x 2 windows.  Every element of d_x is stored exactly once; nothing is zero-filled.
#include "node_internal.h"

namespace node {

namespace {

constexpr int POOL_WAVES = POOL_THREADS / 64;
constexpr int POOL_MAX_BLOCKS = 256 * 8;      // 8 workgroups of 4 waves fill a CU's 32 wave slots; the rest is the grid stride

#define POOL_UPD(m, i, val, tap)        \
  {                                     \
    const float v_ = (val);             \
    if (v_ > m || v_ != v_) {           \
      m = v_;                           \
      i = (tap);                        \
    }                                   \
  }

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  return s;
}

template <bool VEC>
__global__ __launch_bounds__(POOL_THREADS) void k_pool_fwd(const float* __restrict__ x, float* __restrict__ pooled,
                                                           uint8_t* __restrict__ argmax, float* __restrict__ means, PoolArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * POOL_WAVES + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * POOL_WAVES;
  const int hw = a.h * a.w, ohw = a.oh * a.ow;
  const int64_t last0 = (int64_t)(a.t - 1) * a.planes;        // the first plane of the last slice
  const int64_t jobs = means ? (int64_t)a.t * a.planes : a.planes;
  const float NEG = -__builtin_inff();
  for (int64_t job = wave; job < jobs; job += nwaves) {
    const int64_t plane = means ? job : last0 + job;          // over [T, N, C]
    const float* __restrict__ xp = x + plane * hw;
    if (means) {
      float s = 0.f;
      if (VEC) {
        const float4* __restrict__ x4 = reinterpret_cast<const float4*>(xp);
        for (int i = lane; i < (hw >> 2); i += 64) {
          const float4 v = x4[i];
          s += v.x; s += v.y; s += v.z; s += v.w;
        }
      } else {
        for (int i = lane; i < hw; i += 64) s += xp[i];
      }
      s = wave_sum(s);
      if (lane == 0) means[plane] = s / (float)hw;
    }
    if (plane < last0) continue;
    const int64_t q = plane - last0;
    float* __restrict__ yp = pooled + q * ohw;
    uint8_t* __restrict__ ap = argmax ? argmax + q * ohw : nullptr;
    if (VEC) {
      const int owp = a.ow >> 1;                               // W % 4 == 0: OW = W / 2 is even
      for (int it = lane; it < a.oh * owp; it += 64) {
        const int oh = it / owp, j = it - oh * owp;
        const int first = oh == 0 ? 4 : 0;                     // the first row inside the image
        float m0 = NEG, m1 = NEG;
        int i0 = first + (j == 0 ? 1 : 0), i1 = first;
#pragma unroll
        for (int kh = 0; kh < 4; ++kh) {
          const int ih = 2 * oh - 1 + kh;
          if (ih < 0 || ih >= a.h) continue;
          const float* __restrict__ r = xp + ih * a.w + 4 * j;
          const float4 v = *reinterpret_cast<const float4*>(r);
          const float left = j > 0 ? r[-1] : NEG, right = 4 * j + 4 < a.w ? r[4] : NEG;      // -inf never wins: a skipped tap
          POOL_UPD(m0, i0, left, kh * 4 + 0) POOL_UPD(m0, i0, v.x, kh * 4 + 1) POOL_UPD(m0, i0, v.y, kh * 4 + 2) POOL_UPD(m0, i0, v.z, kh * 4 + 3)
          POOL_UPD(m1, i1, v.y, kh * 4 + 0) POOL_UPD(m1, i1, v.z, kh * 4 + 1) POOL_UPD(m1, i1, v.w, kh * 4 + 2) POOL_UPD(m1, i1, right, kh * 4 + 3)
        }
        const int o = oh * a.ow + 2 * j;
        *reinterpret_cast<float2*>(yp + o) = make_float2(m0, m1);
        if (ap) *reinterpret_cast<uchar2*>(ap + o) = make_uchar2((unsigned char)i0, (unsigned char)i1);
      }
    } else {
      for (int o = lane; o < ohw; o += 64) {
        const int oh = o / a.ow, ow = o - oh * a.ow;
        float m = NEG;
        int im = (oh == 0 ? 4 : 0) + (ow == 0 ? 1 : 0);
#pragma unroll
        for (int kh = 0; kh < 4; ++kh) {
          const int ih = 2 * oh - 1 + kh;
          if (ih < 0 || ih >= a.h) continue;
#pragma unroll
          for (int kw = 0; kw < 4; ++kw) {
            const int iw = 2 * ow - 1 + kw;
            if (iw < 0 || iw >= a.w) continue;
            POOL_UPD(m, im, xp[ih * a.w + iw], kh * 4 + kw)
          }
        }
        yp[o] = m;
        if (ap) ap[o] = (uint8_t)im;
      }
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(POOL_THREADS) void k_pool_bwd(const float* __restrict__ gy, const uint8_t* __restrict__ argmax,
                                                           float* __restrict__ dx, PoolArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * POOL_WAVES + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * POOL_WAVES;
  const int hw = a.h * a.w, ohw = a.oh * a.ow;
  for (int64_t q = wave; q < a.planes; q += nwaves) {
    const float* __restrict__ gp = gy + q * ohw;
    const uint8_t* __restrict__ ap = argmax + q * ohw;
    float* __restrict__ dp = dx + q * hw;
    if (VEC) {
      const int wq = a.w >> 2;
      for (int it = lane; it < a.h * wq; it += 64) {
        const int h = it / wq, j = it - h * wq;
        const int oh_hi = (h + 1) >> 1;                          // row h lies in the windows oh_hi - 1 and oh_hi
        float g[2][4];
        int t[2][4];                                             // the tap an output names, minus its tap ROW's 4 kh: 255 where there is no output
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int oh = oh_hi - 1 + r;
          const int kh = h + 1 - 2 * oh;                         // 3 or 2 for the upper window, 1 or 0 for the lower
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int ow = 2 * j - 1 + c;
            const bool ok = oh >= 0 && oh < a.oh && ow >= 0 && ow < a.ow;
            g[r][c] = ok ? gp[oh * a.ow + ow] : 0.f;
            t[r][c] = ok ? (int)ap[oh * a.ow + ow] - 4 * kh : 255;
          }
        }
        // pixel p = w - 4 j lies in the windows c = lo, lo + 1 (ow = 2 j - 1 + c) at the taps kw = p + 3 - 2 c
        float4 o;
        float* op = reinterpret_cast<float*>(&o);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int lo = (p + 1) >> 1;
          float s = 0.f;
#pragma unroll
          for (int r = 0; r < 2; ++r) {
#pragma unroll
            for (int c = lo; c < lo + 2; ++c)
              if (t[r][c] == p + 3 - 2 * c) s += g[r][c];
          }
          op[p] = s;
        }
        *reinterpret_cast<float4*>(dp + h * a.w + 4 * j) = o;
      }
    } else {
      for (int i = lane; i < hw; i += 64) {
        const int h = i / a.w, w = i - h * a.w;
        const int oh_hi = (h + 1) >> 1, ow_hi = (w + 1) >> 1;
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int oh = oh_hi - 1 + r;
          if (oh < 0 || oh >= a.oh) continue;
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int ow = ow_hi - 1 + c;
            if (ow < 0 || ow >= a.ow) continue;
            const int tap = (h + 1 - 2 * oh) * 4 + (w + 1 - 2 * ow);
            if ((int)ap[oh * a.ow + ow] == tap) s += gp[oh * a.ow + ow];
          }
        }
        dp[i] = s;
      }
    }
  }
}

unsigned pool_grid(int64_t jobs) {
  const int64_t blocks = (jobs + POOL_WAVES - 1) / POOL_WAVES;
  return (unsigned)(blocks < POOL_MAX_BLOCKS ? blocks : POOL_MAX_BLOCKS);
}

}  // namespace

void launch_pool_fwd(const PoolArgs& a, bool vec, const float* x, float* pooled, uint8_t* argmax, float* means, hipStream_t s) {
  const dim3 grid(pool_grid(means ? (int64_t)a.t * a.planes : a.planes));
  if (vec) hipLaunchKernelGGL(k_pool_fwd<true>, grid, dim3(POOL_THREADS), 0, s, x, pooled, argmax, means, a);
  else hipLaunchKernelGGL(k_pool_fwd<false>, grid, dim3(POOL_THREADS), 0, s, x, pooled, argmax, means, a);
}

void launch_pool_bwd(const PoolArgs& a, bool vec, const float* gy, const uint8_t* argmax, float* dx, hipStream_t s) {
  const dim3 grid(pool_grid(a.planes));
  if (vec) hipLaunchKernelGGL(k_pool_bwd<true>, grid, dim3(POOL_THREADS), 0, s, gy, argmax, dx, a);
  else hipLaunchKernelGGL(k_pool_bwd<false>, grid, dim3(POOL_THREADS), 0, s, gy, argmax, dx, a);
}

}  // namespace node
