// The 4x4 stride-2 padding-1 convolution that turns an image into the ODE block's state -- the reference's one-shot stem
// (model.py:119-126) and the conv1 of its `ode` / `ode2` stems (model.py:185, 203) -- forward, weight / bias gradient and
// input gradient, NCHW fp32 in and out, fp32 arithmetic on the vector ALU:
//
//   y[n][o][oh][ow]     = b[o] + sum_{c,kh,kw} w[o][c][kh][kw] x[n][c][2 oh - 1 + kh][2 ow - 1 + kw]          (0 outside the image)
//   dw[o][c][kh][kw]    = sum_{n,oh,ow} dy[n][o][oh][ow] x[n][c][2 oh - 1 + kh][2 ow - 1 + kw],   db[o] = sum dy[n][o][oh][ow]
//   dx[n][c][ih][iw]    = sum_{o} sum_{kh = ih + 1 (mod 2), kw = iw + 1 (mod 2)} dy[n][o][(ih + 1 - kh) / 2][(iw + 1 - kw) / 2] w[o][c][kh][kw]
//
// K = 16 in_ch <= 64, so the layer is all bytes: y (or dy) is 16 filters/in_ch times larger than everything else together.
// Every kernel therefore puts consecutive output pixels on consecutive lanes (y and dy move in 256-byte rows per wave) and keeps
// what is small -- the filters -- on the scalar unit or in LDS.
//
//   k_imgconv_fwd    a thread owns ONE output pixel and IMG_FWD_FILTERS filters: its 16 in_ch patch values sit in registers, the
//                    filter taps are wave-uniform (scalar loads, SGPR operands of the FMAs); one coalesced store per filter.
//   k_imgconv_wgrad  a workgroup owns 64 filters and a slab of IMG_SLAB output pixels (flattened over n, oh, ow); it stages dy
//                    [64][64 pixels] and the im2col patch [K][64 pixels] in LDS, 64 pixels at a time; thread (og, tap) keeps
//                    dw of 4 filters x in_ch channels at its tap and sums over the slab's pixels in order.  db comes from the
//                    same staged dy.  The slab's partial goes to ws[slab][filters][K + 1].
//   k_imgconv_wsum   sums the slab partials in slab order: no atomics anywhere, dw and db are bit-reproducible.
//   k_imgconv_dgrad  a lane owns a 2x2 block of input pixels in every channel (all 16 taps of a filter, uniform over the
//                    wave: scalar loads again); the four waves of a workgroup take a quarter of the filters each and are
//                    summed in wave order through LDS.
#include "node_internal.h"

namespace node {

namespace {

constexpr int IMG_THREADS = 256;
constexpr int IMG_PT = 64;             // pixels per LDS stage of the weight gradient
constexpr int IMG_LD = IMG_PT + 4;     // row pitch of the staged tiles: 16-byte rows, rows 4 banks apart

template <int CIN>
__global__ __launch_bounds__(IMG_THREADS) void k_imgconv_fwd(const float* __restrict__ x, const float* __restrict__ wt,
                                                             const float* __restrict__ bias, float* __restrict__ y, ImgConvArgs a) {
  constexpr int K = 16 * CIN;
  const int P = blockIdx.x * IMG_THREADS + threadIdx.x;
  if (P >= a.np) return;
  const int ohw = a.oh * a.ow;
  const int n = P / ohw, pix = P - n * ohw;
  const int oy = pix / a.ow, ox = pix - oy * a.ow;
  float p[K];
#pragma unroll
  for (int c = 0; c < CIN; ++c)
#pragma unroll
    for (int kh = 0; kh < 4; ++kh) {
      const int ih = 2 * oy - 1 + kh;
#pragma unroll
      for (int kw = 0; kw < 4; ++kw) {
        const int iw = 2 * ox - 1 + kw;
        const bool in = ih >= 0 && ih < a.h && iw >= 0 && iw < a.w;
        p[c * 16 + kh * 4 + kw] = in ? x[((size_t)(n * CIN + c) * a.h + ih) * a.w + iw] : 0.f;
      }
    }
  const int f0 = blockIdx.y * IMG_FWD_FILTERS;
  float* dst = y + ((size_t)n * a.filters + f0) * ohw + pix;
  for (int f = 0; f < IMG_FWD_FILTERS; f += 4) {
    const float* wf = wt + (size_t)(f0 + f) * K;       // wave-uniform: scalar loads
    float acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = bias ? bias[f0 + f + j] : 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(p[k], wf[j * K + k], acc[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[(size_t)(f + j) * ohw] = acc[j];
  }
}

template <int CIN>
__global__ __launch_bounds__(IMG_THREADS) void k_imgconv_wgrad(const float* __restrict__ x, const float* __restrict__ dy,
                                                               float* __restrict__ ws, ImgConvArgs a) {
  constexpr int K = 16 * CIN;
  __shared__ __attribute__((aligned(16))) float dyL[64 * IMG_LD];
  __shared__ __attribute__((aligned(16))) float pL[K * IMG_LD];
  const int tid = threadIdx.x;
  const int tap = tid & 15, og = tid >> 4;          // compute role: tap kh * 4 + kw, filters og * 4 .. og * 4 + 3 of the chunk
  const int sp = tid & 63, sr = tid >> 6;           // staging role: pixel of the stage, first row
  const int o0 = blockIdx.y * 64;
  const int ohw = a.oh * a.ow;
  const int slab0 = blockIdx.x * IMG_SLAB;

  float acc[4][CIN], dbs = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int c = 0; c < CIN; ++c) acc[j][c] = 0.f;

  for (int st = 0; st < IMG_SLAB; st += IMG_PT) {
    const int P = slab0 + st + sp;
    const bool live = P < a.np;
    const int n = live ? P / ohw : 0;
    const int pix = live ? P - n * ohw : 0;
    const int oy = pix / a.ow, ox = pix - oy * a.ow;
    __syncthreads();          // the previous stage's readers are done
    const float* src = dy + ((size_t)n * a.filters + o0) * ohw + pix;
#pragma unroll 4
    for (int r = sr; r < 64; r += 4) dyL[r * IMG_LD + sp] = live ? src[(size_t)r * ohw] : 0.f;
#pragma unroll 4
    for (int k = sr; k < K; k += 4) {
      const int c = k >> 4, ih = 2 * oy - 1 + ((k >> 2) & 3), iw = 2 * ox - 1 + (k & 3);
      const bool in = live && ih >= 0 && ih < a.h && iw >= 0 && iw < a.w;
      pL[k * IMG_LD + sp] = in ? x[((size_t)(n * CIN + c) * a.h + ih) * a.w + iw] : 0.f;
    }
    __syncthreads();
#pragma unroll 2
    for (int q = 0; q < IMG_PT; q += 4) {
      float4 d[4], pv[CIN];
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] = *(const float4*)&dyL[(og * 4 + j) * IMG_LD + q];
#pragma unroll
      for (int c = 0; c < CIN; ++c) pv[c] = *(const float4*)&pL[(c * 16 + tap) * IMG_LD + q];
      if (tap < 4) {          // db: taps 0..3 sum a filter each; the other twelve lanes of the sixteen read nothing
        const float4 e = *(const float4*)&dyL[(og * 4 + tap) * IMG_LD + q];
        dbs += e.x;
        dbs += e.y;
        dbs += e.z;
        dbs += e.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < CIN; ++c) {
          acc[j][c] = fmaf(d[j].x, pv[c].x, acc[j][c]);
          acc[j][c] = fmaf(d[j].y, pv[c].y, acc[j][c]);
          acc[j][c] = fmaf(d[j].z, pv[c].z, acc[j][c]);
          acc[j][c] = fmaf(d[j].w, pv[c].w, acc[j][c]);
        }
    }
  }
  float* out = ws + ((size_t)blockIdx.x * a.filters + o0 + og * 4) * (K + 1);
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int c = 0; c < CIN; ++c) out[j * (K + 1) + c * 16 + tap] = acc[j][c];
  if (tap < 4) out[tap * (K + 1) + K] = dbs;
}

// dw[o][k] / db[o] = sum over the slabs, in slab order
__global__ __launch_bounds__(IMG_THREADS) void k_imgconv_wsum(const float* __restrict__ ws, float* __restrict__ dw,
                                                              float* __restrict__ db, int filters, int k, int nslab) {
  const int i = blockIdx.x * IMG_THREADS + threadIdx.x;
  const int total = filters * (k + 1);
  if (i >= total) return;
  // the loads of a batch are in flight together (one latency per batch, not per slab); the adds keep the slab order
  constexpr int B = 32;
  float s = 0.f;
  int sl = 0;
  for (; sl + B <= nslab; sl += B) {
    float v[B];
#pragma unroll
    for (int j = 0; j < B; ++j) v[j] = ws[(size_t)(sl + j) * total + i];
#pragma unroll
    for (int j = 0; j < B; ++j) s += v[j];
  }
  for (; sl < nslab; ++sl) s += ws[(size_t)sl * total + i];
  const int o = i / (k + 1), kk = i - o * (k + 1);
  if (kk < k)
    dw[o * k + kk] = s;
  else if (db)
    db[o] = s;
}

template <int CIN>
__global__ __launch_bounds__(IMG_THREADS) void k_imgconv_dgrad(const float* __restrict__ wt, const float* __restrict__ dy,
                                                               float* __restrict__ dx, ImgConvArgs a) {
  constexpr int K = 16 * CIN;
  __shared__ float red[3][CIN * 4][64];
  const int lane = threadIdx.x & 63;
  const int quarter = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // the wave's index, known uniform: the taps take the scalar path
  const int P = blockIdx.x * 64 + lane;            // the 2x2 input block (n, by, bx): rows 2 by, 2 by + 1, columns 2 bx, 2 bx + 1
  const bool live = P < a.np;
  const int ohw = a.oh * a.ow;
  const int n = live ? P / ohw : 0;
  const int pix = live ? P - n * ohw : 0;
  const int by = pix / a.ow, bx = pix - by * a.ow;
  const int fq = a.filters >> 2;
  // input row 2 by     takes kh = 1 from output row by and kh = 3 from by - 1;
  // input row 2 by + 1 takes kh = 2 from output row by and kh = 0 from by + 1     (columns likewise)
  const bool up = live && by > 0, down = live && by + 1 < a.oh, left = bx > 0, right = bx + 1 < a.ow;
  float acc[CIN][2][2];
#pragma unroll
  for (int c = 0; c < CIN; ++c) acc[c][0][0] = acc[c][0][1] = acc[c][1][0] = acc[c][1][1] = 0.f;
  const float* src = dy + ((size_t)n * a.filters + quarter * fq) * ohw + pix;
  constexpr int U = 4;      // fq % 16 == 0; the dy loads of U filters are in flight together, the taps stay one filter at a time
  for (int o = 0; o < fq; o += U) {
    float d[U][3][3];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float* g = src + (size_t)(o + u) * ohw;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const bool rin = r == 0 ? up : r == 1 ? live : down;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const bool sin = s == 0 ? left : s == 1 ? true : right;
          d[u][r][s] = (rin && sin) ? g[(r - 1) * a.ow + (s - 1)] : 0.f;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float* wf = wt + (size_t)(quarter * fq + o + u) * K;       // wave-uniform: scalar loads
#pragma unroll
      for (int c = 0; c < CIN; ++c)
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
          for (int px = 0; px < 2; ++px) {
            // py = 0: (kh 1, row by = d[1]), (kh 3, row by - 1 = d[0]);   py = 1: (kh 2, d[1]), (kh 0, row by + 1 = d[2])
            const int kha = py ? 2 : 1, ra = 1, khb = py ? 0 : 3, rb = py ? 2 : 0;
            const int kwa = px ? 2 : 1, sa = 1, kwb = px ? 0 : 3, sb = px ? 2 : 0;
            float v = acc[c][py][px];
            v = fmaf(d[u][ra][sa], wf[c * 16 + kha * 4 + kwa], v);
            v = fmaf(d[u][ra][sb], wf[c * 16 + kha * 4 + kwb], v);
            v = fmaf(d[u][rb][sa], wf[c * 16 + khb * 4 + kwa], v);
            v = fmaf(d[u][rb][sb], wf[c * 16 + khb * 4 + kwb], v);
            acc[c][py][px] = v;
          }
    }
  }
  if (quarter > 0) {
#pragma unroll
    for (int c = 0; c < CIN; ++c)
#pragma unroll
      for (int t = 0; t < 4; ++t) red[quarter - 1][c * 4 + t][lane] = acc[c][t >> 1][t & 1];
  }
  __syncthreads();
  if (quarter == 0 && live) {
#pragma unroll
    for (int c = 0; c < CIN; ++c) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float v = acc[c][t >> 1][t & 1];
        v += red[0][c * 4 + t][lane];
        v += red[1][c * 4 + t][lane];
        v += red[2][c * 4 + t][lane];
        acc[c][t >> 1][t & 1] = v;
      }
      float* dst = dx + ((size_t)(n * CIN + c) * a.h + 2 * by) * a.w + 2 * bx;      // w is even: 8-byte aligned
      *(float2*)dst = make_float2(acc[c][0][0], acc[c][0][1]);
      *(float2*)(dst + a.w) = make_float2(acc[c][1][0], acc[c][1][1]);
    }
  }
}

}  // namespace

int imgconv_slabs(int64_t np) { return (int)((np + IMG_SLAB - 1) / IMG_SLAB); }

#define IMG_DISPATCH(CIN, CALL) \
  switch (CIN) {                \
    case 1: { constexpr int C_ = 1; CALL; } break; \
    case 2: { constexpr int C_ = 2; CALL; } break; \
    case 3: { constexpr int C_ = 3; CALL; } break; \
    default: { constexpr int C_ = 4; CALL; } break; \
  }

void launch_imgconv_fwd(const ImgConvArgs& a, int in_ch, const float* x, const float* w, const float* bias, float* y, hipStream_t s) {
  const dim3 grid((unsigned)((a.np + IMG_THREADS - 1) / IMG_THREADS), (unsigned)(a.filters / IMG_FWD_FILTERS));
  IMG_DISPATCH(in_ch, hipLaunchKernelGGL(k_imgconv_fwd<C_>, grid, dim3(IMG_THREADS), 0, s, x, w, bias, y, a));
}

void launch_imgconv_wgrad(const ImgConvArgs& a, int in_ch, const float* x, const float* dy, float* dw, float* db, float* ws,
                          hipStream_t s) {
  const int nslab = imgconv_slabs(a.np);
  const dim3 grid((unsigned)nslab, (unsigned)(a.filters / 64));
  IMG_DISPATCH(in_ch, hipLaunchKernelGGL(k_imgconv_wgrad<C_>, grid, dim3(IMG_THREADS), 0, s, x, dy, ws, a));
  const int k = 16 * in_ch, total = a.filters * (k + 1);
  hipLaunchKernelGGL(k_imgconv_wsum, dim3((unsigned)((total + IMG_THREADS - 1) / IMG_THREADS)), dim3(IMG_THREADS), 0, s, ws, dw, db,
                     a.filters, k, nslab);
}

void launch_imgconv_dgrad(const ImgConvArgs& a, int in_ch, const float* w, const float* dy, float* dx, hipStream_t s) {
  const dim3 grid((unsigned)((a.np + 63) / 64));
  IMG_DISPATCH(in_ch, hipLaunchKernelGGL(k_imgconv_dgrad<C_>, grid, dim3(IMG_THREADS), 0, s, w, dy, dx, a));
}

}  // namespace node
