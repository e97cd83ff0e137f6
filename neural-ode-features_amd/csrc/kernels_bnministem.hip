// BatchNorm(24, batch statistics) + ReLU passes of the `minimal` stem with norm = 'batch' (bnministem.h has the argument structure):
// kernels_batchnorm.hip's two-stage scheme on NHWC tensors of channel pitch 24.
//
// Layout of every pass: a workgroup = one chunk of rows x all 24 channels; 192 threads = 32 rows x 6 channel quads per trip.  A
// chunk starts at a multiple of 32 rows, so the 16-byte word a thread reads in trip k is word (chunk start) * 6 + 192 k + t of the
// tensor: consecutive threads, consecutive words, and t % 6 -- the thread's channel quad -- is the same in every trip.  (256 threads
// do not divide by six quads; 192 do, and three waves a workgroup keep 128 workgroups' worth of waves in flight.)
//
// Statistics, two stages, no atomics: k_bnmini_stats writes per (chunk, channel) the chunk's mean and its CENTRED second moment
// (mean pass, then a centred pass over the same rows, which then come from cache); k_bnmini_apply combines a channel's partials by
// Chan's formula in one fixed order (eight interleaved chains, then those eight).  The backward's sums (sum dy, sum dy xhat) take
// the same two stages with fp64 partials: k_bnmini_bwd_stats -> k_bnmini_bwd_dx.  Every sum has one order: the same bits on every run.
//
// The ReLU mask of the backward is recomputed from h with the forward's own expressions (bnm_xhat, bnm_y), so both directions see
// the same sign bit for bit and the backward reads two tensors (h, d), not three.
//
// No loop or branch here depends on data: a NaN anywhere in the input reaches the statistics of its channel and from there every
// output of that channel.
#include "bnministem.h"

namespace node {

namespace {

constexpr int C = MINI_C;
constexpr int CQ = C / 4;                    // 16-byte channel quads of a pixel
constexpr int TRIP = BNMINI_TRIP;
constexpr int NT = BNMINI_THREADS;
constexpr int CHAINS = NT / C;               // interleaved chains of a combination: thread = (channel t % 24, chain t / 24)

__device__ __forceinline__ float bnm_xhat(float u, float mean, float rstd) { return (u - mean) * rstd; }
__device__ __forceinline__ float bnm_y(float xh, float g, float b) { return __builtin_fmaf(xh, g, b); }

struct Geo { size_t w0, w1; int nrows; };   // the chunk's 16-byte words [w0, w1) and its rows
__device__ __forceinline__ Geo bnm_geo(const BnMiniArgs& a) {
  const int r0 = blockIdx.x * a.chunk_rows, r1 = min(r0 + a.chunk_rows, a.rows);
  Geo g;
  g.w0 = (size_t)r0 * CQ;
  g.w1 = (size_t)r1 * CQ;
  g.nrows = r1 - r0;
  return g;
}

// the thread's quad sums -> the column sums over the workgroup's 32 row slots, in slot order: thread t < 24 returns channel t's,
// the others 0.  red: [32][24].  Ends behind a barrier (red is free again).
__device__ __forceinline__ float colsum24(float4 s, float4* red, int t) {
  red[t] = s;
  __syncthreads();
  float r = 0.f;
  if (t < C) {
    const float* rf = reinterpret_cast<const float*>(red);
#pragma unroll 8
    for (int j = 0; j < TRIP; ++j) r += rf[j * C + t];
  }
  __syncthreads();
  return r;
}
// the same sums taken in fp64 (the backward's sum dy and sum dy xhat)
__device__ __forceinline__ double colsum24d(float4 s, float4* red, int t) {
  red[t] = s;
  __syncthreads();
  double r = 0.0;
  if (t < C) {
    const float* rf = reinterpret_cast<const float*>(red);
#pragma unroll 8
    for (int j = 0; j < TRIP; ++j) r += (double)rf[j * C + t];
  }
  __syncthreads();
  return r;
}

// ============================================================================
// forward, stage 1: per (chunk, channel) the chunk's mean and centred second moment
// ============================================================================
__global__ __launch_bounds__(NT) void k_bnmini_stats(const BnMiniArgs a) {
  __shared__ float4 red[NT];
  __shared__ __align__(16) float cm[C];
  const int t = threadIdx.x, q = t % CQ;
  const Geo g = bnm_geo(a);
  const float4* hp = reinterpret_cast<const float4*>(a.h);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (size_t i = g.w0 + t; i < g.w1; i += NT) {
    const float4 v = hp[i];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  const float sum = colsum24(s, red, t);
  const float mean = sum / (float)g.nrows;
  if (t < C) cm[t] = mean;
  __syncthreads();
  const float4 m = reinterpret_cast<const float4*>(cm)[q];
  s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (size_t i = g.w0 + t; i < g.w1; i += NT) {
    const float4 v = hp[i];
    const float dx = v.x - m.x, dy = v.y - m.y, dz = v.z - m.z, dw = v.w - m.w;
    s.x = __builtin_fmaf(dx, dx, s.x); s.y = __builtin_fmaf(dy, dy, s.y);
    s.z = __builtin_fmaf(dz, dz, s.z); s.w = __builtin_fmaf(dw, dw, s.w);
  }
  const float m2 = colsum24(s, red, t);
  if (t < C) {
    a.part[((size_t)blockIdx.x * 2 + 0) * C + t] = mean;
    a.part[((size_t)blockIdx.x * 2 + 1) * C + t] = m2;
  }
}

// Chan's update of (n, mean, M2) by a chunk of nk > 0 rows
__device__ __forceinline__ void chan_merge(float& n, float& m, float& M2, float nk, float mk, float Mk) {
  const float tot = n + nk, f = nk / tot, d = mk - m;
  m = __builtin_fmaf(d, f, m);
  M2 = M2 + Mk + d * d * n * f;
  n = tot;
}

// ============================================================================
// forward, stage 2: the batch statistics from the partials, a = relu(xhat gamma + beta)
// ============================================================================
__global__ __launch_bounds__(NT) void k_bnmini_apply(const BnMiniArgs a) {
  __shared__ float sm[CHAINS * 3 * C];
  __shared__ __align__(16) float smean[C], srstd[C];
  const int t = threadIdx.x, q = t % CQ;
  {   // thread (c = t % 24, chain = t / 24) merges chunks chain, chain + 8, ..; thread c then the eight chains in order
    const int c = t % C, ch = t / C;
    float n = 0.f, m = 0.f, M2 = 0.f;
    for (int k = ch; k < a.nchunk; k += CHAINS) {
      const float nk = (float)min(a.chunk_rows, a.rows - k * a.chunk_rows);
      chan_merge(n, m, M2, nk, a.part[((size_t)k * 2 + 0) * C + c], a.part[((size_t)k * 2 + 1) * C + c]);
    }
    sm[(ch * 3 + 0) * C + c] = n;
    sm[(ch * 3 + 1) * C + c] = m;
    sm[(ch * 3 + 2) * C + c] = M2;
    __syncthreads();
    if (t < C) {
      n = sm[t]; m = sm[C + t]; M2 = sm[2 * C + t];
#pragma unroll
      for (int j = 1; j < CHAINS; ++j) {
        const float nj = sm[(j * 3 + 0) * C + t];
        if (nj > 0.f) chan_merge(n, m, M2, nj, sm[(j * 3 + 1) * C + t], sm[(j * 3 + 2) * C + t]);   // (fewer than eight chunks: a shape's property, not the data's)
      }
      const float rs = 1.f / sqrtf(M2 / (float)a.rows + a.eps);
      smean[t] = m;
      srstd[t] = rs;
      if (blockIdx.x == 0) {
        a.stats[t] = m;
        a.stats[C + t] = rs;
      }
    }
    __syncthreads();
  }
  const float4 mu = reinterpret_cast<const float4*>(smean)[q], rs = reinterpret_cast<const float4*>(srstd)[q];
  const float4 ga = reinterpret_cast<const float4*>(a.gamma)[q], be = reinterpret_cast<const float4*>(a.beta)[q];
  const Geo g = bnm_geo(a);
  const float4* hp = reinterpret_cast<const float4*>(a.h);
  float4* ap = reinterpret_cast<float4*>(a.a);
  for (size_t i = g.w0 + t; i < g.w1; i += NT) {
    const float4 v = hp[i];
    float4 o;
    o.x = bnm_y(bnm_xhat(v.x, mu.x, rs.x), ga.x, be.x);
    o.y = bnm_y(bnm_xhat(v.y, mu.y, rs.y), ga.y, be.y);
    o.z = bnm_y(bnm_xhat(v.z, mu.z, rs.z), ga.z, be.z);
    o.w = bnm_y(bnm_xhat(v.w, mu.w, rs.w), ga.w, be.w);
    o.x = o.x < 0.f ? 0.f : o.x; o.y = o.y < 0.f ? 0.f : o.y;      // (keeps NaN, as torch's ReLU does)
    o.z = o.z < 0.f ? 0.f : o.z; o.w = o.w < 0.f ? 0.f : o.w;
    ap[i] = o;
  }
}

// dy of one element: da behind the ReLU mask recomputed from xhat
__device__ __forceinline__ float bnm_dy(float xh, float g, float b, float da) { return bnm_y(xh, g, b) <= 0.f ? 0.f : da; }

// ============================================================================
// backward, stage 1: per (chunk, channel) sum dy and sum dy xhat, fp64 from the thread's own few rows on
// ============================================================================
__global__ __launch_bounds__(NT) void k_bnmini_bwd_stats(const BnMiniArgs a) {
  __shared__ float4 red[NT];
  const int t = threadIdx.x, q = t % CQ;
  const Geo g = bnm_geo(a);
  const float4 mu = reinterpret_cast<const float4*>(a.stats)[q], rs = reinterpret_cast<const float4*>(a.stats + C)[q];
  const float4 ga = reinterpret_cast<const float4*>(a.gamma)[q], be = reinterpret_cast<const float4*>(a.beta)[q];
  const float4* hp = reinterpret_cast<const float4*>(a.h);
  const float4* dp = reinterpret_cast<const float4*>(a.d);
  float4 sA = make_float4(0.f, 0.f, 0.f, 0.f), sB = sA;
  for (size_t i = g.w0 + t; i < g.w1; i += NT) {
    const float4 v = hp[i], da = dp[i];
    const float xx = bnm_xhat(v.x, mu.x, rs.x), xy = bnm_xhat(v.y, mu.y, rs.y), xz = bnm_xhat(v.z, mu.z, rs.z),
                xw = bnm_xhat(v.w, mu.w, rs.w);
    const float dx = bnm_dy(xx, ga.x, be.x, da.x), dy = bnm_dy(xy, ga.y, be.y, da.y), dz = bnm_dy(xz, ga.z, be.z, da.z),
                dw = bnm_dy(xw, ga.w, be.w, da.w);
    sA.x += dx; sA.y += dy; sA.z += dz; sA.w += dw;
    sB.x = __builtin_fmaf(dx, xx, sB.x); sB.y = __builtin_fmaf(dy, xy, sB.y);
    sB.z = __builtin_fmaf(dz, xz, sB.z); sB.w = __builtin_fmaf(dw, xw, sB.w);
  }
  const double A = colsum24d(sA, red, t);
  const double B = colsum24d(sB, red, t);
  if (t < C) {
    a.gpart[((size_t)blockIdx.x * 2 + 0) * C + t] = A;
    a.gpart[((size_t)blockIdx.x * 2 + 1) * C + t] = B;
  }
}

// ============================================================================
// backward, stage 2, in place on d: dh = rstd gamma (dy - mean(dy) - xhat mean(dy xhat)); dgamma = sum dy xhat, dbeta = sum dy
// (chunk 0 writes them); the chunk's column sums of dh -> bpart
// ============================================================================
__global__ __launch_bounds__(NT) void k_bnmini_bwd_dx(const BnMiniArgs a) {
  __shared__ double dsm[CHAINS * 2 * C];
  __shared__ float4 red[NT];
  __shared__ __align__(16) float sAs[C], sBs[C];
  const int t = threadIdx.x, q = t % CQ;
  {
    const int c = t % C, ch = t / C;
    double A = 0.0, B = 0.0;
    for (int k = ch; k < a.nchunk; k += CHAINS) {
      A += a.gpart[((size_t)k * 2 + 0) * C + c];
      B += a.gpart[((size_t)k * 2 + 1) * C + c];
    }
    dsm[(ch * 2 + 0) * C + c] = A;
    dsm[(ch * 2 + 1) * C + c] = B;
    __syncthreads();
    if (t < C) {
      A = ((dsm[t] + dsm[2 * C + t]) + (dsm[4 * C + t] + dsm[6 * C + t])) +
          ((dsm[8 * C + t] + dsm[10 * C + t]) + (dsm[12 * C + t] + dsm[14 * C + t]));
      B = ((dsm[C + t] + dsm[3 * C + t]) + (dsm[5 * C + t] + dsm[7 * C + t])) +
          ((dsm[9 * C + t] + dsm[11 * C + t]) + (dsm[13 * C + t] + dsm[15 * C + t]));
      sAs[t] = (float)(A / (double)a.rows);             // mean(dy), mean(dy xhat)
      sBs[t] = (float)(B / (double)a.rows);
      if (blockIdx.x == 0) {
        if (a.dgamma) a.dgamma[t] = (float)B;
        if (a.dbeta) a.dbeta[t] = (float)A;
      }
    }
    __syncthreads();
  }
  const Geo g = bnm_geo(a);
  const float4 mu = reinterpret_cast<const float4*>(a.stats)[q], rs = reinterpret_cast<const float4*>(a.stats + C)[q];
  const float4 ga = reinterpret_cast<const float4*>(a.gamma)[q], be = reinterpret_cast<const float4*>(a.beta)[q];
  const float4 mA = reinterpret_cast<const float4*>(sAs)[q], mB = reinterpret_cast<const float4*>(sBs)[q];
  const float4 kk = make_float4(rs.x * ga.x, rs.y * ga.y, rs.z * ga.z, rs.w * ga.w);
  const float4* hp = reinterpret_cast<const float4*>(a.h);
  float4* dp = reinterpret_cast<float4*>(a.d);
  float4 sb = make_float4(0.f, 0.f, 0.f, 0.f);
  for (size_t i = g.w0 + t; i < g.w1; i += NT) {
    const float4 v = hp[i], da = dp[i];
    const float xx = bnm_xhat(v.x, mu.x, rs.x), xy = bnm_xhat(v.y, mu.y, rs.y), xz = bnm_xhat(v.z, mu.z, rs.z),
                xw = bnm_xhat(v.w, mu.w, rs.w);
    float4 o;
    o.x = kk.x * __builtin_fmaf(-xx, mB.x, bnm_dy(xx, ga.x, be.x, da.x) - mA.x);
    o.y = kk.y * __builtin_fmaf(-xy, mB.y, bnm_dy(xy, ga.y, be.y, da.y) - mA.y);
    o.z = kk.z * __builtin_fmaf(-xz, mB.z, bnm_dy(xz, ga.z, be.z, da.z) - mA.z);
    o.w = kk.w * __builtin_fmaf(-xw, mB.w, bnm_dy(xw, ga.w, be.w, da.w) - mA.w);
    dp[i] = o;
    sb.x += o.x; sb.y += o.y; sb.z += o.z; sb.w += o.w;
  }
  if (a.bpart == nullptr) return;      // (a launch argument: the whole grid leaves here or nobody does)
  const float SB = colsum24(sb, red, t);
  if (t < C) a.bpart[(size_t)blockIdx.x * C + t] = SB;
}

}  // namespace

// NODE_TUNE_BNMINI_MAXCHUNK (measurements only; read again by every plan, so once per call; part of the workspace layout): another
// cap on the chunks, 1 .. 1024.  Unset or 0: BNMINI_MAX_CHUNKS.  No kernel depends on the cap: every combination loops over nchunk.
int bnmini_chunk_rows(int rows) {
  int cap = env_int("NODE_TUNE_BNMINI_MAXCHUNK", 0);
  if (cap <= 0) cap = BNMINI_MAX_CHUNKS;
  if (cap > 1024) cap = 1024;
  int cr = (rows + cap - 1) / cap;
  cr = (cr + TRIP - 1) / TRIP * TRIP;
  return cr < TRIP ? TRIP : cr;
}

void launch_bnmini_stats(const BnMiniArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_bnmini_stats, dim3(a.nchunk), dim3(NT), 0, s, a); }
void launch_bnmini_apply(const BnMiniArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_bnmini_apply, dim3(a.nchunk), dim3(NT), 0, s, a); }
void launch_bnmini_bwd_stats(const BnMiniArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_bnmini_bwd_stats, dim3(a.nchunk), dim3(NT), 0, s, a);
}
void launch_bnmini_bwd_dx(const BnMiniArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_bnmini_bwd_dx, dim3(a.nchunk), dim3(NT), 0, s, a); }

}  // namespace node
