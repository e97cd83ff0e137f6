// The classifier head of a `norm='batch'` net up to (not including) its Linear layer -- model.py:231-250 with model.py:274:
//     pooled[n][c] = scale[n][c] * mean_px relu(gamma_c xhat + beta_c),   xhat normalised by the statistics of channel c over all N H W
// values of the NCHW tensor the net's body leaves (batchnorm.h: SBnHeadArgs).  The GroupNorm head (kernels_head.hip) holds a sample's
// group in one workgroup; BatchNorm needs sums ACROSS the samples, so this is a family of its own: two launches each way.
//
// Layout of every pass: a workgroup = (channel c, chunk of S samples), four waves; a wave takes one (n, c) plane at a time, lane = pixel
// (stride 64).  A plane is H W contiguous floats -- 256 bytes, two whole cache lines, at 8 x 8: one load instruction of the wave --
// and workgroups of neighbouring channels read neighbouring planes.
//
// Statistics, two stages, no atomics, as in kernels_batchnorm.hip: k_bnhead_stats writes per (chunk, channel) the chunk's mean and its
// CENTRED second moment (mean pass, then a centred pass over the same planes, which then come from cache); the consumers combine a
// channel's partials by Chan's formula in one fixed tree over the lanes.  E[x^2] - E[x]^2 would lose the variance of x = 50 + randn to
// cancellation.  The backward's sums (sum dy, sum dy xhat) take the same two stages, fp64 from the lane's own few pixels on
// (k_bn_bwd_stats says why).  Every sum has one order -- lanes by xor butterflies, whose two operands commute, then the four waves,
// then the chunks -- so a run returns the same bits as the run before.
//
// No loop or branch here depends on data: a NaN reaches the statistics of its channel and from there every output of that channel.
#include "batchnorm.h"

namespace node {

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ double wave_sumd(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
// the four waves' sums in wave order; every thread returns the total.  sm: [4].  Ends behind a barrier (sm is free again).
__device__ __forceinline__ float block_sum(float v, float* sm, int wave, int lane) {
  v = wave_sum(v);
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  const float r = (sm[0] + sm[1]) + (sm[2] + sm[3]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ double block_sumd(double v, double* sm, int wave, int lane) {
  v = wave_sumd(v);
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  const double r = (sm[0] + sm[1]) + (sm[2] + sm[3]);
  __syncthreads();
  return r;
}

struct HGeo { int c, chunk, n0, n1, wave, lane; };
__device__ __forceinline__ HGeo head_geo(const SBnHeadArgs& a) {
  HGeo g;
  g.chunk = blockIdx.x / a.C;
  g.c = blockIdx.x - g.chunk * a.C;
  g.n0 = g.chunk * a.chunk_samples;
  g.n1 = min(g.n0 + a.chunk_samples, a.N);
  g.wave = threadIdx.x >> 6;
  g.lane = threadIdx.x & 63;
  return g;
}
__device__ __forceinline__ const float* plane_of(const SBnHeadArgs& a, int n, int c) { return a.z + ((size_t)n * a.C + c) * a.HW; }

// ============================================================================
// forward, stage 1: per (chunk, channel) the chunk's mean and centred second moment
// ============================================================================
__device__ __forceinline__ void bnhead_stats_body(const SBnHeadArgs& a) {
  __shared__ float sm[4];
  const HGeo g = head_geo(a);
  float s = 0.f;
  for (int n = g.n0 + g.wave; n < g.n1; n += 4) {
    const float* z = plane_of(a, n, g.c);
    for (int p = g.lane; p < a.HW; p += 64) s += z[p];
  }
  const float mean = block_sum(s, sm, g.wave, g.lane) / (float)((g.n1 - g.n0) * a.HW);
  s = 0.f;
  for (int n = g.n0 + g.wave; n < g.n1; n += 4) {
    const float* z = plane_of(a, n, g.c);
    for (int p = g.lane; p < a.HW; p += 64) {
      const float d = z[p] - mean;
      s = __builtin_fmaf(d, d, s);
    }
  }
  const float m2 = block_sum(s, sm, g.wave, g.lane);
  if (threadIdx.x == 0) {
    a.part[((size_t)g.chunk * 2 + 0) * a.C + g.c] = mean;
    a.part[((size_t)g.chunk * 2 + 1) * a.C + g.c] = m2;
  }
}
__global__ __launch_bounds__(256) void k_bnhead_stats(const SBnHeadArgs a) { bnhead_stats_body(a); }

// The batch statistics of channel c from its partials: lane k < nchunk holds chunk k, six xor steps merge neighbours by Chan's formula,
// always (lower lanes' set, higher lanes' set) in that order, so every lane of every wave of every workgroup ends with the same bits.
// A set of no rows (lanes past nchunk; nchunk is the shape's property, not the data's) merges as nothing.
__device__ __forceinline__ void head_combine(const SBnHeadArgs& a, int c, int lane, float& mean, float& rstd) {
  float n = 0.f, m = 0.f, M2 = 0.f;
  if (lane < a.nchunk) {
    n = (float)((min(a.chunk_samples, a.N - lane * a.chunk_samples)) * a.HW);
    m = a.part[((size_t)lane * 2 + 0) * a.C + c];
    M2 = a.part[((size_t)lane * 2 + 1) * a.C + c];
  }
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const float no = __shfl_xor(n, k), mo = __shfl_xor(m, k), Mo = __shfl_xor(M2, k);
    const bool hi = (lane & k) != 0;
    const float nl = hi ? no : n, ml = hi ? mo : m, Ml = hi ? Mo : M2;
    const float nh = hi ? n : no, mh = hi ? m : mo, Mh = hi ? M2 : Mo;
    const float tot = nl + nh;
    const float f = tot > 0.f ? nh / tot : 0.f, d = mh - ml;
    m = __builtin_fmaf(d, f, ml);
    M2 = Ml + Mh + d * d * nl * f;
    n = tot;
  }
  mean = m;
  rstd = 1.f / sqrtf(M2 / ((float)a.N * (float)a.HW) + a.eps);
}

// ============================================================================
// forward, stage 2: pooled = scale * mean_px relu(xhat gamma + beta)
// ============================================================================
__device__ __forceinline__ void bnhead_apply_body(const SBnHeadArgs& a) {
  const HGeo g = head_geo(a);
  float mean, rstd;
  head_combine(a, g.c, g.lane, mean, rstd);
  if (g.chunk == 0 && threadIdx.x == 0) {
    a.stats[g.c] = mean;
    a.stats[a.C + g.c] = rstd;
  }
  const float ga = a.gamma[g.c], be = a.beta[g.c];
  for (int n = g.n0 + g.wave; n < g.n1; n += 4) {
    const float* z = plane_of(a, n, g.c);
    float s = 0.f;
    for (int p = g.lane; p < a.HW; p += 64) {
      const float y = __builtin_fmaf((z[p] - mean) * rstd, ga, be);
      s += y < 0.f ? 0.f : y;
    }
    s = wave_sum(s);
    if (g.lane == 0) {
      const float v = s / (float)a.HW;
      const size_t o = (size_t)n * a.C + g.c;
      a.pooled[o] = a.scale != nullptr ? v * a.scale[o] : v;
    }
  }
}
__global__ __launch_bounds__(256) void k_bnhead_apply(const SBnHeadArgs a) { bnhead_apply_body(a); }

// The two forward passes with a slice coordinate (blockIdx.y): z [slices][N][C][HW], statistics, partials and pooled rows PER SLICE
// -- the reference sends a trajectory's time slices through the norm one by one.  A slice's workgroups run the bodies above on that
// slice's tensors: the chunking within a slice is what the plain launch picks for [N][C][HW], Chan's combine is per (slice, channel)
// in the same tree, so every slice has the bits of its own plain call.  Forward only: no dropout scale.
__device__ __forceinline__ SBnHeadArgs slice_of(SBnHeadArgs a) {
  const size_t s = blockIdx.y;
  a.z += s * (size_t)a.N * a.C * a.HW;
  a.part += s * (size_t)a.nchunk * 2 * a.C;
  a.stats += s * 2 * (size_t)a.C;
  a.pooled += s * (size_t)a.N * a.C;
  return a;
}
__global__ __launch_bounds__(256) void k_bnhead_stats_slices(const SBnHeadArgs a) { bnhead_stats_body(slice_of(a)); }
__global__ __launch_bounds__(256) void k_bnhead_apply_slices(const SBnHeadArgs a) { bnhead_apply_body(slice_of(a)); }

// dy of a plane's pixels: g_pooled scale / (H W) behind the ReLU mask, which is recomputed from xhat as the forward formed it
__device__ __forceinline__ float head_gp(const SBnHeadArgs& a, int n, int c) {
  const size_t o = (size_t)n * a.C + c;
  const float gp = a.scale != nullptr ? a.g_pooled[o] * a.scale[o] : a.g_pooled[o];
  return gp / (float)a.HW;
}

// ============================================================================
// backward, stage 1: per (chunk, channel) sum dy and sum dy xhat, fp64 from the lane's own pixels on
// ============================================================================
__global__ __launch_bounds__(256) void k_bnhead_bwd_stats(const SBnHeadArgs a) {
  __shared__ double sm[4];
  const HGeo g = head_geo(a);
  const float mean = a.stats[g.c], rstd = a.stats[a.C + g.c], ga = a.gamma[g.c], be = a.beta[g.c];
  float sA = 0.f, sB = 0.f;
  for (int n = g.n0 + g.wave; n < g.n1; n += 4) {
    const float* z = plane_of(a, n, g.c);
    const float gp = head_gp(a, n, g.c);
    for (int p = g.lane; p < a.HW; p += 64) {
      const float xh = (z[p] - mean) * rstd;
      const float d = __builtin_fmaf(xh, ga, be) <= 0.f ? 0.f : gp;
      sA += d;
      sB = __builtin_fmaf(d, xh, sB);
    }
  }
  const double A = block_sumd((double)sA, sm, g.wave, g.lane);
  const double B = block_sumd((double)sB, sm, g.wave, g.lane);
  if (threadIdx.x == 0) {
    a.gpart[((size_t)g.chunk * 2 + 0) * a.C + g.c] = A;
    a.gpart[((size_t)g.chunk * 2 + 1) * a.C + g.c] = B;
  }
}

// ============================================================================
// backward, stage 2: dz = rstd gamma (dy - mean(dy) - xhat mean(dy xhat)); dgamma = sum dy xhat, dbeta = sum dy (chunk 0 writes them)
// ============================================================================
__global__ __launch_bounds__(256) void k_bnhead_bwd_dx(const SBnHeadArgs a) {
  const HGeo g = head_geo(a);
  double A = 0.0, B = 0.0;
  if (g.lane < a.nchunk) {
    A = a.gpart[((size_t)g.lane * 2 + 0) * a.C + g.c];
    B = a.gpart[((size_t)g.lane * 2 + 1) * a.C + g.c];
  }
  A = wave_sumd(A);
  B = wave_sumd(B);
  const double rows = (double)a.N * (double)a.HW;
  const float mA = (float)(A / rows), mB = (float)(B / rows);
  if (g.chunk == 0 && threadIdx.x == 0) {
    a.dgamma[g.c] = (float)B;
    a.dbeta[g.c] = (float)A;
  }
  const float mean = a.stats[g.c], rstd = a.stats[a.C + g.c], ga = a.gamma[g.c], be = a.beta[g.c];
  for (int n = g.n0 + g.wave; n < g.n1; n += 4) {
    const float* z = plane_of(a, n, g.c);
    float* dz = a.dz + ((size_t)n * a.C + g.c) * a.HW;
    const float gp = head_gp(a, n, g.c);
    for (int p = g.lane; p < a.HW; p += 64) {
      const float xh = (z[p] - mean) * rstd;
      const float d = __builtin_fmaf(xh, ga, be) <= 0.f ? 0.f : gp;
      dz[p] = rstd * ga * __builtin_fmaf(-xh, mB, d - mA);
    }
  }
}

}  // namespace

// ============================================================================
// launchers
// ============================================================================
int bnhead_chunk_samples(int N, int C) {
  int maxchunk = 2048 / C;                 // about 2048 workgroups at most
  if (maxchunk > BNHEAD_MAX_CHUNKS) maxchunk = BNHEAD_MAX_CHUNKS;
  if (maxchunk > (N + 3) / 4) maxchunk = (N + 3) / 4;      // a plane per wave at least
  if (maxchunk < 1) maxchunk = 1;
  return (N + maxchunk - 1) / maxchunk;
}
static dim3 head_grid(const SBnHeadArgs& a) { return dim3((unsigned)(a.nchunk * a.C)); }

void launch_bnhead_stats(const SBnHeadArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_bnhead_stats, head_grid(a), dim3(256), 0, s, a); }
void launch_bnhead_apply(const SBnHeadArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_bnhead_apply, head_grid(a), dim3(256), 0, s, a); }
void launch_bnhead_stats_slices(const SBnHeadArgs& a, int slices, hipStream_t s) {
  hipLaunchKernelGGL(k_bnhead_stats_slices, dim3((unsigned)(a.nchunk * a.C), (unsigned)slices), dim3(256), 0, s, a);
}
void launch_bnhead_apply_slices(const SBnHeadArgs& a, int slices, hipStream_t s) {
  hipLaunchKernelGGL(k_bnhead_apply_slices, dim3((unsigned)(a.nchunk * a.C), (unsigned)slices), dim3(256), 0, s, a);
}
void launch_bnhead_bwd_stats(const SBnHeadArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_bnhead_bwd_stats, head_grid(a), dim3(256), 0, s, a); }
void launch_bnhead_bwd_dx(const SBnHeadArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_bnhead_bwd_dx, head_grid(a), dim3(256), 0, s, a); }

}  // namespace node
