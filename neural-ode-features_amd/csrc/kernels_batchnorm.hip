// BatchNorm with batch statistics (model.py:274: nn.BatchNorm2d(C, track_running_stats=False)) and the time channel of
// ConcatConv2d (model.py:313-323) for the stem's kernel family: what `norm='batch'` dynamics need around the gather GEMMs
// of kernels_stem.hip (batchnorm.h has the argument structures).
//
// Layout of every pass: a workgroup = (chunk of rows) x (64 channels) of an fp32 NHWC tensor [rows][C]; thread = eight
// consecutive channels (two 16-byte loads; eight lanes cover the 256 bytes = two cache lines of a row piece) of every 32nd row
// of the chunk, so a wave reads eight whole row pieces per instruction pair and the triples leave as 16-byte stores.
//
// Statistics, two stages, no atomics: k_bn_stats writes per (chunk, channel) the chunk's mean and its CENTRED second moment
// (mean pass, then a centred pass over the same rows, which then come from cache); the consumers (k_bn_apply) combine a
// channel's partials by Chan's formula in one fixed order (four interleaved chains, then those four).  E[x^2] - E[x]^2 loses the variance of
// x = 50 + randn to cancellation (2.7e-4 of max|y| against fp64); this form does not.  The backward's sums (sum dy, sum dy
// xhat) take the same two stages: k_bn_bwd_stats -> k_bn_bwd_dx.  Every sum has one order: the same bits on every run.
//
// The time channel: the convolution ran on w[:, 1:] with its bias in the epilogue; its output h lacks t * T[class][c]
// (batchnorm.h).  The term is added by the passes that READ h (statistics, apply, both backward passes), through one helper,
// so forward and backward see the same u bit for bit and the tensor is never rewritten: a term in the convolution's
// epilogue would need a variant of k_stem_conv, a materialised plane through its residual pointer a full tensor of traffic.
// Its gradients come out of the dx pass that writes the gradient of u: per (chunk, class, channel) sums and the workgroup's
// share of sum du * T; k_bn_reduce turns them into dW[:, 0], db and d_t.
//
// No loop or branch here depends on data: a NaN anywhere in the input reaches the statistics of its channel and from there
// every output of that channel (the ReLU keeps NaN, as torch's does).
#include "batchnorm.h"

namespace node {

namespace {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// x = h + m + l exactly (stem.h)
__device__ __forceinline__ void bn_split3(float x, bf16_t& h, bf16_t& m, bf16_t& l) {
  const __bf16 bh = (__bf16)x;
  const float r = x - (float)bh;
  const __bf16 bm = (__bf16)r;
  const float r2 = r - (float)bm;
  const __bf16 bl = (__bf16)r2;
  h = __builtin_bit_cast(bf16_t, bh);
  m = __builtin_bit_cast(bf16_t, bm);
  l = __builtin_bit_cast(bf16_t, bl);
}
__device__ __forceinline__ void bn_split8(const float (&v)[8], u32x4& hh, u32x4& mm, u32x4& ll) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 p = {v[2 * i], v[2 * i + 1]};
    const bf16x2 h = __builtin_convertvector(p, bf16x2);
    const f32x2 r = p - __builtin_convertvector(h, f32x2);
    const bf16x2 m = __builtin_convertvector(r, bf16x2);
    const f32x2 r2 = r - __builtin_convertvector(m, f32x2);
    const bf16x2 l = __builtin_convertvector(r2, bf16x2);
    hh[i] = __builtin_bit_cast(unsigned, h);
    mm[i] = __builtin_bit_cast(unsigned, m);
    ll[i] = __builtin_bit_cast(unsigned, l);
  }
}
__device__ __forceinline__ void store_triples(bf16_t* dst, size_t plane, const float (&v)[8]) {
  u32x4 hh, mm, ll;
  bn_split8(v, hh, mm, ll);
  *reinterpret_cast<u32x4*>(dst) = hh;
  *reinterpret_cast<u32x4*>(dst + plane) = mm;
  *reinterpret_cast<u32x4*>(dst + 2 * plane) = ll;
}
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
  reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}

// class of a row's pixel: 3 * (top, middle, bottom) + (left, middle, right); H, W >= 3 keep the classes apart
__device__ __forceinline__ int pixel_class(int row, int H, int W) {
  const int p = row % (H * W), y = p / W, x = p - y * W;
  return 3 * (y == 0 ? 0 : y == H - 1 ? 2 : 1) + (x == 0 ? 0 : x == W - 1 ? 2 : 1);
}
// tap k of a 3-tap axis lies inside the image for the pixels of axis class `cls`
__device__ __forceinline__ bool tap_inside(int k, int cls) { return k == 1 || (k == 0 ? cls != 0 : cls != 2); }

// the normalised tensor at (row, channels c .. c + 7): the ONE place that forms u, for every pass
__device__ __forceinline__ void load_u(const SBnArgs& a, float tv, int row, int c, float (&u)[8]) {
  load8(a.h + (size_t)row * a.C + c, u);
  if (a.T != nullptr) {
    float tt[8];
    load8(a.T + (size_t)pixel_class(row, a.H, a.W) * a.C + c, tt);
#pragma unroll
    for (int k = 0; k < 8; ++k) u[k] = __builtin_fmaf(tv, tt[k], u[k]);
  }
}
__device__ __forceinline__ float bn_xhat(float u, float mean, float rstd) { return (u - mean) * rstd; }
__device__ __forceinline__ float bn_y(float xh, float g, float b) { return __builtin_fmaf(xh, g, b); }

// the thread's eight column sums -> the sums over the workgroup's 32 row slots, in row-slot order: thread t < 64 returns
// column t's, the others 0.  red: [32][64].  Ends behind a barrier (red is free again).
__device__ __forceinline__ float colsum64(const float (&s)[8], float* red, int t) {
  store8(red + (t >> 3) * 64 + 8 * (t & 7), s);
  __syncthreads();
  float r = 0.f;
  if (t < 64) {
#pragma unroll 8
    for (int j = 0; j < 32; ++j) r += red[j * 64 + t];
  }
  __syncthreads();
  return r;
}

// the same sums taken in fp64 (the backward's sum dy and sum dy xhat: see k_bn_bwd_stats)
__device__ __forceinline__ double colsum64d(const float (&s)[8], float* red, int t) {
  store8(red + (t >> 3) * 64 + 8 * (t & 7), s);
  __syncthreads();
  double r = 0.0;
  if (t < 64) {
#pragma unroll 8
    for (int j = 0; j < 32; ++j) r += (double)red[j * 64 + t];
  }
  __syncthreads();
  return r;
}

// sl, k: the chunk's slice and its index inside the slice (SLICED; otherwise 0 and the chunk itself)
struct Geo { int chunk, c0, c, r0, r1, rr, sl, k; };
// SLICED (batchnorm.h): chunks never straddle a slice -- chunk = slice * chunks_per_slice + k covers the rows
// slice * rows_per_slice + k * chunk_rows .. of its own slice only, the last one of every slice possibly short.  A variant at compile
// time, so the unsliced instances every other node launches keep their instruction streams.
template <bool SLICED = false>
__device__ __forceinline__ Geo bn_geo(const SBnArgs& a) {
  Geo g;
  const int nct = a.C >> 6, t = threadIdx.x;
  g.chunk = blockIdx.x / nct;
  g.c0 = (blockIdx.x - g.chunk * nct) << 6;
  g.c = g.c0 + 8 * (t & 7);
  g.rr = t >> 3;
  if constexpr (SLICED) {
    g.sl = g.chunk / a.chunks_per_slice;
    g.k = g.chunk - g.sl * a.chunks_per_slice;
    const int s0 = g.sl * a.rows_per_slice;
    g.r0 = s0 + g.k * a.chunk_rows;
    g.r1 = min(g.r0 + a.chunk_rows, s0 + a.rows_per_slice);
  } else {
    g.sl = 0;
    g.k = g.chunk;
    g.r0 = g.chunk * a.chunk_rows;
    g.r1 = min(g.r0 + a.chunk_rows, a.rows);
  }
  return g;
}

// ============================================================================
// forward, stage 1: per (chunk, channel) the chunk's mean and centred second moment
// ============================================================================
template <bool SLICED>
__global__ __launch_bounds__(256) void k_bn_stats(const SBnArgs a) {
  __shared__ __align__(16) float red[32 * 64];
  __shared__ float cm[64];
  const int t = threadIdx.x;
  const Geo g = bn_geo<SLICED>(a);
  const float tv = a.T != nullptr ? *a.t : 0.f;
  float s[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = 0.f;
  for (int r = g.r0 + g.rr; r < g.r1; r += 32) {
    float u[8];
    load_u(a, tv, r, g.c, u);
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] += u[k];
  }
  const float sum = colsum64(s, red, t);
  const float mean = sum / (float)(g.r1 - g.r0);
  if (t < 64) cm[t] = mean;
  __syncthreads();
  float m[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { m[k] = cm[8 * (t & 7) + k]; s[k] = 0.f; }
  for (int r = g.r0 + g.rr; r < g.r1; r += 32) {
    float u[8];
    load_u(a, tv, r, g.c, u);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float d = u[k] - m[k];
      s[k] = __builtin_fmaf(d, d, s[k]);
    }
  }
  const float m2 = colsum64(s, red, t);
  if (t < 64) {
    a.part[((size_t)g.chunk * 2 + 0) * a.C + g.c0 + t] = mean;
    a.part[((size_t)g.chunk * 2 + 1) * a.C + g.c0 + t] = m2;
  }
}

// Chan's update of (n, mean, M2) by a chunk of nk > 0 rows
__device__ __forceinline__ void chan_merge(float& n, float& m, float& M2, float nk, float mk, float Mk) {
  const float tot = n + nk, f = nk / tot, d = mk - m;
  m = __builtin_fmaf(d, f, m);
  M2 = M2 + Mk + d * d * n * f;
  n = tot;
}
// the batch statistics of the workgroup's 64 channels from the partials: thread (c = t % 64, q = t / 64) merges chunks q, q + 4, ..,
// thread c then the four chains in order.  sm: [4][3][64].  mean, rstd: [64], valid behind the closing barrier.
// SLICED: only the chunks_per_slice partials of slice `sl`, in the same order, over rows_per_slice rows: what an unsliced call on
// that slice alone combines, so the same bits.
template <bool SLICED>
__device__ __forceinline__ void bn_combine(const SBnArgs& a, int c0, int sl, float* sm, float* mean, float* rstd, int t) {
  const int c = t & 63, q = t >> 6;
  const int nk_all = SLICED ? a.chunks_per_slice : a.nchunk, rows = SLICED ? a.rows_per_slice : a.rows;
  const float* part = SLICED ? a.part + (size_t)sl * a.chunks_per_slice * 2 * a.C : a.part;
  float n = 0.f, m = 0.f, M2 = 0.f;
  for (int k = q; k < nk_all; k += 4) {
    const float nk = (float)min(a.chunk_rows, rows - k * a.chunk_rows);
    chan_merge(n, m, M2, nk, part[((size_t)k * 2 + 0) * a.C + c0 + c], part[((size_t)k * 2 + 1) * a.C + c0 + c]);
  }
  sm[(q * 3 + 0) * 64 + c] = n;
  sm[(q * 3 + 1) * 64 + c] = m;
  sm[(q * 3 + 2) * 64 + c] = M2;
  __syncthreads();
  if (t < 64) {
    n = sm[t]; m = sm[64 + t]; M2 = sm[128 + t];
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      const float nj = sm[(j * 3 + 0) * 64 + t];
      if (nj > 0.f) chan_merge(n, m, M2, nj, sm[(j * 3 + 1) * 64 + t], sm[(j * 3 + 2) * 64 + t]);     // (fewer than four chunks: a shape's property, not the data's)
    }
    mean[t] = m;
    rstd[t] = 1.f / sqrtf(M2 / (float)rows + a.eps);
  }
  __syncthreads();
}

// ============================================================================
// forward, stage 2: y = [relu](xhat gamma + beta) as triples and / or fp32
// ============================================================================
template <bool SLICED>
__global__ __launch_bounds__(256) void k_bn_apply(const SBnArgs a) {
  __shared__ float sm[4 * 3 * 64];
  __shared__ float smean[64], srstd[64];
  const int t = threadIdx.x;
  const Geo g = bn_geo<SLICED>(a);
  bn_combine<SLICED>(a, g.c0, g.sl, sm, smean, srstd, t);
  if (g.k == 0 && t < 64) {      // the first chunk of the slice: stats [slices][2][C]
    float* st = SLICED ? a.stats + (size_t)g.sl * 2 * a.C : a.stats;
    st[g.c0 + t] = smean[t];
    st[a.C + g.c0 + t] = srstd[t];
  }
  const float tv = a.T != nullptr ? *a.t : 0.f;
  float mu[8], rs[8], ga[8], be[8];
  load8(a.gamma + g.c, ga);
  load8(a.beta + g.c, be);
#pragma unroll
  for (int k = 0; k < 8; ++k) { mu[k] = smean[8 * (t & 7) + k]; rs[k] = srstd[8 * (t & 7) + k]; }
  for (int r = g.r0 + g.rr; r < g.r1; r += 32) {
    float u[8];
    load_u(a, tv, r, g.c, u);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float y = bn_y(bn_xhat(u[k], mu[k], rs[k]), ga[k], be[k]);
      u[k] = (a.relu && y < 0.f) ? 0.f : y;
    }
    const size_t o = (size_t)r * a.C + g.c;
    if (a.a3) store_triples(a.a3 + o, a.a_plane, u);
    if (a.y) {
#pragma unroll
      for (int k = 0; k < 8; ++k) u[k] *= a.out_scale;
      store8(a.y + o, u);
    }
  }
}

// ============================================================================
// backward, stage 1: per (chunk, channel) sum dy and sum dy xhat, dy = da behind the ReLU mask recomputed from xhat
// The partials and their combination are fp64 from the thread's own few rows on: an error e of mean(dy) shifts EVERY du of the channel
// by the same amount, so sum du -- zero identically, and what d_t = sum du * T relies on to cancel the interior's share -- is off by
// rows * e; with fp32 partials that cost d_t 3e-5 of its value at 4096 rows.
// ============================================================================
__global__ __launch_bounds__(256) void k_bn_bwd_stats(const SBnArgs a) {
  __shared__ __align__(16) float red[32 * 64];
  const int t = threadIdx.x;
  const Geo g = bn_geo(a);
  const float tv = a.T != nullptr ? *a.t : 0.f;
  float mu[8], rs[8], ga[8], be[8], sA[8], sB[8];
  load8(a.stats + g.c, mu);
  load8(a.stats + a.C + g.c, rs);
  load8(a.gamma + g.c, ga);
  load8(a.beta + g.c, be);
#pragma unroll
  for (int k = 0; k < 8; ++k) sA[k] = sB[k] = 0.f;
  for (int r = g.r0 + g.rr; r < g.r1; r += 32) {
    float u[8], dy[8];
    load_u(a, tv, r, g.c, u);
    load8(a.da + (size_t)r * a.C + g.c, dy);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float xh = bn_xhat(u[k], mu[k], rs[k]);
      const float d = (a.relu && bn_y(xh, ga[k], be[k]) <= 0.f) ? 0.f : a.da_scale * dy[k];
      sA[k] += d;
      sB[k] = __builtin_fmaf(d, xh, sB[k]);
    }
  }
  const double A = colsum64d(sA, red, t);
  const double B = colsum64d(sB, red, t);
  if (t < 64) {
    a.gpart[((size_t)g.chunk * 2 + 0) * a.C + g.c0 + t] = A;
    a.gpart[((size_t)g.chunk * 2 + 1) * a.C + g.c0 + t] = B;
  }
}

// ============================================================================
// backward, stage 2: du = rstd gamma (dy - mean(dy) - xhat mean(dy xhat)); dgamma = sum dy xhat, dbeta = sum dy (chunk 0 writes them)
// TIME: also the per-class sums of du and the workgroup's share of sum du * T.  Every thread owns 9 x 8 accumulators in LDS
// (a row's class is one index into them: registers would need a dynamic index).
// SKIP (only without TIME: the residual trunk's norm1, whose input also is the block's shortcut): the gradient written is du + skip.
// A variant at compile time, so the two instances the dynamics launch keep their instruction streams.
// ============================================================================
template <bool TIME, bool SKIP = false>
__global__ __launch_bounds__(256) void k_bn_bwd_dx(const SBnArgs a) {
  extern __shared__ __align__(16) unsigned char dyn[];      // (no static __shared__ next to a dynamic region above 64 KB: the attribute call refuses their sum)
  float* sm = reinterpret_cast<float*>(dyn);                // [4][2][64] doubles
  float* sAs = sm + 1024;                                   // [64]
  float* sBs = sAs + 64;                                    // [64]
  const int t = threadIdx.x;
  const Geo g = bn_geo(a);
  {
    const int c = t & 63, q = t >> 6;
    double* dsm = reinterpret_cast<double*>(sm);          // [4][2][64]
    double A = 0.0, B = 0.0;
    for (int k = q; k < a.nchunk; k += 4) {
      A += a.gpart[((size_t)k * 2 + 0) * a.C + g.c0 + c];
      B += a.gpart[((size_t)k * 2 + 1) * a.C + g.c0 + c];
    }
    dsm[(q * 2 + 0) * 64 + c] = A;
    dsm[(q * 2 + 1) * 64 + c] = B;
    __syncthreads();
    if (t < 64) {
      A = (dsm[t] + dsm[128 + t]) + (dsm[256 + t] + dsm[384 + t]);
      B = (dsm[64 + t] + dsm[192 + t]) + (dsm[320 + t] + dsm[448 + t]);
    }
    __syncthreads();
    if (t < 64) {
      sAs[t] = (float)(A / (double)a.rows);             // mean(dy), mean(dy xhat)
      sBs[t] = (float)(B / (double)a.rows);
      if (g.chunk == 0) {
        if (a.dgamma) a.dgamma[g.c0 + t] = (float)B;
        if (a.dbeta) a.dbeta[g.c0 + t] = (float)A;
      }
    }
    __syncthreads();
  }
  const float tv = a.T != nullptr ? *a.t : 0.f;
  float mu[8], rs[8], ga[8], be[8], mA[8], mB[8];
  load8(a.stats + g.c, mu);
  load8(a.stats + a.C + g.c, rs);
  load8(a.gamma + g.c, ga);
  load8(a.beta + g.c, be);
#pragma unroll
  for (int k = 0; k < 8; ++k) { mA[k] = sAs[8 * (t & 7) + k]; mB[k] = sBs[8 * (t & 7) + k]; }
  float* lacc = sBs + 64;                                   // TIME: [9][256][8], then [9][64] doubles
  if constexpr (TIME) {
    float z[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) z[k] = 0.f;
#pragma unroll
    for (int cls = 0; cls < 9; ++cls) store8(lacc + ((size_t)cls * 256 + t) * 8, z);
  }
  for (int r = g.r0 + g.rr; r < g.r1; r += 32) {
    float u[8], dy[8];
    load_u(a, tv, r, g.c, u);
    load8(a.da + (size_t)r * a.C + g.c, dy);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float xh = bn_xhat(u[k], mu[k], rs[k]);
      const float d = (a.relu && bn_y(xh, ga[k], be[k]) <= 0.f) ? 0.f : a.da_scale * dy[k];
      u[k] = rs[k] * ga[k] * __builtin_fmaf(-xh, mB[k], d - mA[k]);     // (explicit: both instances of this kernel round alike)
    }
    const size_t o = (size_t)r * a.C + g.c;
    if constexpr (SKIP) {
      float sk[8];
      load8(a.skip + o, sk);
#pragma unroll
      for (int k = 0; k < 8; ++k) u[k] += sk[k];
    }
    if (a.dh) store8(a.dh + o, u);
    if (a.dh3) store_triples(a.dh3 + o, a.dh_plane, u);
    if constexpr (TIME) {
      float* slot = lacc + ((size_t)pixel_class(r, a.H, a.W) * 256 + t) * 8;
      float acc[8];
      load8(slot, acc);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += u[k];
      store8(slot, acc);
    }
  }
  if constexpr (TIME) {
    // sum du * T cancels heavily: du is a BatchNorm backward's output, so sum du = 0 per channel identically and only the border
    // classes' deviation from the interior's T (class 4) counts.  The share is therefore taken as sum du * (T - T[4]) -- the same
    // number in exact arithmetic, without the rounding noise of sum du (which is the bias gradient) times T[4] -- and in fp64 from
    // here on: long fp32 chains over (class, channel, chunk) lost 5e-5 of d_t at 4096 rows.
    double* prod = reinterpret_cast<double*>(lacc + 9 * 256 * 8);     // [9][64]
    double* dsm = reinterpret_cast<double*>(sm);                      // [64]
    __syncthreads();
    for (int o = t; o < 9 * 64; o += 256) {
      const int cls = o >> 6, cc = o & 63;
      float s = 0.f;
#pragma unroll 8
      for (int j = 0; j < 32; ++j) s += lacc[((size_t)cls * 256 + j * 8 + (cc >> 3)) * 8 + (cc & 7)];
      a.clsp[((size_t)g.chunk * 9 + cls) * a.C + g.c0 + cc] = s;
      prod[o] = (double)s * ((double)a.T[(size_t)cls * a.C + g.c0 + cc] - (double)a.T[(size_t)4 * a.C + g.c0 + cc]);
    }
    __syncthreads();
    if (t < 64) {
      double s = 0.0;
#pragma unroll
      for (int cls = 0; cls < 9; ++cls) s += prod[cls * 64 + t];
      dsm[t] = s;
    }
    __syncthreads();
    if (t == 0) {
      double s = 0.0;
      for (int j = 0; j < 64; ++j) s += dsm[j];
      a.dtp[(size_t)g.chunk * (a.C >> 6) + (g.c0 >> 6)] = s;
    }
  }
}

// ============================================================================
// once per forward: filters' x part -> triples (both operand layouts), time tables, zero rows
// ============================================================================
__global__ __launch_bounds__(256) void k_bn_prep(const SBnPrepArgs a, unsigned blk_t, unsigned blk_z) {
  const int C = a.C;
  const size_t total = (size_t)9 * C * C;
  if (blockIdx.x < blk_t) {
    const unsigned per = blk_t >> 1;
    const int j = blockIdx.x >= per ? 1 : 0;
    const size_t idx = (size_t)(blockIdx.x - j * per) * 256 + threadIdx.x;
    if (idx >= total) return;
    const float* w = j ? a.w[1] : a.w[0];
    bf16_t* wf = j ? a.wf[1] : a.wf[0];
    bf16_t* wd = j ? a.wd[1] : a.wd[0];
    const int ci = (int)(idx % C);
    const size_t r = idx / C;
    const int co = (int)(r % C), tap = (int)(r / C);
    const float v = w[((size_t)co * (C + 1) + 1 + ci) * 9 + tap];
    bf16_t h, m, l;
    bn_split3(v, h, m, l);
    const size_t of = ((size_t)tap * C + co) * C + ci, od = ((size_t)tap * C + ci) * C + co;
    wf[of] = h; wf[of + total] = m; wf[of + 2 * total] = l;
    wd[od] = h; wd[od + total] = m; wd[od + 2 * total] = l;
    return;
  }
  if (blockIdx.x < blk_z) {      // T[j][cls][co] = sum of w[co][0][ky][kx] over the taps inside the image for class cls
    const int idx = (int)(blockIdx.x - blk_t) * 256 + threadIdx.x;
    if (idx >= 2 * 9 * C) return;
    const int j = idx / (9 * C), rem = idx - j * 9 * C, cls = rem / C, co = rem - cls * C;
    const float* w = (j ? a.w[1] : a.w[0]) + (size_t)co * (C + 1) * 9;
    const int cy = cls / 3, cx = cls - 3 * cy;
    float s = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
        if (tap_inside(ky, cy) && tap_inside(kx, cx)) s += w[ky * 3 + kx];
    (j ? a.T[1] : a.T[0])[rem] = s;
    return;
  }
  const int idx = (int)(blockIdx.x - blk_z) * 256 + threadIdx.x;
  const int which = idx / C, e = idx - which * C;
  if (which >= a.nzero * 3) return;
  const int ten = which / 3, p = which - 3 * ten;
  bf16_t* z = ten == 0 ? a.zero[0] : ten == 1 ? a.zero[1] : a.zero[2];
  const size_t plane = ten == 0 ? a.zero_plane[0] : ten == 1 ? a.zero_plane[1] : a.zero_plane[2];
  z[p * plane + e] = 0;
}

// ============================================================================
// once per backward.  Workgroups, in this order:
//   [want_params] 2 x (C x 9): slab sums of one (output channel, tap) -> dW[co][1 + ci][tap] (k_stem_reduce's kind 0 with the
//                 pitch of the [C][C + 1][3][3] filter)
//   [want_params] 2 x (C / 64): the class sums of 64 channels over the chunks -> db[c] and dW[c][0][ky][kx] = t * (sum over the
//                 classes whose pixels have tap (ky, kx) inside)
//   1:            d_t = the sum of both convolutions' workgroup shares, in index order
// ============================================================================
__global__ __launch_bounds__(256) void k_bn_reduce(const SBnReduceArgs a) {
  __shared__ __align__(8) float part[4][9 * 64];
  const int t = threadIdx.x, C = a.C;
  const unsigned nslab = a.want_params ? (unsigned)C * 9 : 0u, ntime = a.want_params ? (unsigned)(C >> 6) : 0u;
  unsigned bx = blockIdx.x;
  if (bx < 2 * nslab) {
    const int j = bx >= nslab ? 1 : 0;
    bx -= j * nslab;
    const float* slab = j ? a.slab1 : a.slab0;
    float* out = j ? a.dw1 : a.dw0;
    const int ns = j ? a.ns1 : a.ns0;
    const int co = bx / 9, tap = bx - co * 9;
    const size_t total = (size_t)9 * C * C;
    const int cl = t & 63, sub = t >> 6;
    for (int c0 = 0; c0 < C; c0 += 64) {
      const float* src = slab + ((size_t)tap * C + co) * C + c0 + cl;
      float s0 = 0.f, s1 = 0.f;
      int k = sub;
      for (; k + 4 < ns; k += 8) {
        s0 += src[(size_t)k * total];
        s1 += src[(size_t)(k + 4) * total];
      }
      if (k < ns) s0 += src[(size_t)k * total];
      part[sub][cl] = s0 + s1;
      __syncthreads();
      if (sub == 0) out[((size_t)co * (C + 1) + 1 + c0 + cl) * 9 + tap] = (part[0][cl] + part[1][cl]) + (part[2][cl] + part[3][cl]);
      __syncthreads();
    }
    return;
  }
  bx -= 2 * nslab;
  if (bx < 2 * ntime) {
    const int j = bx >= ntime ? 1 : 0;
    bx -= j * ntime;
    const float* clsp = j ? a.clsp1 : a.clsp0;
    float* dw = j ? a.dw1 : a.dw0;
    float* db = j ? a.db1 : a.db0;
    const int c0 = bx << 6, c = t & 63, q = t >> 6;
#pragma unroll
    for (int cls = 0; cls < 9; ++cls) {
      float s = 0.f;
      for (int k = q; k < a.nchunk; k += 4) s += clsp[((size_t)k * 9 + cls) * C + c0 + c];
      part[q][cls * 64 + c] = s;
    }
    __syncthreads();
    if (t < 64) {
      float S[9];
#pragma unroll
      for (int cls = 0; cls < 9; ++cls)
        S[cls] = (part[0][cls * 64 + t] + part[1][cls * 64 + t]) + (part[2][cls * 64 + t] + part[3][cls * 64 + t]);
      float sb = 0.f;
#pragma unroll
      for (int cls = 0; cls < 9; ++cls) sb += S[cls];
      db[c0 + t] = sb;
      const float tv = *a.t;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          float m = 0.f;
#pragma unroll
          for (int cls = 0; cls < 9; ++cls)
            if (tap_inside(ky, cls / 3) && tap_inside(kx, cls % 3)) m += S[cls];
          dw[(size_t)(c0 + t) * (C + 1) * 9 + ky * 3 + kx] = tv * m;
        }
    }
    return;
  }
  if (a.d_t == nullptr) return;
  const int n = a.nchunk * (C >> 6);
  double* dpart = reinterpret_cast<double*>(&part[0][0]);      // [256]
  double s = 0.0;
  for (int i = t; i < n; i += 256) s += a.dtp1[i];        // conv2's term first: the order the backward produced them in
  for (int i = t; i < n; i += 256) s += a.dtp0[i];
  dpart[t] = s;
  __syncthreads();
  if (t == 0) {
    double d = 0.0;
    for (int i = 0; i < 256; ++i) d += dpart[i];
    *a.d_t = (float)d;
  }
}

// ============================================================================
// the small passes of a solve: <a, b> in two stages (fp64 partials, one order), y += x, a device scalar
// ============================================================================
__global__ __launch_bounds__(256) void k_bn_dot(const float* __restrict__ x, const float* __restrict__ y, size_t n4, double* __restrict__ part) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const size_t stride = (size_t)gridDim.x * 256;
  double s = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + t; i < n4; i += stride) {
    const float4 a = reinterpret_cast<const float4*>(x)[i], b = reinterpret_cast<const float4*>(y)[i];
    s += ((double)a.x * (double)b.x + (double)a.y * (double)b.y) + ((double)a.z * (double)b.z + (double)a.w * (double)b.w);
  }
  red[t] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) part[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(64) void k_bn_dot_final(const double* __restrict__ part, int nblk, float* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < nblk; ++i) s += part[i];
  *out = (float)s;
}
__global__ __launch_bounds__(256) void k_bn_add(float* __restrict__ y, const float* __restrict__ x, size_t n4) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 a = reinterpret_cast<float4*>(y)[i];
    const float4 b = reinterpret_cast<const float4*>(x)[i];
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    reinterpret_cast<float4*>(y)[i] = a;
  }
}
__global__ void k_bn_set_scalar(float* dst, float v) { *dst = v; }

}  // namespace

// ============================================================================
// launchers
// ============================================================================
int bn_chunk_rows(int rows, int C) {
  int maxchunk = 256 / (C >> 6);
  if (maxchunk > 128) maxchunk = 128;
  if (maxchunk < 16) maxchunk = 16;
  int cr = (rows + maxchunk - 1) / maxchunk;
  cr = (cr + 31) & ~31;
  return cr < 32 ? 32 : cr;
}
static dim3 bn_grid(const SBnArgs& a) { return dim3((unsigned)(a.nchunk * (a.C >> 6))); }

// slices > 1: the sliced instances (nchunk = slices * chunks_per_slice); everything else launches the unsliced ones
void launch_bn_stats(const SBnArgs& a, hipStream_t s) {
  if (a.slices > 1) hipLaunchKernelGGL(k_bn_stats<true>, bn_grid(a), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_bn_stats<false>, bn_grid(a), dim3(256), 0, s, a);
}
void launch_bn_apply(const SBnArgs& a, hipStream_t s) {
  if (a.slices > 1) hipLaunchKernelGGL(k_bn_apply<true>, bn_grid(a), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_bn_apply<false>, bn_grid(a), dim3(256), 0, s, a);
}
void launch_bn_bwd_stats(const SBnArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_bn_bwd_stats, bn_grid(a), dim3(256), 0, s, a); }
void launch_bn_bwd_dx(const SBnArgs& a, hipStream_t s) {
  if (a.clsp != nullptr) {
    static bool attr[MAX_DEVICES] = {};
    allow_full_lds(reinterpret_cast<const void*>(k_bn_bwd_dx<true>), attr);
    const size_t lds = ((size_t)1152 + 9 * 256 * 8) * sizeof(float) + 9 * 64 * sizeof(double);
    hipLaunchKernelGGL(k_bn_bwd_dx<true>, bn_grid(a), dim3(256), lds, s, a);
  } else if (a.skip != nullptr) {
    hipLaunchKernelGGL((k_bn_bwd_dx<false, true>), bn_grid(a), dim3(256), 1152 * sizeof(float), s, a);
  } else {
    hipLaunchKernelGGL(k_bn_bwd_dx<false>, bn_grid(a), dim3(256), 1152 * sizeof(float), s, a);
  }
}
void launch_bn_prep(const SBnPrepArgs& a, hipStream_t s) {
  const unsigned per = (unsigned)(((size_t)9 * a.C * a.C + 255) / 256);
  const unsigned blk_t = 2 * per;
  const unsigned blk_z = blk_t + (unsigned)((2 * 9 * a.C + 255) / 256);
  const unsigned end = blk_z + (unsigned)((a.nzero * 3 * a.C + 255) / 256);
  hipLaunchKernelGGL(k_bn_prep, dim3(end), dim3(256), 0, s, a, blk_t, blk_z);
}
void launch_bn_reduce(const SBnReduceArgs& a, hipStream_t s) {
  const unsigned grid = (a.want_params ? 2u * ((unsigned)a.C * 9 + (unsigned)(a.C >> 6)) : 0u) + 1u;
  hipLaunchKernelGGL(k_bn_reduce, dim3(grid), dim3(256), 0, s, a);
}
static unsigned flat_blocks(size_t n4, unsigned cap) {
  const size_t b = (n4 + 255) / 256;
  return b > cap ? cap : b < 1 ? 1u : (unsigned)b;
}
void launch_bn_dot(const float* a, const float* b, size_t n, double* part, float* out, hipStream_t s) {
  const unsigned blocks = flat_blocks(n / 4, BN_DOT_BLOCKS);
  hipLaunchKernelGGL(k_bn_dot, dim3(blocks), dim3(256), 0, s, a, b, n / 4, part);
  hipLaunchKernelGGL(k_bn_dot_final, dim3(1), dim3(64), 0, s, part, (int)blocks, out);
}
void launch_bn_add(float* y, const float* x, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_bn_add, dim3(flat_blocks(n / 4, 2048)), dim3(256), 0, s, y, x, n / 4);
}
void launch_bn_set_scalar(float* dst, float v, hipStream_t s) { hipLaunchKernelGGL(k_bn_set_scalar, dim3(1), dim3(1), 0, s, dst, v); }

}  // namespace node
