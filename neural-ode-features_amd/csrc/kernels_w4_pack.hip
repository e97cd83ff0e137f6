// Winograd F(4x4,3x3) pipeline, stage 2: the once-per-solve filter transform (k_w4_pack), the scales of the fp16-pair operands
// (k_w4_scales) and the bf16 split checker.  gfx950 (MI355X / CDNA4) only.  See wino4.h for the data layouts.
#include "w4_gemm.h"

namespace node {

// ----------------------------------------------------------------------------
// U = G g G^T for every (co, ci) pair, written in MFMA-ready blocks (wino4.h).  dgrad: the data-gradient filter
// g'[ci][co][kh][kw] = g[co][ci][2-kh][2-kw].  Weights are [C][C+1][3][3] (input channel 0 = time, model.py:320-323).
// ----------------------------------------------------------------------------
// With jobs.ub: additionally the split-precision form k_w4_gemm64b reads -- every fp32 value u as three bf16 parts
// h = bf16(u), m = bf16(u - h), l = bf16(u - h - m) (u = h + m + l exactly), laid out [comp][cb][g/2][part 3][hi 2][col 32]
// [8 values: g even e 0..3, g odd e 0..3], i.e. one 16-B load per lane and part feeds one K = 16 bf16 MFMA.
__device__ __forceinline__ unsigned short w4_bf16_rne(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);   // round to nearest even (finite inputs)
}
__device__ __forceinline__ float w4_bf16_f32(unsigned short b) { return __builtin_bit_cast(float, (unsigned)b << 16); }

__global__ __launch_bounds__(256) void k_w4_pack(W4PackJobs jobs, int C) {
  const float* __restrict__ w = jobs.w[blockIdx.y];
  float* __restrict__ U = jobs.u[blockIdx.y];
  unsigned short* __restrict__ Ub = jobs.ub[blockIdx.y];
  _Float16* __restrict__ Uh = reinterpret_cast<_Float16*>(jobs.uh[blockIdx.y]);
  const float uscale = Uh != nullptr ? ldexpf(1.f, *jobs.uh_exp[blockIdx.y]) : 1.f;
  const int dgrad = jobs.dgrad[blockIdx.y];
  const int CI = jobs.plain[blockIdx.y] ? C : C + 1, c_off = jobs.plain[blockIdx.y] ? 0 : 1;   // input-channel stride / first data channel
  const int G8 = C >> 3;
  const size_t total = (size_t)C * C;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    // consecutive threads write consecutive elements of the layout this launch produces: fp32 [cb][g][hi][col][e], or
    // the bf16 triples [cb][g/2][part][hi][col][g & 1][e] (eight values = one 16-B operand of a lane)
    int e, col, hi, g, cb;
    if (Ub == nullptr && Uh == nullptr) {
      e = idx & 3; col = (idx >> 2) & 31; hi = (idx >> 7) & 1;
      g = (int)((idx >> 8) % G8); cb = (int)((idx >> 8) / G8);
    } else {
      e = idx & 3; col = (idx >> 3) & 31; hi = (idx >> 8) & 1;
      const int g2 = (int)((idx >> 9) % (G8 >> 1));
      g = 2 * g2 + (int)((idx >> 2) & 1); cb = (int)((idx >> 9) / (G8 >> 1));
    }
    const int nidx = cb * 32 + col, kidx = 8 * g + 4 * hi + e;   // output column / reduction index of the GEMM
    double gg[3][3];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
        gg[kh][kw] = dgrad ? (double)w[(((size_t)kidx * CI + c_off + nidx) * 3 + (2 - kh)) * 3 + (2 - kw)]
                           : (double)w[(((size_t)nidx * CI + c_off + kidx) * 3 + kh) * 3 + kw];
    double gt[6][3];   // G g
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) gt[i][kw] = W4_G[i][0] * gg[0][kw] + W4_G[i][1] * gg[1][kw] + W4_G[i][2] * gg[2][kw];
    const size_t fidx = ((((size_t)cb * G8 + g) * 2 + hi) * 32 + col) * 4 + e;
    const size_t bidx = ((((size_t)cb * (G8 >> 1) + (g >> 1)) * 3) * 64 + (size_t)(hi * 32 + col)) * 8 + (g & 1) * 4 + e;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int l = 0; l < 6; ++l) {
        const double v = gt[i][0] * W4_G[l][0] + gt[i][1] * W4_G[l][1] + gt[i][2] * W4_G[l][2];
        const float uf = (float)v;
        if (Uh != nullptr) {          // "U pairs" (wino4.h): [cb][g2][part][hi][col][gp][e], the parts 512 halves apart
          const float us = uf * uscale;
          const _Float16 hh = (_Float16)us;
          const _Float16 lh = (_Float16)(us - (float)hh);
          _Float16* o = Uh + (size_t)(i * 6 + l) * total * 2 + ((((size_t)cb * (G8 >> 1) + (g >> 1)) * 2) * 64 + (size_t)(hi * 32 + col)) * 8 + (g & 1) * 4 + e;
          o[0] = hh;
          o[512] = lh;
        }
        if (Ub != nullptr) {          // (an augmented solve prepares both: its first evaluations run the triples, wino4.h)
          const unsigned short hb = w4_bf16_rne(uf);
          const float r1 = uf - w4_bf16_f32(hb);
          const unsigned short mb = w4_bf16_rne(r1);
          const unsigned short lb = w4_bf16_rne(r1 - w4_bf16_f32(mb));
          unsigned short* o = Ub + (size_t)(i * 6 + l) * total * 3 + bidx;
          o[0] = hb;
          o[512] = mb;
          o[1024] = lb;
        }
        if (Ub == nullptr && Uh == nullptr) U[(size_t)(i * 6 + l) * total + fidx] = uf;
      }
  }
}
void launch_w4_pack(const W4PackJobs& jobs, int count, int C, hipStream_t s) {
  int blocks = (int)(((size_t)C * C + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(k_w4_pack, dim3(blocks, count), dim3(256), 0, s, jobs, C);
}

// diagnostics (node_w4_split3): the three parts of every element, as floats
__global__ __launch_bounds__(256) void k_w4_split_check(const float* __restrict__ x, float* __restrict__ out, size_t n8) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const float4 p = reinterpret_cast<const float4*>(x)[2 * i], q = reinterpret_cast<const float4*>(x)[2 * i + 1];
  const W4Split sp = w4_split8(p, q);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    out[(8 * i + k) * 3 + 0] = (float)sp.h[k];
    out[(8 * i + k) * 3 + 1] = (float)sp.m[k];
    out[(8 * i + k) * 3 + 2] = (float)sp.l[k];
  }
}
void launch_w4_split_check(const float* x, float* out, size_t n, hipStream_t s) {
  const size_t n8 = n / 8;
  hipLaunchKernelGGL(k_w4_split_check, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, x, out, n8);
}

// ----------------------------------------------------------------------------
// k_w4_scales: the power-of-two scales of a solve's fp16-pair operands (wino4.h, W4Scales) in one launch: block (x, job) adds the
// maximum of its slice of job's tensor by atomicMax on the fp32 bit pattern (non-negative floats order like unsigned integers);
// the last block to arrive derives the exponents and zeroes the scratch words for the next launch.
// ----------------------------------------------------------------------------
constexpr int W4SC_BLOCKS = 32;       // per big tensor (every block takes one returning ticket at the end: few blocks, several requests in flight each)
__global__ __launch_bounds__(256) void k_w4_scales(W4ScaleJobs j, int nbig) {
  __shared__ float red[4];
  // blocks [0, nbig W4SC_BLOCKS): slices of the big tensors (the conv weights; diagnostics: a whole activation tensor as "beta");
  // then one block per [C] vector
  int job, part, parts;
  if ((int)blockIdx.x < nbig * W4SC_BLOCKS) {
    const int b = blockIdx.x / W4SC_BLOCKS;
    part = blockIdx.x - b * W4SC_BLOCKS; parts = W4SC_BLOCKS;
    job = j.bigjob[b];
  } else {
    job = 2 + ((int)blockIdx.x - nbig * W4SC_BLOCKS); part = 0; parts = 1;
  }
  const float* p = job < 2 ? j.w[job] : j.gb[job - 2];
  size_t n = job < 2 ? j.wn : (size_t)j.C;
  const bool big_vec = (job == 3 || job == 5) && j.vn[(job - 3) >> 1] != 0;
  if (big_vec) n = j.vn[(job - 3) >> 1];
  if (parts == 1 && big_vec) p = nullptr;     // (a big "vector" is taken by its sliced blocks)
  float m = 0.f;
  if (p != nullptr) {
    const size_t i0 = (size_t)part * 256 + threadIdx.x, step = (size_t)parts * 256;
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && (n & 3) == 0) {      // 16-B loads, four in flight
      const float4* q = reinterpret_cast<const float4*>(p);
      const size_t n4 = n >> 2;
      for (size_t i = i0; i < n4; i += 4 * step) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = i + u * step < n4 ? q[i + u * step] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < 4; ++u) m = fmaxf(fmaxf(m, fmaxf(fabsf(v[u].x), fabsf(v[u].y))), fmaxf(fabsf(v[u].z), fabsf(v[u].w)));
      }
    } else {
      for (size_t i = i0; i < n; i += step) m = fmaxf(m, fabsf(p[i]));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x != 0) return;
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  W4Scales* sc = j.sc;
  if (m > 0.f) atomicMax(&sc->mx[job], __builtin_bit_cast(unsigned, m));
  __threadfence();
  const unsigned ticket = atomicAdd(&sc->arrived, 1u);
  if (ticket != gridDim.x - 1) return;
  __threadfence();
  float mx[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    mx[q] = __builtin_bit_cast(float, __hip_atomic_load(&sc->mx[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    __hip_atomic_store(&sc->mx[q], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __hip_atomic_store(&sc->arrived, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // |U| = |G g G^T| <= (28/15)^2 max|w|; ceiling 2^14 (a factor four under fp16's)
  if (j.w[0] != nullptr) sc->e[W4_E_U1] = w4_scale_exp(3.49f * mx[0], 14);
  if (j.w[1] != nullptr) sc->e[W4_E_U2] = w4_scale_exp(3.49f * mx[1], 14);
  // |B^T d B| <= 49 max|d|, d = relu(gamma xhat + beta), |xhat| <= sqrt(m - 1): ceiling 2^15 for the BOUND (what the data reaches is
  // typically 2^5 under it)
  const float rm = sqrtf((float)j.gn_m);
  if (j.gb[0] != nullptr || j.gb[1] != nullptr) sc->e[W4_E_V1] = w4_scale_exp(49.f * (rm * mx[2] + mx[3]), 15);
  if (j.gb[2] != nullptr || j.gb[3] != nullptr) sc->e[W4_E_V2] = w4_scale_exp(49.f * (rm * mx[4] + mx[5]), 15);
}
void launch_w4_scales(const W4ScaleJobs& j_in, hipStream_t s) {
  W4ScaleJobs j = j_in;
  int nbig = 0;      // the tensors cut over W4SC_BLOCKS blocks: the conv weights, and a "vector" with a length of its own (diagnostics)
  if (j.w[0] != nullptr) j.bigjob[nbig++] = 0;
  if (j.w[1] != nullptr) j.bigjob[nbig++] = 1;
  if (j.vn[0] != 0) j.bigjob[nbig++] = 3;
  if (j.vn[1] != 0) j.bigjob[nbig++] = 5;
  hipLaunchKernelGGL(k_w4_scales, dim3(nbig * W4SC_BLOCKS + 4), dim3(256), 0, s, j, nbig);
}

}  // namespace node
