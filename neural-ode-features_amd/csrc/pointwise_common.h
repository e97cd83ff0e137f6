// Device helpers of the HBM-bound kernels (kernels_groupnorm.hip, kernels_step_control.hip, kernels_generic.hip,
// kernels_theta_finalize.hip): wave and workgroup reductions in a fixed order, 16-byte loads and stores.
#pragma once
#include "node_internal.h"

namespace node {

__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ inline float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// deterministic block sum (256 threads), result valid in every thread
__device__ inline float block_sum_256(float v, float* red /*[4]*/) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ inline float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ inline void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// the ERR_BLOCKS = 512 per-workgroup partial sums of a norm pass, by one 256-thread workgroup
__device__ inline float reduce_partials_512(const float* p, float* red) {
  float v = p[threadIdx.x] + p[threadIdx.x + 256];
  return block_sum_256(v, red);
}

}  // namespace node
