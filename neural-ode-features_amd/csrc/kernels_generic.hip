// Helper kernels of the generic solver (api_flat.hip: dynamics evaluated by the caller, flat state) and of backprop through the steps:
// axpy, its fan-out over several tensors, fill, and the dot product behind adj_t.
#include "pointwise_common.h"

namespace node {

__global__ __launch_bounds__(256) void k_axpy(float* y, const float* x, float alpha, size_t n) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) y[i] += alpha * x[i];
}
void launch_axpy(float* y, const float* x, float alpha, size_t n, hipStream_t s) {
  size_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_axpy, dim3((unsigned)blocks), dim3(256), 0, s, y, x, alpha, n);
}
__global__ __launch_bounds__(256) void k_scatter_axpy(ScatterArgs a) {
  const size_t stride = (size_t)gridDim.x * 256;
  const size_t n4 = a.n >> 2;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const float4 v = reinterpret_cast<const float4*>(a.src)[i];
    for (int q = 0; q < a.nt; ++q) {
      float4* d = reinterpret_cast<float4*>(a.dst[q]) + i;
      float4 o = *d;
      const float c = a.coef[q];
      o.x += c * v.x; o.y += c * v.y; o.z += c * v.z; o.w += c * v.w;
      *d = o;
    }
  }
  if (blockIdx.x == 0)
    for (size_t i = (n4 << 2) + threadIdx.x; i < a.n; i += 256)
      for (int q = 0; q < a.nt; ++q) a.dst[q][i] += a.coef[q] * a.src[i];
}
void launch_scatter_axpy(const ScatterArgs& a, hipStream_t s) {
  if (a.nt <= 0 || a.n == 0) return;
  size_t blocks = (a.n / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_scatter_axpy, dim3((unsigned)blocks), dim3(256), 0, s, a);
}
__global__ __launch_bounds__(256) void k_fill(float* p, float v, size_t n) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) p[i] = v;
}
void launch_fill(float* p, float v, size_t n, hipStream_t s) {
  size_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks == 0) return;
  hipLaunchKernelGGL(k_fill, dim3((unsigned)blocks), dim3(256), 0, s, p, v, n);
}

// adj_t <- adj_t - <f_i, g_i>     (adjoint: "effect of moving the current time measurement point")
__global__ __launch_bounds__(256) void k_dot_partial(const float* a, const float* b, size_t n, float* partial) {
  __shared__ float red[4];
  float acc = 0.f;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) acc += a[i] * b[i];
  const float tot = block_sum_256(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}
__global__ __launch_bounds__(256) void k_dot_final(Ctrl* c, const float* partial, float sign, float* out_dot) {
  __shared__ float red[4];
  const float tot = sign * reduce_partials_512(partial, red);
  if (threadIdx.x == 0) {
    c->ts_cur = c->ts_cur - tot;
    if (out_dot) *out_dot = tot;
  }
}
void launch_dot_sub_scalar(Ctrl* ctrl, const float* a, const float* b, size_t n, float sign, float* partial, float* out_dot, hipStream_t s) {
  hipLaunchKernelGGL(k_dot_partial, dim3(ERR_BLOCKS), dim3(256), 0, s, a, b, n, partial);
  hipLaunchKernelGGL(k_dot_final, dim3(1), dim3(256), 0, s, ctrl, partial, sign, out_dot);
}
__global__ void k_copy_scalar_out(const Ctrl* c, float* dst) { *dst = c->ts_cur; }
void launch_copy_scalar_out(const Ctrl* ctrl, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(k_copy_scalar_out, dim3(1), dim3(1), 0, s, ctrl, dst);
}

}  // namespace node
