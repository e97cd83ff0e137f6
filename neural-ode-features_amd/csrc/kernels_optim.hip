// Fused optimizer steps.  SGD with momentum and weight decay exactly as torch.optim.SGD(lr, momentum, weight_decay)
// computes it (the reference's optimizer, train.py:136, stepped and zeroed at train.py:56-58), for EVERY parameter
// tensor of the model in one launch (a table of up to SGD_TABLE tensors travels in the kernel arguments):
//     g   = grad_scale * grad + weight_decay * p
//     buf = momentum * buf + g            (buf starts at zero, so the first step gives buf = g like PyTorch)
//     p   = p - lr * buf
// Gradients are read wherever autograd (or the data-parallel reducer's bucket) left them: no flattening pass.
// HBM-bound: 12 B read + 8 B written per element; ~2.0 M parameters at cfg 2 = 40 MB -> ~10 us.
#include "node_internal.h"

namespace node {

__global__ __launch_bounds__(256) void k_sgd_multi(SgdTable tb, float lr, float momentum, float wd, float gscale, const float* skip) {
  if (skip != nullptr && *skip != 0.f) return;   // a solve of this step reported a miss: nothing is committed
  const SgdEntry e = tb.e[blockIdx.y];
  float* __restrict__ p = e.p;
  const float* __restrict__ g = e.g;
  float* __restrict__ m = e.m;
  const size_t n = e.n;
  const size_t stride = (size_t)gridDim.x * 256;
  const size_t start = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) == 0;
  size_t done = 0;
  if (m == nullptr) {   // momentum == 0: torch.optim.SGD keeps no buffer then, p = p - lr (grad_scale grad + wd p)
    for (size_t i = start; i < n; i += stride) p[i] -= lr * (gscale * g[i] + wd * p[i]);
    return;
  }
  if (vec) {
    const size_t n4 = n >> 2;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    for (size_t i = start; i < n4; i += stride) {
      float4 pv = p4[i];
      const float4 gv = g4[i];
      float4 mv = m4[i];
      // same operation order as PyTorch's kernels: (grad + wd * p), (momentum * buf + g), (p - lr * buf)
      mv.x = momentum * mv.x + (gscale * gv.x + wd * pv.x);
      mv.y = momentum * mv.y + (gscale * gv.y + wd * pv.y);
      mv.z = momentum * mv.z + (gscale * gv.z + wd * pv.z);
      mv.w = momentum * mv.w + (gscale * gv.w + wd * pv.w);
      pv.x -= lr * mv.x; pv.y -= lr * mv.y; pv.z -= lr * mv.z; pv.w -= lr * mv.w;
      p4[i] = pv;
      m4[i] = mv;
    }
    done = n4 << 2;
  }
  for (size_t i = done + start; i < n; i += stride) {
    const float b = momentum * m[i] + (gscale * g[i] + wd * p[i]);
    m[i] = b;
    p[i] -= lr * b;
  }
}

void launch_sgd_multi(const SgdTable& tb, int count, size_t max_n, float lr, float momentum, float wd, float gscale,
                      const float* skip, hipStream_t s) {
  size_t bx = (max_n / 4 + 255) / 256;
  if (bx > 64) bx = 64;
  if (bx < 1) bx = 1;
  hipLaunchKernelGGL(k_sgd_multi, dim3((unsigned)bx, (unsigned)count), dim3(256), 0, s, tb, lr, momentum, wd, gscale, skip);
}

// Adam as torch.optim.Adam(lr, betas, eps, weight_decay) computes it (the reference's `-o adam`, train.py:138: amsgrad off,
// coupled L2 weight decay), same table form, in torch's operation order:
//     g = grad_scale * grad + weight_decay * p
//     m = m + (1 - b1) (g - m)                      (exp_avg.lerp_)
//     v = b2 v + (1 - b2) g g                       (exp_avg_sq.mul_().addcmul_())
//     t = step + 1
//     p = p - (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// `step` is one fp32 counter per tensor IN DEVICE MEMORY: a launch skipped by the flag must not advance it, and the host does
// not know the verdict when it launches.  k_adam_multi only READS the counters; k_adam_advance, one workgroup behind it on the
// stream and under the same predicate, adds 1 to each -- so no workgroup reads a word another one of its launch writes.
// HBM-bound: 16 B read + 12 B written per element.

// b^t for a whole t >= 0 by squaring, in double: the bias corrections are formed as PyTorch forms them (Python floats) and
// rounded to fp32 only as the two final factors.  t is wave-uniform, so is the loop.
__device__ inline double pow_whole(double b, float t) {
  double r = 1.0;
  for (unsigned k = (unsigned)t; k != 0; k >>= 1) {
    if (k & 1) r *= b;
    b *= b;
  }
  return r;
}

struct AdamCoef { float gscale, wd, w1, b2, w2, step_size, sqrt_c2, eps; };

__device__ inline void adam_elem(float& p, float g, float& m, float& v, const AdamCoef& c) {
  g = c.gscale * g + c.wd * p;
  m = m + c.w1 * (g - m);
  v = c.b2 * v + (c.w2 * g) * g;
  p = p - c.step_size * (m / (sqrtf(v) / c.sqrt_c2 + c.eps));
}

__global__ __launch_bounds__(256) void k_adam_multi(AdamTable tb, float lr, double b1, double b2, float eps, float wd, float gscale,
                                                    const float* skip) {
  if (skip != nullptr && *skip != 0.f) return;   // a solve of this step reported a miss: nothing is committed
  const AdamEntry e = tb.e[blockIdx.y];
  float* __restrict__ p = e.p;
  const float* __restrict__ g = e.g;
  float* __restrict__ m = e.m;
  float* __restrict__ v = e.v;
  const size_t n = e.n;
  const size_t stride = (size_t)gridDim.x * 256;
  const size_t start = (size_t)blockIdx.x * 256 + threadIdx.x;
  const float t = *e.step + 1.f;
  const double c1 = 1.0 - pow_whole(b1, t), c2 = 1.0 - pow_whole(b2, t);
  const AdamCoef c = {gscale, wd, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)((double)lr / c1), (float)sqrt(c2), eps};
  const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  size_t done = 0;
  if (vec) {
    const size_t n4 = n >> 2;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    for (size_t i = start; i < n4; i += stride) {
      float4 pv = p4[i];
      const float4 gv = g4[i];
      float4 mv = m4[i];
      float4 vv = v4[i];
      adam_elem(pv.x, gv.x, mv.x, vv.x, c);
      adam_elem(pv.y, gv.y, mv.y, vv.y, c);
      adam_elem(pv.z, gv.z, mv.z, vv.z, c);
      adam_elem(pv.w, gv.w, mv.w, vv.w, c);
      p4[i] = pv;
      m4[i] = mv;
      v4[i] = vv;
    }
    done = n4 << 2;
  }
  for (size_t i = done + start; i < n; i += stride) {
    float pv = p[i], mv = m[i], vv = v[i];
    adam_elem(pv, g[i], mv, vv, c);
    p[i] = pv;
    m[i] = mv;
    v[i] = vv;
  }
}

__global__ __launch_bounds__(ADAM_TABLE) void k_adam_advance(AdamTable tb, int count, const float* skip) {
  if (skip != nullptr && *skip != 0.f) return;   // a skipped step is not counted
  if ((int)threadIdx.x < count) *tb.e[threadIdx.x].step += 1.f;
}

void launch_adam_multi(const AdamTable& tb, int count, size_t max_n, float lr, double b1, double b2, float eps, float wd,
                       float gscale, const float* skip, hipStream_t s) {
  size_t bx = (max_n / 4 + 255) / 256;
  if (bx > 64) bx = 64;
  if (bx < 1) bx = 1;
  hipLaunchKernelGGL(k_adam_multi, dim3((unsigned)bx, (unsigned)count), dim3(256), 0, s, tb, lr, b1, b2, eps, wd, gscale, skip);
  hipLaunchKernelGGL(k_adam_advance, dim3(1), dim3(ADAM_TABLE), 0, s, tb, count, skip);
}

}  // namespace node
