// The basic-iterative (BIM / PGD) attack's per-iteration arithmetic: two launches per iteration for the whole batch, one
// workgroup per sample, no synchronisation, no allocation, no read-back.  Reference: adversarial/attack.py:72 (foolbox 2.x
// LinfinityBasicIterativeAttack / L2BasicIterativeAttack, binary_search=False, no random start, untargeted).
//
//   k_attack_step   x <- clip(x0 + project(x + stepsize * direction(g) - x0), lo, hi);  xn <- (x - mean) / std
//       Linf: direction = sign(g) s,                  project = clip(., -eps s, eps s)
//       L2:   direction = g / max(1e-12, rms(g)) s,   project = . * min(1, eps s / max(1e-12, rms(.)))        (s = hi - lo)
//     g is the gradient with respect to the NORMALISED input; the chain rule through (x - mean) / std divides it by std.
//     The Linf arithmetic is written with the explicitly rounded intrinsics (no contraction into fused multiply-adds): every
//     operation is the one a fp32 tensor program performs, so the result agrees with it bit for bit.
//   k_attack_judge  arg-max of the logits (first index on ties), and the book-keeping of the attack: original class, adversarial
//     class, iteration, distance (foolbox's MeanSquaredDistance / Linfinity: mean((x - x0)^2) / s^2, max |x - x0| / s).
//
// Both reductions of a sample stay inside its workgroup: per-thread partial in a fixed element order, wave shuffle, four wave
// partials through LDS summed in wave order -- no atomics, the same bits on every run.  Sums of squares accumulate in fp64.
#include "attack.h"

namespace node {

namespace {

constexpr int NW = ATTACK_THREADS / 64;

__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int t = threadIdx.x;
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) s += red[w];
  __syncthreads();
  return s;
}

__device__ __forceinline__ float block_max(float v, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
  const int t = threadIdx.x;
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) s = fmaxf(s, red[w]);
  __syncthreads();
  return s;
}

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

__global__ __launch_bounds__(ATTACK_THREADS) void k_attack_step(const AttackStepArgs a) {
  __shared__ double red[NW];
  const int n = blockIdx.x, t = threadIdx.x;
  if (a.active[n] == 0) return;              // (the whole workgroup: an inactive sample keeps its bits)
  const int D = a.c * a.hw;
  const size_t base = (size_t)n * D;
  const float* g = a.g + base;
  const float* x0 = a.x0 + base;
  float* x = a.x + base;
  float* xn = a.xn + base;
  if (!a.l2) {
    for (int i = t; i < D; i += ATTACK_THREADS) {
      const int ch = i / a.hw;
      const float sd = a.std ? a.std[ch] : 1.f, mu = a.mean ? a.mean[ch] : 0.f;
      const float gx = a.std ? __fdiv_rn(g[i], sd) : g[i];
      const float sg = gx > 0.f ? 1.f : (gx < 0.f ? -1.f : 0.f);
      const float x1 = __fadd_rn(x[i], __fmul_rn(a.stepsize, __fmul_rn(sg, a.s)));
      const float p = clampf(__fsub_rn(x1, x0[i]), -a.eps_s, a.eps_s);
      const float v = clampf(__fadd_rn(x0[i], p), a.lo, a.hi);
      x[i] = v;
      xn[i] = __fdiv_rn(__fsub_rn(v, mu), sd);
    }
    return;
  }
  double acc = 0.0;
  for (int i = t; i < D; i += ATTACK_THREADS) {
    const float gx = a.std ? g[i] / a.std[i / a.hw] : g[i];
    acc += (double)gx * (double)gx;
  }
  const float rms_g = (float)sqrt(block_sum(acc, red) / (double)D);
  const float f = a.s / fmaxf(1e-12f, rms_g);
  acc = 0.0;
  for (int i = t; i < D; i += ATTACK_THREADS) {
    const float gx = a.std ? g[i] / a.std[i / a.hw] : g[i];
    const float df = __fsub_rn(__fadd_rn(x[i], __fmul_rn(a.stepsize, __fmul_rn(gx, f))), x0[i]);
    acc += (double)df * (double)df;
  }
  const float rms_p = (float)sqrt(block_sum(acc, red) / (double)D);
  const float sc = fminf(1.f, a.eps_s / fmaxf(1e-12f, rms_p));
  for (int i = t; i < D; i += ATTACK_THREADS) {
    const int ch = i / a.hw;
    const float sd = a.std ? a.std[ch] : 1.f, mu = a.mean ? a.mean[ch] : 0.f;
    const float gx = a.std ? g[i] / sd : g[i];
    const float df = __fsub_rn(__fadd_rn(x[i], __fmul_rn(a.stepsize, __fmul_rn(gx, f))), x0[i]);      // the second pass's value, bit for bit
    const float v = clampf(__fadd_rn(x0[i], __fmul_rn(df, sc)), a.lo, a.hi);
    x[i] = v;
    xn[i] = __fdiv_rn(__fsub_rn(v, mu), sd);
  }
}

__global__ __launch_bounds__(ATTACK_THREADS) void k_attack_judge(const AttackJudgeArgs a) {
  __shared__ double red[NW];
  __shared__ float redv[NW];
  __shared__ int redi[NW];
  const int n = blockIdx.x, t = threadIdx.x;
  // arg-max, first index on ties: a thread scans its classes in rising order with a strict comparison; pairs merge by
  // (larger value, then smaller index)
  const float* lg = a.logits + (size_t)n * a.classes;
  float bv = 0.f;
  int bi = 0x7fffffff;
  for (int j = t; j < a.classes; j += ATTACK_THREADS) {
    const float v = lg[j];
    if (bi == 0x7fffffff || v > bv) { bv = v; bi = j; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_down(bv, off, 64);
    const int oi = __shfl_down(bi, off, 64);
    if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
  }
  if ((t & 63) == 0) { redv[t >> 6] = bv; redi[t >> 6] = bi; }
  __syncthreads();
  bv = redv[0];
  bi = redi[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    const float ov = redv[w];
    const int oi = redi[w];
    if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
  }
  __syncthreads();                            // (redv is used again by the distance's reduction)
  const int pred = bi;
  const bool wrong = (int64_t)pred != a.labels[n];
  if (a.initial) {
    // a natural error: distance 0, never stepped
    if (t == 0) {
      a.original_class[n] = pred;
      if (wrong) {
        a.adversarial_class[n] = pred;
        a.found_iteration[n] = 0;
        a.distance[n] = 0.f;
        a.active[n] = 0;
      }
    }
    if (wrong && a.best_x) {
      const size_t base = (size_t)n * a.d;
      for (int i = t; i < a.d; i += ATTACK_THREADS) a.best_x[base + i] = a.x[base + i];
    }
    return;
  }
  if (a.active[n] == 0 || !wrong) return;     // (uniform over the workgroup)
  const size_t base = (size_t)n * a.d;
  const float* x = a.x + base;
  const float* x0 = a.x0 + base;
  float dist;
  if (a.l2) {
    double acc = 0.0;
    for (int i = t; i < a.d; i += ATTACK_THREADS) {
      const float df = __fsub_rn(x[i], x0[i]);
      acc += (double)df * (double)df;
    }
    dist = (float)(block_sum(acc, red) / (double)a.d / ((double)a.s * (double)a.s));
  } else {
    float m = 0.f;
    for (int i = t; i < a.d; i += ATTACK_THREADS) m = fmaxf(m, fabsf(__fsub_rn(x[i], x0[i])));
    dist = block_max(m, redv) / a.s;
  }
  // every thread holds `dist`; the old record is read before anyone writes it
  const bool better = a.return_early || dist < a.distance[n];
  __syncthreads();
  if (!better) return;
  if (t == 0) {
    a.adversarial_class[n] = pred;
    a.found_iteration[n] = a.iteration;
    a.distance[n] = dist;
    if (a.return_early) a.active[n] = 0;
  }
  if (a.best_x)
    for (int i = t; i < a.d; i += ATTACK_THREADS) a.best_x[base + i] = x[i];
}

}  // namespace

void launch_attack_step(const AttackStepArgs& a, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_attack_step, dim3(n), dim3(ATTACK_THREADS), 0, s, a);
}
void launch_attack_judge(const AttackJudgeArgs& a, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_attack_judge, dim3(n), dim3(ATTACK_THREADS), 0, s, a);
}

}  // namespace node
