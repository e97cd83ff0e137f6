// Step control of the integrator, all of it on the device: the wavefront-reduced error norm, the step controller (accept / dt / t
// never leave the GPU except for one 64-byte read-back per step), Hairer's initial step, the FSAL commit, the quartic dense-output
// interpolant, the fixed-grid end-of-step combine, the setters of `Ctrl` and the record a deferred solve leaves behind.
// tests/test_gpu_step_control.py drives each of them on its own.
//
// Algorithm follows the restated torchdiffeq spec; the CPU
// statement of the same arithmetic is oracle/torchdiffeq_restated.py.
#include "pointwise_common.h"
#include "wino4.h"
#include "step_control.h"
#include <cstring>
#include "../../include/node_hip.h"

namespace node {

// (Dormand-Prince / Shampine coefficients c_CSOL / c_CERR, the step controller's and the initial step's decisions: step_control.h)

// ============================================================================
// Error norm:  sum_i (err_i / (atol + rtol*max(|y0_i|,|y1_i|)))^2,
//   err = dt * sum_j c_err_j k_j    -- wave-reduced, one partial per workgroup
// For segments whose intermediate stages are never consumed (adj_params) the same
// pass also forms y1 = y0 + dt * sum_j b_j k_j.
// ============================================================================
// One launch for up to three state segments (grid.y = segment): the augmented state's y, a and theta segments used to
// be three launches per step.
struct ErrSegs { ErrSeg seg[3]; float* partial[3]; };
__device__ void error_norm_body(const ErrSeg& seg, const Ctrl* ctrl, float rtol, float atol, float* partial);
__global__ __launch_bounds__(256) void k_error_norm(ErrSegs a, const Ctrl* ctrl, float rtol, float atol) {
  if (ctrl->done) return;
  error_norm_body(a.seg[blockIdx.y], ctrl, rtol, atol, a.partial[blockIdx.y]);
}
__device__ void error_norm_body(const ErrSeg& seg, const Ctrl* ctrl, float rtol, float atol, float* partial) {
  __shared__ float red[4];
  const float dtf = (float)ctrl->dt;
  float ce[7], cb[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) { ce[j] = dtf * c_CERR[j]; cb[j] = dtf * c_CSOL[j]; }
  float acc = 0.f;
  const size_t n4 = seg.n >> 2;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < n4; v += stride) {
    const size_t off = v * 4;
    float4 kv[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) kv[j] = (j == 1) ? make_float4(0, 0, 0, 0) : ld4(seg.k[j] + off);
    const float4 y0 = ld4(seg.y0 + off);
    float4 y1;
    if (seg.compute_y1) {
      float4 s;
      s.x = cb[0] * kv[0].x; s.y = cb[0] * kv[0].y; s.z = cb[0] * kv[0].z; s.w = cb[0] * kv[0].w;
#pragma unroll
      for (int j = 2; j < 6; ++j) { s.x += cb[j] * kv[j].x; s.y += cb[j] * kv[j].y; s.z += cb[j] * kv[j].z; s.w += cb[j] * kv[j].w; }
      y1 = make_float4(y0.x + s.x, y0.y + s.y, y0.z + s.z, y0.w + s.w);
      st4(seg.y1 + off, y1);
    } else {
      y1 = ld4(seg.y1 + off);
    }
    float4 e;
    e.x = ce[0] * kv[0].x; e.y = ce[0] * kv[0].y; e.z = ce[0] * kv[0].z; e.w = ce[0] * kv[0].w;
#pragma unroll
    for (int j = 2; j < 7; ++j) { e.x += ce[j] * kv[j].x; e.y += ce[j] * kv[j].y; e.z += ce[j] * kv[j].z; e.w += ce[j] * kv[j].w; }
    float r;
    r = e.x / (atol + rtol * fmaxf(fabsf(y0.x), fabsf(y1.x))); acc += r * r;
    r = e.y / (atol + rtol * fmaxf(fabsf(y0.y), fabsf(y1.y))); acc += r * r;
    r = e.z / (atol + rtol * fmaxf(fabsf(y0.z), fabsf(y1.z))); acc += r * r;
    r = e.w / (atol + rtol * fmaxf(fabsf(y0.w), fabsf(y1.w))); acc += r * r;
    // upstream asserts the state is finite at every step ('non-finite values in state `y`'); fmaxf above drops a
    // NaN operand and ReLU turns a NaN pre-activation into 0, so an infinite / NaN state would otherwise pass
    // unnoticed: 0 * (inf or NaN) = NaN poisons the sum, and the controller reports NODE_ERR_NONFINITE
    acc += 0.f * (((y0.x + y0.y) + (y0.z + y0.w)) + ((y1.x + y1.y) + (y1.z + y1.w)));
  }
  // scalar tail (n % 4), handled by block 0
  if (blockIdx.x == 0) {
    for (size_t i = (n4 << 2) + threadIdx.x; i < seg.n; i += 256) {
      float kk[7];
#pragma unroll
      for (int j = 0; j < 7; ++j) kk[j] = (j == 1) ? 0.f : seg.k[j][i];
      const float y0 = seg.y0[i];
      float y1;
      if (seg.compute_y1) {
        float s = cb[0] * kk[0];
#pragma unroll
        for (int j = 2; j < 6; ++j) s += cb[j] * kk[j];
        y1 = y0 + s;
        seg.y1[i] = y1;
      } else {
        y1 = seg.y1[i];
      }
      float e = ce[0] * kk[0];
#pragma unroll
      for (int j = 2; j < 7; ++j) e += ce[j] * kk[j];
      const float r = e / (atol + rtol * fmaxf(fabsf(y0), fabsf(y1)));
      acc += r * r;
      acc += 0.f * (y0 + y1);
    }
  }
  const float tot = block_sum_256(acc, red);
  // (an agent-scope, write-through store where a plain one would do: k_step_controller reads the partials in a LATER launch.  Kept as it
  //  was when a one-launch variant, measured and not kept, read them inside the same launch: the live kernel's code is unchanged)
  if (threadIdx.x == 0) __hip_atomic_store(&partial[blockIdx.x], tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

void launch_error_norm(const ErrSeg* segs, float* const* partial, int nseg, const Ctrl* ctrl, float rtol, float atol, hipStream_t s) {
  ErrSegs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < nseg; ++i) { a.seg[i] = segs[i]; a.partial[i] = partial[i]; }
  hipLaunchKernelGGL(k_error_norm, dim3(ERR_BLOCKS, nseg), dim3(256), 0, s, a, ctrl, rtol, atol);
}

// ============================================================================
// Step controller (one workgroup).  Mirrors `_adaptive_dopri5_step` /
// `_optimal_step_size` of the restated solver: accept iff every segment's mean
// squared error ratio <= 1; dt <- dt / clamp(sqrt(max ratio)^(1/5)/0.9, 0.1, 1/dfactor).
// t / dt are float64 like upstream's adaptive solvers.
// ============================================================================
__device__ inline void step_controller_body(const StepCtlArgs& a, float* red, float* ratios) {
  for (int sgi = 0; sgi < a.nseg; ++sgi) {
    if (a.gbuf != nullptr) {      // global-norm mode: the sums of all ranks (k_norm_pack + the caller's all-reduce)
      if (threadIdx.x == 0) ratios[sgi] = (float)((double)a.gbuf[sgi] / (a.numel[sgi] * (double)a.gworld));
      continue;
    }
    const float tot = reduce_partials_512(a.partial[sgi], red);
    if (threadIdx.x == 0) ratios[sgi] = (float)((double)tot / a.numel[sgi]);
    __syncthreads();
  }
  bool w4_ovf = false;
  if (a.w4sc != nullptr) w4_ovf = w4_gscale_update(a.w4sc, threadIdx.x, red);   // (all 256 threads)
  if (a.gbuf != nullptr && a.gbuf[4] > 0.f) w4_ovf = true;                      // (some rank's cotangent left its scale: all repeat)
  if (threadIdx.x != 0) return;
  if (a.w4sc != nullptr) {
    // fp16-pair operands (wino4.h): the next step's cotangent scale from this step's recorded maximum (above); a step in which a pass
    // met a value beyond its scale's range is REPEATED at the new scale -- nothing accepted, t and dt as they were, not a solver step
    W4Scales* sc = a.w4sc;
    if (w4_ovf && sc->pad[0] < 8u) {
      sc->pad[0] += 1u;                    // (consecutive repeats: bounded)
      Ctrl* c = a.ctrl;
      c->accept = 0;
      c->t_prev = c->t;
      c->dt_used = c->dt;
      c->j0 = c->j1 = c->j;
      return;
    }
    sc->pad[0] = 0u;
  }
  step_controller_decide(a, ratios);
}
__global__ __launch_bounds__(256) void k_step_controller(StepCtlArgs a) {
  __shared__ float red[4];
  __shared__ float ratios[4];
  if (a.ctrl->done) {   // a step enqueued past the end of the interval: nothing was computed, nothing is emitted
    if (threadIdx.x == 0) a.ctrl->j0 = a.ctrl->j1 = a.ctrl->j;
    return;
  }
  step_controller_body(a, red, ratios);
}

void launch_step_controller(const StepCtlArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_step_controller, dim3(1), dim3(256), 0, s, a);
}

__global__ __launch_bounds__(256) void k_w4_gscale(W4Scales* sc, int skew) {
  __shared__ float red[4];
  (void)w4_gscale_update(sc, threadIdx.x, red);
  if (threadIdx.x == 0 && skew != 0) sc->e[W4_E_G] += skew;
}
void launch_w4_gscale(W4Scales* sc, hipStream_t s, int skew) { hipLaunchKernelGGL(k_w4_gscale, dim3(1), dim3(256), 0, s, sc, skew); }

// ============================================================================
// Hairer initial step (`_select_initial_step`, order argument 4)
//   phase 0: sum (y0/scale)^2, sum (f0/scale)^2      scale = atol + |y0| rtol
//   phase 1: sum ((f1-f0)/scale)^2
// ============================================================================
struct InitSegs { InitSeg seg[3]; float* partial[3]; };
__device__ inline void init_norms_body(const InitSegs& a, float rtol, float atol, int phase, float* red);
__global__ __launch_bounds__(256) void k_init_norms(InitSegs a, float rtol, float atol, int phase) {
  __shared__ float red[4];
  init_norms_body(a, rtol, atol, phase, red);
}
__device__ inline void init_norms_body(const InitSegs& a, float rtol, float atol, int phase, float* red) {
  const InitSeg& seg = a.seg[blockIdx.y];
  float* partial = a.partial[blockIdx.y];
  float a0 = 0.f, a1 = 0.f;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < seg.n; i += stride) {
    const float y = seg.y0[i];
    const float sc = atol + fabsf(y) * rtol;
    if (phase == 0) {
      const float u = y / sc, v = seg.f0[i] / sc;
      a0 += u * u;
      a1 += v * v;
    } else {
      const float u = (seg.f1[i] - seg.f0[i]) / sc;
      a0 += u * u;
    }
  }
  const float t0 = block_sum_256(a0, red);
  const float t1 = block_sum_256(a1, red);
  if (threadIdx.x == 0) {      // (agent-scope stores where plain ones would do, as in error_norm_body: k_init_controller is a later launch)
    __hip_atomic_store(&partial[blockIdx.x * 2], t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&partial[blockIdx.x * 2 + 1], t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
void launch_init_norms(const InitSeg* segs, float* const* partial, int nseg, float rtol, float atol, int phase, hipStream_t s) {
  InitSegs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < nseg; ++i) { a.seg[i] = segs[i]; a.partial[i] = partial[i]; }
  hipLaunchKernelGGL(k_init_norms, dim3(ERR_BLOCKS, nseg), dim3(256), 0, s, a, rtol, atol, phase);
}

// global-norm mode: this rank's sums of the coming decision -> gbuf[8] (see NormPackArgs; the caller's hook adds the ranks')
__global__ __launch_bounds__(256) void k_norm_pack(NormPackArgs a) {
  __shared__ float red[4];
  const Ctrl* c = a.ctrl;
  float out[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int sgi = 0; sgi < a.nseg; ++sgi) {
    const float* p = a.partial[sgi];
    if (a.mode == 0) {
      out[sgi] = reduce_partials_512(p, red);
    } else {
      float v0 = p[threadIdx.x * 2] + p[(threadIdx.x + 256) * 2];
      float v1 = p[threadIdx.x * 2 + 1] + p[(threadIdx.x + 256) * 2 + 1];
      v0 = block_sum_256(v0, red);
      v1 = block_sum_256(v1, red);
      if (a.mode == 1) { out[2 * sgi] = v0; out[2 * sgi + 1] = v1; }
      else out[sgi] = v0;
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if (a.has_scalar) {
    if (a.mode == 0) {        // the scalar segment's squared error ratio, as step_controller_decide forms it
      const float dtf = (float)c->dt;
      float e = (dtf * c_CERR[0]) * c->ts_k[0];
      float s = (dtf * c_CSOL[0]) * c->ts_k[0];
#pragma unroll
      for (int j = 2; j < 7; ++j) { e += (dtf * c_CERR[j]) * c->ts_k[j]; if (j < 6) s += (dtf * c_CSOL[j]) * c->ts_k[j]; }
      const float y1 = c->ts_cur + s;
      const float r = e / (a.atol + a.rtol * fmaxf(fabsf(c->ts_cur), fabsf(y1)));
      out[3] = r * r;
    } else {
      const float sc = a.atol + fabsf(c->ts_cur) * a.rtol;
      if (a.mode == 1) { const float d0 = c->ts_cur / sc, d1 = c->ts_k[0] / sc; out[6] = d0 * d0; out[7] = d1 * d1; }
      else { const float d2 = (c->ts_k[1] - c->ts_k[0]) / sc; out[3] = d2 * d2; }
    }
  }
  if (a.mode == 0 && a.w4sc != nullptr && __hip_atomic_load(&a.w4sc->ovf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) out[4] = 1.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) a.gbuf[i] = out[i];
}
void launch_norm_pack(const NormPackArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_norm_pack, dim3(1), dim3(256), 0, s, a); }

__global__ __launch_bounds__(256) void k_init_controller(InitCtlArgs a) {
  __shared__ float red[4];
  __shared__ float sums[3][2];
  if (a.gbuf != nullptr) {      // global-norm mode: the sums of all ranks; the counts are the ranks' together
    if (threadIdx.x == 0) {
      float gs[3][2];
      InitCtlArgs b = a;
      for (int sgi = 0; sgi < a.nseg; ++sgi) {
        gs[sgi][0] = a.phase == 0 ? a.gbuf[2 * sgi] : a.gbuf[sgi];
        gs[sgi][1] = a.phase == 0 ? a.gbuf[2 * sgi + 1] : 0.f;
        b.numel[sgi] = a.numel[sgi] * (double)a.gworld;
      }
      init_controller_decide(b, gs);
    }
    return;
  }
  for (int sgi = 0; sgi < a.nseg; ++sgi) {
    const float* p = a.partial[sgi];
    float v0 = p[threadIdx.x * 2] + p[(threadIdx.x + 256) * 2];
    float v1 = p[threadIdx.x * 2 + 1] + p[(threadIdx.x + 256) * 2 + 1];
    v0 = block_sum_256(v0, red);
    v1 = block_sum_256(v1, red);
    if (threadIdx.x == 0) { sums[sgi][0] = v0; sums[sgi][1] = v1; }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  init_controller_decide(a, sums);
}
void launch_init_controller(const InitCtlArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_init_controller, dim3(1), dim3(256), 0, s, a);
}

__global__ void k_set_ctrl(Ctrl* c, double t, double dt, int reset) { ctrl_set(c, t, dt, reset); }
void launch_set_ctrl(Ctrl* ctrl, double t, double dt, int reset, hipStream_t s) {
  hipLaunchKernelGGL(k_set_ctrl, dim3(1), dim3(1), 0, s, ctrl, t, dt, reset);
}
// which: 0 ts_cur = v ; 1 rk4 end-of-step: ts_cur += dt*(k0+3k1+3k2+k3)/8 ; 2 ts_k[0] = ts_k[6]
__global__ void k_set_scalar_state(Ctrl* c, float v, int which) {
  if (which == 0) c->ts_cur = v;
  else if (which == 1) {
    const float dtf = (float)c->dt;
    c->ts_cur = c->ts_cur + (c->ts_k[0] + 3.f * c->ts_k[1] + 3.f * c->ts_k[2] + c->ts_k[3]) * (dtf * 0.125f);
  } else if (which == 2) c->ts_k[0] = c->ts_k[6];
}
void launch_set_scalar_state(Ctrl* ctrl, float v, int which, hipStream_t s) {
  hipLaunchKernelGGL(k_set_scalar_state, dim3(1), dim3(1), 0, s, ctrl, v, which);
}

// ============================================================================
// Dense output: quartic through (y0, y1, y_mid, f0, f1) of the last accepted step
//   (`_interp_fit_dopri5` + `_interp_evaluate`, power form like upstream)
// ============================================================================
// ----------------------------------------------------------------------------
// Device-resident stepping: what the host used to do between two steps after reading `Ctrl` back.
// ----------------------------------------------------------------------------
// Dense output of the forward solve for the targets [j0, j1) the finished step passed, written straight into the
// caller's NCHW trajectory: workgroup = (64 channels x 64 pixels of one sample) through an LDS tile, reads
// coalesced along the channels (NHWC state), writes coalesced along the pixels.
__global__ __launch_bounds__(256) void k_emit_outputs(EmitArgs a, Dims d) {
  const Ctrl* c = a.ctrl;
  const int j0 = c->j0, j1 = c->j1;
  if (j1 <= j0) return;
  __shared__ float tile[64][65];
  const int n = blockIdx.z, c0 = blockIdx.x * 64, p0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // 64 x 4
  const float dt = (float)c->dt_used;
  const float t0f = (float)c->t_prev, t1f = (float)c->t;
  const size_t sample = (size_t)n * d.HW * d.C;
  for (int j = j0; j < j1; ++j) {
    const float x = ((float)a.targets[j] - t0f) / (t1f - t0f);   // upstream rounds t0, t1, t to the state dtype first
    for (int i = ty; i < 64; i += 4) {
      const int p = p0 + i, ch = c0 + tx;
      if (p < d.HW && ch < d.C) {
        const size_t idx = sample + (size_t)p * d.C + ch;
        float kk[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) kk[q] = (q == 1) ? 0.f : a.k[q][idx];
        tile[i][tx] = interp_one(a.y0[idx], a.y1[idx], kk, dt, x);
      }
    }
    __syncthreads();
    float* out = a.y_out + (size_t)j * d.N * d.C * d.HW + sample;
    for (int i = ty; i < 64; i += 4) {
      const int ch = c0 + i, p = p0 + tx;
      if (p < d.HW && ch < d.C) out[(size_t)ch * d.HW + p] = tile[tx][i];
    }
    __syncthreads();
  }
}
void launch_emit_outputs(const Dims& d, const EmitArgs& a, hipStream_t s) {
  dim3 grid((d.C + 63) / 64, (d.HW + 63) / 64, d.N);
  hipLaunchKernelGGL(k_emit_outputs, grid, dim3(256), 0, s, a, d);
}

// The same for a FLAT state (the generic solver, node_flat_*: dynamics evaluated by the caller, no layout): out[j][i]
__global__ __launch_bounds__(256) void k_emit_flat(EmitArgs a, size_t n) {
  const Ctrl* c = a.ctrl;
  const int j0 = c->j0, j1 = c->j1;
  if (j1 <= j0) return;
  const float dt = (float)c->dt_used;
  const float t0f = (float)c->t_prev, t1f = (float)c->t;
  const size_t stride = (size_t)gridDim.x * 256;
  for (int j = j0; j < j1; ++j) {
    const float x = ((float)a.targets[j] - t0f) / (t1f - t0f);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
      float kk[7];
#pragma unroll
      for (int q = 0; q < 7; ++q) kk[q] = (q == 1) ? 0.f : a.k[q][i];
      a.y_out[(size_t)j * n + i] = interp_one(a.y0[i], a.y1[i], kk, dt, x);
    }
  }
}
void launch_emit_flat(const EmitArgs& a, size_t n, hipStream_t s) {
  size_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_emit_flat, dim3((unsigned)blocks), dim3(256), 0, s, a, n);
}
// the time an evaluation of the caller's dynamics happens at, as a device float (the caller hands it to its function)
__global__ void k_flat_time(EvalTime et, float* out) { *out = eval_time(et); }
void launch_flat_time(const EvalTime& et, float* out, hipStream_t s) { hipLaunchKernelGGL(k_flat_time, dim3(1), dim3(1), 0, s, et, out); }
// the scalar segment of a flat state lives in the controller: which = -1 its value, 0..6 its stage derivatives
__global__ void k_flat_scalar(Ctrl* c, int which, const float* src, float scale, int accumulate) {
  const float v = scale * src[0];
  if (which < 0) c->ts_cur = (accumulate ? c->ts_cur : 0.f) + v;
  else c->ts_k[which] = (accumulate ? c->ts_k[which] : 0.f) + v;
}
void launch_flat_scalar(Ctrl* ctrl, int which, const float* src, float scale, int accumulate, hipStream_t s) {
  hipLaunchKernelGGL(k_flat_scalar, dim3(1), dim3(1), 0, s, ctrl, which, src, scale, accumulate);
}

// Accepted step, interval not finished: y <- y1, k0 <- k6 (FSAL) for every tensor segment.  Augmented solve at the
// end of its interval: every segment <- dense output at the interval's end time, in place (element-wise).
__device__ inline void export_record(const Ctrl* c, node_step_record* r, float* miss_flag, int expect);
__global__ __launch_bounds__(256) void k_commit(CommitArgs a) {
  const Ctrl* c = a.ctrl;
  if (a.rec != nullptr && blockIdx.x == 0 && threadIdx.x == 0) export_record(c, a.rec, a.miss_flag, a.expect_steps);
  if (!c->accept || c->step_idx == 0) return;
  const bool fin = c->done != 0;
  if (fin && !(a.interp_final && c->j1 > c->j0 && c->status == 0)) return;
  // (a step enqueued past the end: the controller left j0 == j1, so nothing happens here either)
  const size_t stride = (size_t)gridDim.x * 256, start = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (!fin) {
    for (int sg = 0; sg < a.nseg; ++sg) {
      const size_t n4 = a.n[sg] >> 2;
      float4* y = reinterpret_cast<float4*>(a.y[sg]);
      const float4* y1 = reinterpret_cast<const float4*>(a.y1[sg]);
      float4* k0 = reinterpret_cast<float4*>(a.k0[sg]);
      const float4* k6 = reinterpret_cast<const float4*>(a.k6[sg]);
      for (size_t i = start; i < n4; i += stride) { y[i] = y1[i]; k0[i] = k6[i]; }
      for (size_t i = (n4 << 2) + start; i < a.n[sg]; i += stride) { a.y[sg][i] = a.y1[sg][i]; a.k0[sg][i] = a.k6[sg][i]; }
    }
    return;
  }
  const float dt = (float)c->dt_used;
  const float t0f = (float)c->t_prev, t1f = (float)c->t;
  const float x = ((float)a.targets[0] - t0f) / (t1f - t0f);
  for (int sg = 0; sg < a.nseg; ++sg)
    for (size_t i = start; i < a.n[sg]; i += stride) {
      float kk[7];
#pragma unroll
      for (int q = 0; q < 7; ++q) kk[q] = (q == 1) ? 0.f : a.k[sg][q][i];
      a.y[sg][i] = interp_one(a.y[sg][i], a.y1[sg][i], kk, dt, x);
    }
}
void launch_commit(const CommitArgs& a, hipStream_t s) {
  size_t nmax = 0;
  for (int i = 0; i < a.nseg; ++i) nmax = a.n[i] > nmax ? a.n[i] : nmax;
  size_t blocks = (nmax / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_commit, dim3((unsigned)blocks), dim3(256), 0, s, a);
}

__global__ void k_set_target(double* targets, double t_end) { targets[0] = t_end; }
void launch_set_target(double* targets, double t_end, hipStream_t s) {
  hipLaunchKernelGGL(k_set_target, dim3(1), dim3(1), 0, s, targets, t_end);
}
// Deferred completion: what the host would have read back, left in the caller's device record; a miss (the steps
// enqueued did not finish the interval, or it stopped with a status) also bumps the caller's flag, on which the
// optimizer step is predicated.
__device__ inline void export_record(const Ctrl* c, node_step_record* r, float* miss_flag, int expect) {
  const int miss = !(c->done && c->status == 0 && c->step_idx <= expect);   // (steps past the end did nothing)
  r->done = c->done; r->status = c->status; r->steps = c->step_idx; r->accepted = c->n_acc; r->rejected = c->n_rej;
  r->miss = miss; r->t = c->t; r->dt = c->dt; r->first_dt = c->first_dt; r->t_prev = c->t_prev; r->dt_used = c->dt_used;
  if (miss && miss_flag != nullptr) *miss_flag += 1.f;
}
__global__ void k_export_record(const Ctrl* c, node_step_record* r, float* miss_flag, int expect) { export_record(c, r, miss_flag, expect); }
void launch_export_record(const Ctrl* ctrl, node_step_record* rec, float* miss_flag, int expect_steps, hipStream_t s) {
  hipLaunchKernelGGL(k_export_record, dim3(1), dim3(1), 0, s, ctrl, rec, miss_flag, expect_steps);
}
__global__ void k_set_interval(Ctrl* c, double t, double dt) { ctrl_set_interval(c, t, dt); }
void launch_set_interval(Ctrl* ctrl, double t, double dt, hipStream_t s) {
  hipLaunchKernelGGL(k_set_interval, dim3(1), dim3(1), 0, s, ctrl, t, dt);
}

// out = y + scale * sum_j coef_j k_j   (flat; fixed-grid solver's end-of-step update)
__global__ __launch_bounds__(256) void k_lincomb(Comb c, const Ctrl* ctrl, float* out, size_t n) {
  const float scale = comb_scale(c, ctrl);
  float cf[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) cf[j] = scale * c.coef[j];
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float s = 0.f;
    for (int j = 0; j < c.nk; ++j) s += cf[j] * c.k[j][i];
    out[i] = c.y[i] + s;
  }
}
void launch_lincomb(const Comb& c, const Ctrl* ctrl, float* out, size_t n, hipStream_t s) {
  size_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_lincomb, dim3((unsigned)blocks), dim3(256), 0, s, c, ctrl, out, n);
}

}  // namespace node
