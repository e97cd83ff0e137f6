// C ABI of what stands beside the solver: the F(4x4,3x3) diagnostics, GroupNorm + ReLU and the classifier head as
// stand-alone layers, the SGD and Adam steps.
#include "solver.h"     // (g_w4_pair_stats)

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace node;

// The double a caller of a float argument meant: the shortest decimal that rounds to `b` (0.999f -> 0.999, the double
// PyTorch works with).  node_adam_step needs it for 1 - beta: (double)0.999f is 0.99900001287, whose 1 - beta2 is off by
// 1.3e-5 of its value -- and so would exp_avg_sq be, 200 fp32 ulps away from torch.optim.Adam's.
static double shortest_decimal(float b) {
  char text[32];
  for (int digits = 1; digits <= 9; ++digits) {
    snprintf(text, sizeof(text), "%.*g", digits, (double)b);
    const double d = strtod(text, nullptr);
    if ((float)d == b) return d;
  }
  return (double)b;
}

extern "C" {

// Diagnostics: one bias-free 3x3 convolution (pad 1) of an [N, C, 8, 8] tensor through the F(4x4,3x3) pipeline with
// stand-alone transform kernels around the component GEMMs -- what the solver fuses into its GroupNorm passes.
size_t node_conv3x3_w4_workspace_bytes(const node_shape* shape) {
  if (!shape) return 0;
  const size_t numel = (size_t)shape->n * shape->c * shape->h * shape->w;
  const int nv = (shape->n * (shape->h == 16 ? 4 : 1) + 7) & ~7;
  return (2 * numel + 2 * w4_v_elems(nv, shape->c) + w4_u_elems(shape->c)) * sizeof(float) +
         w4_ub_elems(shape->c) * sizeof(unsigned short) + sizeof(W4Scales) + 8 * 256;
}
int node_conv3x3_w4(const node_shape* shape, const float* weight, int dgrad, const float* x, float* y, void* ws,
                    size_t ws_bytes, void* stream) {
  w4_refresh_tuning();     // (the NODE_TUNE_W4_* switches: once per call, not per launch)
  if (!shape || !weight || !x || !y || !ws) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  Dims d;
  TRY(dims_for(shape, &d));
  const bool sq8 = d.H == 8 && d.W == 8, sq16 = d.H == 16 && d.W == 16;
  if (!((sq8 || sq16) && d.C % 64 == 0 && (d.N * (sq16 ? 4 : 1)) % 8 == 0))
    return fail(NODE_ERR_UNSUPPORTED, "the F(4x4,3x3) pipeline takes 8x8 (N %% 8 == 0) or 16x16 (N %% 2 == 0) images, C %% 64 == 0");
  const int Q = sq16 ? 4 : 1, Nv = d.N * Q;
  if (ws_bytes < node_conv3x3_w4_workspace_bytes(shape)) return fail(NODE_ERR_ARG, "workspace too small");
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  Bump b(ws);
  float* xn = b.take<float>(d.numel);
  float* yn = b.take<float>(d.numel);
  float* V = b.take<float>(w4_v_elems(Nv, d.C));
  float* M = b.take<float>(w4_v_elems(Nv, d.C));
  float* U = b.take<float>(w4_u_elems(d.C));
  unsigned short* Ub = b.take<unsigned short>(w4_ub_elems(d.C));
  W4Scales* sc = b.take<W4Scales>(1);
  W4PackJobs jobs;
  memset(&jobs, 0, sizeof(jobs));
  const bool b16 = w4_uses_bf16(Nv, d.C);
  const bool f16 = w4_f16_fits(Nv, d.C);     // fp16-pair operands (k_w4_gemm64h): the scales from max|w| and max|x|
  if (f16) {
    (void)hipMemsetAsync(sc, 0, sizeof(W4Scales), st);
    W4ScaleJobs sj;
    memset(&sj, 0, sizeof(sj));
    sj.w[0] = weight; sj.wn = (size_t)d.C * (d.C + 1) * 9; sj.gb[1] = x; sj.vn[0] = d.numel; sj.C = d.C; sj.gn_m = 1; sj.sc = sc;
    launch_w4_scales(sj, st);
  }
  jobs.w[0] = weight; jobs.u[0] = U; jobs.ub[0] = (b16 && !f16) ? Ub : nullptr; jobs.dgrad[0] = dgrad ? 1 : 0;
  if (f16) { jobs.uh[0] = reinterpret_cast<unsigned*>(U); jobs.uh_exp[0] = &sc->e[W4_E_U1]; }
  launch_w4_pack(jobs, 1, d.C, st);
  launch_w4s_from_nchw(x, xn, d.N, d.C, Q, st);
  launch_w4_input(xn, V, d.N, d.C, Q, Nv, st, f16 ? &sc->e[W4_E_V1] : nullptr);
  if (f16) launch_w4_gemm_f16(reinterpret_cast<const unsigned*>(V), reinterpret_cast<const unsigned*>(U), M, nullptr, Nv, d.C, &sc->e[W4_E_V1], &sc->e[W4_E_U1], st);
  else launch_w4_gemm(V, U, M, nullptr, Nv, d.C, st, b16 ? Ub : nullptr);
  launch_w4_output(M, yn, d.N, d.C, Q, st);
  launch_w4s_to_nchw(yn, y, d.N, d.C, Q, st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch failed: %s", hipGetErrorString(e));
  return NODE_OK;
}

// Diagnostics: the state-layout launches of an F(4x4,3x3) solve on the caller's tensors, and the border maps of its set-up launch.
static int w4s_diag_geom(const node_shape* shape, int* Q) {
  if (!shape) return fail(NODE_ERR_NULL, "shape is NULL");
  const bool sq8 = shape->h == 8 && shape->w == 8, sq16 = shape->h == 16 && shape->w == 16;
  if (!(sq8 || sq16) || shape->n < 1 || shape->c < 16 || shape->c % 16 != 0)
    return fail(NODE_ERR_UNSUPPORTED, "the state layout of the F(4x4,3x3) passes takes 8x8 or 16x16 images, C %% 16 == 0");
  *Q = sq16 ? 4 : 1;
  return NODE_OK;
}
int node_w4s_layout(const node_shape* shape, const float* src, float* dst, int to_nchw, void* stream) {
  int Q = 1;
  TRY(w4s_diag_geom(shape, &Q));
  if (!src || !dst) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if (to_nchw) launch_w4s_to_nchw(src, dst, shape->n, shape->c, Q, (hipStream_t)stream);
  else launch_w4s_from_nchw(src, dst, shape->n, shape->c, Q, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch failed: %s", hipGetErrorString(e));
  return NODE_OK;
}
int node_w4s_layout_jobs(const node_shape* shape, int njobs, const float* const* src, float* const* dst, float* const* copies,
                         void* stream) {
  int Q = 1;
  TRY(w4s_diag_geom(shape, &Q));
  if (njobs < 1 || njobs > 2) return fail(NODE_ERR_ARG, "one or two jobs");
  if (!src || !dst || !copies) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  W4sLayoutJobs lj;
  memset(&lj, 0, sizeof(lj));
  lj.njobs = njobs;
  for (int i = 0; i < njobs; ++i) {
    if (!src[i] || !dst[i]) return fail(NODE_ERR_NULL, "src / dst of a job is NULL");
    lj.src[i] = src[i]; lj.dst[i] = dst[i]; lj.copy[i][0] = copies[2 * i]; lj.copy[i][1] = copies[2 * i + 1];
  }
  launch_w4s_from_nchw_jobs(lj, shape->n, shape->c, Q, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch failed: %s", hipGetErrorString(e));
  return NODE_OK;
}
int node_w4s_tmaps(const node_shape* shape, const float* conv1_w, const float* conv2_w, float* tmap, float* tmap_s, void* stream) {
  int Q = 1;
  TRY(w4s_diag_geom(shape, &Q));
  if (!conv1_w || !conv2_w || !tmap || !tmap_s) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  Dims d;
  memset(&d, 0, sizeof(d));
  d.N = shape->n; d.C = shape->c; d.H = shape->h; d.W = shape->w; d.HW = shape->h * shape->w;     // (all launch_time_prep reads)
  const size_t m = (size_t)d.HW * d.C;
  launch_time_prep(d, conv1_w, conv2_w, tmap, tmap + m, nullptr, nullptr, nullptr, nullptr, 0, (hipStream_t)stream, tmap_s, tmap_s + m, Q);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch failed: %s", hipGetErrorString(e));
  return NODE_OK;
}

int node_w4_pair_stats(int32_t* out4) {
  if (!out4) return fail(NODE_ERR_NULL, "out4 is NULL");
  for (int i = 0; i < 4; ++i) out4[i] = g_w4_pair_stats[i];
  return NODE_OK;
}

// Diagnostics: the exact three-way bf16 split the component GEMMs apply to their fp32 row operands (k_w4_gemm64b and its
// siblings), element by element: out[3 i + p] = part p of x[i] as a float.
int node_w4_split3(const float* x, float* out, size_t n, void* stream) {
  if (!x || !out) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if (n == 0 || n % 8 != 0) return fail(NODE_ERR_ARG, "n must be a positive multiple of 8");
  launch_w4_split_check(x, out, n, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch failed: %s", hipGetErrorString(e));
  return NODE_OK;
}

int node_gn_relu_fwd(const node_shape* shape, const float* z, const float* gamma, const float* beta, int relu, float* out,
                     float* stats, void* stream) {
  char why[200];
  const int rc = head_check(shape, why, sizeof(why));
  if (rc != NODE_OK && rc != NODE_ERR_UNSUPPORTED) return fail(rc, "%s", why);   // (the per-group kernels take any C)
  if (!z || !gamma || !beta || !out || !stats) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  launch_gn_relu_fwd(*shape, z, gamma, beta, relu, out, stats, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch of node_gn_relu_fwd failed: %s", hipGetErrorString(e));
  return NODE_OK;
}

int node_gn_relu_bwd(const node_shape* shape, const float* z, const float* gamma, const float* beta, const float* stats,
                     int relu, const float* g_out, float* dz, float* gpart, float* gsum, void* stream) {
  char why[200];
  const int rc = head_check(shape, why, sizeof(why));
  if (rc != NODE_OK && rc != NODE_ERR_UNSUPPORTED) return fail(rc, "%s", why);
  if (!z || !gamma || !beta || !stats || !g_out || !dz || !gpart) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  launch_gn_relu_bwd(*shape, z, gamma, beta, stats, relu, g_out, dz, gpart, (hipStream_t)stream);
  if (gsum != nullptr) launch_head_gsum(gpart, gsum, shape->n, shape->c, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch of node_gn_relu_bwd failed: %s", hipGetErrorString(e));
  return NODE_OK;
}

int node_head_fwd(const node_shape* shape, const float* z, const float* gamma, const float* beta, const float* scale,
                  float* pooled, float* stats, void* stream) {
  char why[200];
  const int rc = head_check(shape, why, sizeof(why));
  if (rc != NODE_OK) return fail(rc, "%s", why);
  if (!z || !gamma || !beta || !pooled || !stats) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  launch_head_fwd(*shape, z, gamma, beta, scale, pooled, stats, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch of node_head_fwd failed: %s", hipGetErrorString(e));
  return NODE_OK;
}

int node_gn_relu_distance(const node_shape* shape, const float* a, const float* b, const float* gamma, const float* beta, float* out,
                          void* stream) {
  char why[200];
  const int rc = head_check(shape, why, sizeof(why));
  if (rc != NODE_OK) return fail(rc, "%s", why);
  if (!a || !b || !gamma || !beta || !out) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if ((((uintptr_t)a) | ((uintptr_t)b)) & 15) return fail(NODE_ERR_ARG, "a and b must be 16-byte aligned");
  launch_gn_relu_distance(*shape, a, b, gamma, beta, out, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch of node_gn_relu_distance failed: %s", hipGetErrorString(e));
  return NODE_OK;
}

int node_head_bwd(const node_shape* shape, const float* z, const float* gamma, const float* beta, const float* scale,
                  const float* stats, const float* g_pooled, float* dz, float* gpart, float* gsum, void* stream) {
  char why[200];
  const int rc = head_check(shape, why, sizeof(why));
  if (rc != NODE_OK) return fail(rc, "%s", why);
  if (!z || !gamma || !beta || !stats || !g_pooled || !dz || !gpart) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  launch_head_bwd(*shape, z, gamma, beta, scale, stats, g_pooled, dz, gpart, (hipStream_t)stream);
  if (gsum != nullptr) launch_head_gsum(gpart, gsum, shape->n, shape->c, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch of node_head_bwd failed: %s", hipGetErrorString(e));
  return NODE_OK;
}

int node_sgd_step(const node_sgd_tensor* tensors, int count, float lr, float momentum, float weight_decay, float grad_scale,
                  const float* skip_if_nonzero, void* stream) {
  if (count < 0) return fail(NODE_ERR_ARG, "count < 0");
  if (count == 0) return NODE_OK;
  if (!tensors) return fail(NODE_ERR_NULL, "tensors is NULL");
  if (!(lr >= 0.f) || !(momentum >= 0.f) || !(weight_decay >= 0.f)) return fail(NODE_ERR_ARG, "lr / momentum / weight_decay must be >= 0");
  for (int i = 0; i < count; ++i) {
    if (!tensors[i].param || !tensors[i].grad) return fail(NODE_ERR_NULL, "tensor %d: a pointer is NULL", i);
    if (!tensors[i].momentum_buf && momentum != 0.f) return fail(NODE_ERR_NULL, "tensor %d: momentum buffer is NULL with momentum %g", i, momentum);
    if ((((uintptr_t)tensors[i].param) | ((uintptr_t)tensors[i].grad) | ((uintptr_t)tensors[i].momentum_buf)) & 3)
      return fail(NODE_ERR_ARG, "tensor %d: pointers must be 4-byte aligned", i);
  }
  for (int base = 0; base < count; base += SGD_TABLE) {
    SgdTable tb;
    memset(&tb, 0, sizeof(tb));
    const int m = count - base < SGD_TABLE ? count - base : SGD_TABLE;
    size_t max_n = 0;
    for (int i = 0; i < m; ++i) {
      tb.e[i].p = tensors[base + i].param; tb.e[i].g = tensors[base + i].grad; tb.e[i].m = tensors[base + i].momentum_buf;
      tb.e[i].n = tensors[base + i].n;
      if (tb.e[i].n > max_n) max_n = tb.e[i].n;
    }
    launch_sgd_multi(tb, m, max_n, lr, momentum, weight_decay, grad_scale, skip_if_nonzero, (hipStream_t)stream);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch of node_sgd_step failed: %s", hipGetErrorString(e));
  return NODE_OK;
}

int node_adam_step(const node_adam_tensor* tensors, int count, float lr, float beta1, float beta2, float eps, float weight_decay,
                   float grad_scale, const float* skip_if_nonzero, void* stream) {
  if (count < 0) return fail(NODE_ERR_ARG, "count < 0");
  if (count == 0) return NODE_OK;
  if (!tensors) return fail(NODE_ERR_NULL, "tensors is NULL");
  if (!(lr >= 0.f) || !(eps >= 0.f) || !(weight_decay >= 0.f)) return fail(NODE_ERR_ARG, "lr / eps / weight_decay must be >= 0");
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return fail(NODE_ERR_ARG, "beta1 / beta2 must lie in [0, 1)");
  for (int i = 0; i < count; ++i) {
    const node_adam_tensor& t = tensors[i];
    if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq || !t.step) return fail(NODE_ERR_NULL, "tensor %d: a pointer is NULL", i);
    if ((((uintptr_t)t.param) | ((uintptr_t)t.grad) | ((uintptr_t)t.exp_avg) | ((uintptr_t)t.exp_avg_sq) | ((uintptr_t)t.step)) & 3)
      return fail(NODE_ERR_ARG, "tensor %d: pointers must be 4-byte aligned", i);
  }
  const double b1 = shortest_decimal(beta1), b2 = shortest_decimal(beta2);
  for (int base = 0; base < count; base += ADAM_TABLE) {
    AdamTable tb;
    memset(&tb, 0, sizeof(tb));
    const int m = count - base < ADAM_TABLE ? count - base : ADAM_TABLE;
    size_t max_n = 0;
    for (int i = 0; i < m; ++i) {
      const node_adam_tensor& t = tensors[base + i];
      tb.e[i].p = t.param; tb.e[i].g = t.grad; tb.e[i].m = t.exp_avg; tb.e[i].v = t.exp_avg_sq; tb.e[i].step = t.step;
      tb.e[i].n = t.n;
      if (t.n > max_n) max_n = t.n;
    }
    launch_adam_multi(tb, m, max_n, lr, b1, b2, eps, weight_decay, grad_scale, skip_if_nonzero, (hipStream_t)stream);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch of node_adam_step failed: %s", hipGetErrorString(e));
  return NODE_OK;
}

}  // extern "C"
