// C ABI of the `minimal` stem with norm = 'batch' (include/node_hip.h: node_bnministem_fwd / node_bnministem_bwd) -- model.py:129-145
// (`MinimalConvDownsample`) whose norms are model.py:274 (nn.BatchNorm2d(24, track_running_stats=False)) -- as a host-side plan.
// It is ministem_api.hip's plan with the other norm, as bnconvstem_api.hip is convstem_api.hip's: the BatchNorm passes of
// kernels_bnministem.hip (two-stage statistics, Chan's formula, fp64 backward partials) around the 24-channel convolutions of
// kernels_ministem.hip, used as they are.  NHWC of channel pitch 24 inside the workspace, NCHW at the boundary.
//
// forward (7 launches):   conv0 | stats, apply (norm + ReLU) | conv 4x4/2 | stats, apply | conv 4x4/2 -> NCHW
// backward, last layer first:
//   parameters (5 launches): the last bias gradient | per 4x4 convolution its weight gradient's slabs | conv0's per-sample
//                          weight gradient | ONE launch of sums: three slab sets, two bias partials
//   data chain (6 launches): per 4x4 convolution its data gradient and the BatchNorm backward's two stages (sums, dx in place)
//   image (1 launch):      the transposed first layer
// grads == NULL runs the data chain and the image's launch alone (7 launches); d_x == NULL leaves the image's launch out.
// dgamma / dbeta leave the dx passes directly (their chunk-0 workgroup), so the sums launch carries no norm job.  The biases of
// conv0 and the middle convolution stand in front of a BatchNorm: their gradients are zero identically and are computed the way
// the modules compute them (column sums of the gradient of h: the dx pass leaves them per chunk), rounding noise around zero.
#include "host_common.h"
#include "bnministem.h"
#include "stem_plan.h"
#include <cstring>

using namespace node;

namespace {

inline int down4(int h) { return (h + 2 - 4) / 2 + 1; }     // 4x4 stride 2 pad 1

struct Split { int nsplit, rps; float* slab; };

// split-K of a weight gradient over R rows: ministem_api.hip's rule (about 256 workgroups, whole chunks of 32 rows)
Split make_split(int R, int Cout) {
  const int by = (Cout + MINI_COB - 1) / MINI_COB;
  int target = 256 / by;
  if (target < 1) target = 1;
  int rps = ((R + target - 1) / target + 31) & ~31;
  if (rps < 32) rps = 32;
  Split s;
  s.rps = rps;
  s.nsplit = (R + rps - 1) / rps;
  s.slab = nullptr;
  return s;
}

struct Norm {                     // one BatchNorm of the plan: its input tensor's rows and chunks
  int rows, cr, nchunk;
  float* stats;
  float* bpart;
};
struct BnMiniPlan {
  int N, Cin, H, W, F;
  int H0, W0, H1, W1, H2, W2, R0, R1, R2;
  float eps;
  float *h0, *a0, *h1, *a1;
  Norm n[2];                      // of h0, h1
  float* part;                    // forward partials of the pass in flight
  // backward
  float *d1, *d0;                 // gradient of a1 / a0, then (in place) of h1 / h0
  double* gpart;
  Split w2, w1;
  float* slab0;
  size_t bytes;
};

BnMiniPlan make_plan(const node_ministem_shape* sh, bool keep, void* base) {
  BnMiniPlan p;
  memset(&p, 0, sizeof(p));
  p.N = sh->n; p.Cin = sh->in_ch; p.H = sh->h; p.W = sh->w; p.F = sh->filters; p.eps = sh->eps;
  p.H0 = p.H - 2; p.W0 = p.W - 2;
  p.H1 = down4(p.H0); p.W1 = down4(p.W0);
  p.H2 = down4(p.H1); p.W2 = down4(p.W1);
  p.R0 = p.N * p.H0 * p.W0; p.R1 = p.N * p.H1 * p.W1; p.R2 = p.N * p.H2 * p.W2;
  p.n[0].rows = p.R0;
  p.n[1].rows = p.R1;
  size_t npart = 0;
  for (Norm& k : p.n) {
    k.cr = bnmini_chunk_rows(k.rows);
    k.nchunk = (k.rows + k.cr - 1) / k.cr;
    const size_t need = (size_t)k.nchunk * 2 * MINI_C;
    if (need > npart) npart = need;
  }
  Bump b(base);
  p.h0 = b.take<float>((size_t)p.R0 * MINI_C);
  p.a0 = b.take<float>((size_t)p.R0 * MINI_C);
  p.h1 = b.take<float>((size_t)p.R1 * MINI_C);
  p.a1 = b.take<float>((size_t)p.R1 * MINI_C);
  p.n[0].stats = b.take<float>(2 * MINI_C);
  p.n[1].stats = b.take<float>(2 * MINI_C);
  p.part = b.take<float>(npart);
  if (keep) {
    p.d1 = b.take<float>((size_t)p.R1 * MINI_C);
    p.d0 = b.take<float>((size_t)p.R0 * MINI_C);
    p.gpart = b.take<double>(npart);
    for (Norm& k : p.n) k.bpart = b.take<float>((size_t)k.nchunk * MINI_C);
    p.w2 = make_split(p.R2, p.F);
    p.w2.slab = b.take<float>((size_t)p.w2.nsplit * p.F * MINI_C * 16);
    p.w1 = make_split(p.R1, MINI_C);
    p.w1.slab = b.take<float>((size_t)p.w1.nsplit * MINI_C * MINI_C * 16);
    p.slab0 = b.take<float>((size_t)p.N * MINI_C * 9 * p.Cin);
  }
  p.bytes = b.off + 256;
  return p;
}

int check_shape(const node_ministem_shape* sh) {
  if (!sh) return fail(NODE_ERR_NULL, "shape is NULL");
  if (sh->n <= 0 || sh->in_ch <= 0 || sh->h <= 0 || sh->w <= 0 || sh->filters <= 0) return fail(NODE_ERR_SHAPE, "bad stem shape");
  if (sh->h < 10 || sh->w < 10) return fail(NODE_ERR_SHAPE, "bad stem shape: the minimal stem takes images of 10 x 10 pixels and more (got %d x %d)", sh->h, sh->w);
  if (sh->in_ch > 3) return fail(NODE_ERR_UNSUPPORTED, "the stem's first layer takes in_ch <= 3 (got %d)", sh->in_ch);
  if (sh->filters < 64 || sh->filters > 4096 || (sh->filters & (sh->filters - 1)) != 0)
    return fail(NODE_ERR_UNSUPPORTED, "the minimal stem's kernels take filters a power of two in [64, 4096] (got %d)", sh->filters);
  const size_t biggest = (size_t)sh->n * sh->h * sh->w * MINI_C;
  if (biggest + 4096 >= ((size_t)1 << 31) || (size_t)sh->n * sh->h * sh->w * sh->filters >= ((size_t)1 << 31))
    return fail(NODE_ERR_UNSUPPORTED, "stem tensors must stay under 2^31 elements");
  return NODE_OK;
}

// node_ministem_params / node_ministem_grads: ten non-NULL, 16-byte aligned pointers
int check_ten(const void* s, const char* what) {
  const void* const* pp = reinterpret_cast<const void* const*>(s);
  for (int i = 0; i < 10; ++i) {
    if (!pp[i]) return fail(NODE_ERR_NULL, "stem %s %d is NULL", what, i);
    if (((uintptr_t)pp[i]) & 15) return fail(NODE_ERR_ARG, "stem %s %d must be 16-byte aligned", what, i);
  }
  return NODE_OK;
}

BnMiniArgs bn_args(const BnMiniPlan& p, const Norm& k, const float* h, const float* gamma, const float* beta) {
  BnMiniArgs a;
  memset(&a, 0, sizeof(a));
  a.h = h; a.gamma = gamma; a.beta = beta; a.stats = k.stats;
  a.rows = k.rows; a.chunk_rows = k.cr; a.nchunk = k.nchunk; a.eps = p.eps;
  return a;
}

#define LAUNCHED(what)                                  \
  do {                                                  \
    if ((rc = launch_ok(what)) != NODE_OK) return rc;   \
  } while (0)

// act = relu(norm(h)); leaves the batch statistics in the norm's `stats`
int norm_relu(const BnMiniPlan& p, const Norm& k, const float* h, const float* gamma, const float* beta, float* act, hipStream_t st) {
  int rc;
  BnMiniArgs a = bn_args(p, k, h, gamma, beta);
  a.part = p.part;
  launch_bnmini_stats(a, st);
  LAUNCHED("bnmini_stats");
  a.a = act;
  launch_bnmini_apply(a, st);
  LAUNCHED("bnmini_apply");
  return NODE_OK;
}

// in place on d: the activation's gradient -> the gradient of h; dgamma / dbeta and the bias partials only with `params`
int norm_relu_bwd(const BnMiniPlan& p, const Norm& k, const float* h, const float* gamma, const float* beta, float* d, float* dgamma,
                  float* dbeta, bool params, hipStream_t st) {
  int rc;
  BnMiniArgs a = bn_args(p, k, h, gamma, beta);
  a.d = d; a.gpart = p.gpart;
  launch_bnmini_bwd_stats(a, st);
  LAUNCHED("bnmini_bwd_stats");
  if (params) { a.dgamma = dgamma; a.dbeta = dbeta; a.bpart = k.bpart; }
  launch_bnmini_bwd_dx(a, st);
  LAUNCHED("bnmini_bwd_dx");
  return NODE_OK;
}

}  // namespace

extern "C" {

size_t node_bnministem_workspace_bytes(const node_ministem_shape* shape, int keep_for_backward) {
  if (check_shape(shape) != NODE_OK) return 0;
  return make_plan(shape, keep_for_backward != 0, nullptr).bytes;
}

int node_bnministem_describe(const node_ministem_shape* shape, node_bnministem_info out[2]) {
  if (!out) return fail(NODE_ERR_NULL, "out is NULL");
  memset(out, 0, 2 * sizeof(*out));
  const int rc = check_shape(shape);
  if (rc != NODE_OK) return rc;
  const BnMiniPlan p = make_plan(shape, true, nullptr);
  const Split* reader[2] = {&p.w1, &p.w2};      // the weight gradient of the convolution that reads the norm's output
  for (int i = 0; i < 2; ++i) {
    const Norm& k = p.n[i];
    out[i].rows = k.rows; out[i].chunk_rows = k.cr; out[i].nchunk = k.nchunk;
    out[i].last_chunk_rows = k.rows - (k.nchunk - 1) * k.cr;
    out[i].trip_rows = BNMINI_TRIP;
    out[i].wgrad_nsplit = reader[i]->nsplit; out[i].wgrad_rows_per_split = reader[i]->rps;
  }
  return NODE_OK;
}

int node_bnministem_fwd(const node_ministem_shape* shape, const node_ministem_params* prm, const float* x, float* out,
                        int keep_for_backward, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_shape(shape);
  if (rc != NODE_OK) return rc;
  if (!prm || !x || !out || !ws) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if ((rc = check_ten(prm, "parameter")) != NODE_OK) return rc;
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const BnMiniPlan p = make_plan(shape, keep_for_backward != 0, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "stem workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  launch_mini_conv0_fwd(x, prm->c0_w, prm->c0_b, p.h0, p.N, p.Cin, p.H, p.W, st);
  LAUNCHED("mini_conv0_fwd");
  if ((rc = norm_relu(p, p.n[0], p.h0, prm->n1_w, prm->n1_b, p.a0, st)) != NODE_OK) return rc;
  launch_mini_conv4_fwd(p.a0, prm->c1_w, prm->c1_b, p.h1, p.N, p.H0, p.W0, p.H1, p.W1, MINI_C, 0, st);
  LAUNCHED("mini_conv4_fwd");
  if ((rc = norm_relu(p, p.n[1], p.h1, prm->n2_w, prm->n2_b, p.a1, st)) != NODE_OK) return rc;
  launch_mini_conv4_fwd(p.a1, prm->c2_w, prm->c2_b, out, p.N, p.H1, p.W1, p.H2, p.W2, p.F, 1, st);
  return launch_ok("node_bnministem_fwd");
}

int node_bnministem_bwd(const node_ministem_shape* shape, const node_ministem_params* prm, const float* x, const float* grad_out,
                        const node_ministem_grads* gr, float* d_x, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_shape(shape);
  if (rc != NODE_OK) return rc;
  if (!prm || !x || !grad_out || !ws) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if (!gr && !d_x) return fail(NODE_ERR_NULL, "grads and d_x are both NULL: nothing to compute");
  if ((rc = check_ten(prm, "parameter")) != NODE_OK) return rc;
  if (gr && (rc = check_ten(gr, "gradient")) != NODE_OK) return rc;
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const BnMiniPlan p = make_plan(shape, true, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "stem workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int N = p.N, F = p.F;
  const int HW1 = p.H1 * p.W1, HW2 = p.H2 * p.W2;
  const MiniDy g2 = {grad_out, (long long)F * HW2, HW2, 1};
  const MiniDy g1 = {p.d1, (long long)MINI_C * HW1, 1, MINI_C};

  // the last convolution (4x4 / 2, 24 -> F): reads a1
  if (gr) {
    launch_mini_chansum(grad_out, gr->c2_b, N, F, HW2, st);
    LAUNCHED("mini_chansum");
    launch_mini_conv4_wgrad(g2, p.a1, p.w2.slab, N, p.H1, p.W1, p.H2, p.W2, F, p.w2.nsplit, p.w2.rps, st);
    LAUNCHED("mini_conv4_wgrad");
  }
  launch_mini_conv4_dgrad(g2, prm->c2_w, p.d1, N, p.H1, p.W1, p.H2, p.W2, F, st);
  LAUNCHED("mini_conv4_dgrad");
  if ((rc = norm_relu_bwd(p, p.n[1], p.h1, prm->n2_w, prm->n2_b, p.d1, gr ? gr->n2_w : nullptr, gr ? gr->n2_b : nullptr, gr != nullptr,
                          st)) != NODE_OK)
    return rc;
  // the middle convolution (4x4 / 2, 24 -> 24): reads a0
  if (gr) {
    launch_mini_conv4_wgrad(g1, p.a0, p.w1.slab, N, p.H0, p.W0, p.H1, p.W1, MINI_C, p.w1.nsplit, p.w1.rps, st);
    LAUNCHED("mini_conv4_wgrad");
  }
  launch_mini_conv4_dgrad(g1, prm->c1_w, p.d0, N, p.H0, p.W0, p.H1, p.W1, MINI_C, st);
  LAUNCHED("mini_conv4_dgrad");
  if ((rc = norm_relu_bwd(p, p.n[0], p.h0, prm->n1_w, prm->n1_b, p.d0, gr ? gr->n1_w : nullptr, gr ? gr->n1_b : nullptr, gr != nullptr,
                          st)) != NODE_OK)
    return rc;
  if (d_x) {   // the transposed first layer: the gradient of h0 -> the image
    launch_mini_conv0_dgrad(p.d0, prm->c0_w, d_x, N, p.Cin, p.H, p.W, st);
    LAUNCHED("mini_conv0_dgrad");
  }
  if (!gr) return launch_ok("node_bnministem_bwd");
  launch_mini_conv0_wgrad(x, p.d0, p.slab0, N, p.Cin, p.H, p.W, st);
  LAUNCHED("mini_conv0_wgrad");

  MiniSumArgs sa;
  memset(&sa, 0, sizeof(sa));
  int nj = 0;
  sa.job[nj++] = {p.w2.slab, gr->c2_w, p.w2.nsplit, (long long)F * MINI_C * 16, F * MINI_C * 16};
  sa.job[nj++] = {p.w1.slab, gr->c1_w, p.w1.nsplit, (long long)MINI_C * MINI_C * 16, MINI_C * MINI_C * 16};
  sa.job[nj++] = {p.slab0, gr->c0_w, N, (long long)MINI_C * 9 * p.Cin, MINI_C * 9 * p.Cin};
  sa.job[nj++] = {p.n[0].bpart, gr->c0_b, p.n[0].nchunk, MINI_C, MINI_C};
  sa.job[nj++] = {p.n[1].bpart, gr->c1_b, p.n[1].nchunk, MINI_C, MINI_C};
  sa.njobs = nj;
  launch_mini_sums(sa, st);
  return launch_ok("node_bnministem_bwd");
}

}  // extern "C"
