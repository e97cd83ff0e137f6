// C ABI of the `minimal` stem (include/node_hip.h: node_ministem_fwd / node_ministem_bwd) -- model.py:129-145
// (`MinimalConvDownsample`): Conv2d(in_ch, 24, 3, 1) | GN(24, 24) + ReLU | Conv2d(24, 24, 4, 2, 1) | GN(24, 24) + ReLU |
// Conv2d(24, filters, 4, 2, 1), every convolution with bias -- as a host-side plan of kernels_ministem.hip.  NHWC of channel
// pitch 24 inside the workspace.
//
// forward (5 launches):   conv0 | GN + ReLU | conv 4x4/2 | GN + ReLU | conv 4x4/2 -> NCHW
// backward, last layer first:
//   parameters (5 launches): the last bias gradient | per 4x4 convolution its weight gradient's slabs | conv0's per-sample
//                          weight gradient | ONE launch of sums: three slab sets, two GroupNorm partials, two bias partials
//   data chain (4 launches): per 4x4 convolution its data gradient and the GroupNorm backward (in place)
//   image (1 launch):      the transposed first layer
// grads == NULL runs the data chain and the image's launch alone; d_x == NULL leaves the image's launch out.
#include "host_common.h"
#include "ministem.h"
#include "stem_plan.h"
#include <cstring>

using namespace node;

namespace {

inline int down4(int h) { return (h + 2 - 4) / 2 + 1; }     // 4x4 stride 2 pad 1

struct Split { int nsplit, rps; float* slab; };

// split-K of a weight gradient over R rows: about 256 workgroups, whole chunks of 32 rows
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

struct MiniPlan {
  int N, Cin, H, W, F;
  int H0, W0, H1, W1, H2, W2, R0, R1, R2;
  float eps;
  float *h0, *a0, *h1, *a1;
  float* stats[2];
  // backward
  float *d1, *d0;            // gradient of a1 / a0, then (in place) of h1 / h0
  float* gpart[2];
  float* bpart[2];
  Split w2, w1;
  float* slab0;
  size_t bytes;
};

MiniPlan make_plan(const node_ministem_shape* sh, bool keep, void* base) {
  MiniPlan p;
  memset(&p, 0, sizeof(p));
  p.N = sh->n; p.Cin = sh->in_ch; p.H = sh->h; p.W = sh->w; p.F = sh->filters; p.eps = sh->eps;
  p.H0 = p.H - 2; p.W0 = p.W - 2;
  p.H1 = down4(p.H0); p.W1 = down4(p.W0);
  p.H2 = down4(p.H1); p.W2 = down4(p.W1);
  p.R0 = p.N * p.H0 * p.W0; p.R1 = p.N * p.H1 * p.W1; p.R2 = p.N * p.H2 * p.W2;
  Bump b(base);
  p.h0 = b.take<float>((size_t)p.R0 * MINI_C);
  p.a0 = b.take<float>((size_t)p.R0 * MINI_C);
  p.h1 = b.take<float>((size_t)p.R1 * MINI_C);
  p.a1 = b.take<float>((size_t)p.R1 * MINI_C);
  p.stats[0] = b.take<float>((size_t)p.N * MINI_C * 2);
  p.stats[1] = b.take<float>((size_t)p.N * MINI_C * 2);
  if (keep) {
    p.d1 = b.take<float>((size_t)p.R1 * MINI_C);
    p.d0 = b.take<float>((size_t)p.R0 * MINI_C);
    for (int i = 0; i < 2; ++i) {
      p.gpart[i] = b.take<float>((size_t)p.N * 2 * MINI_C);
      p.bpart[i] = b.take<float>((size_t)p.N * MINI_C);
    }
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

int check_ten(const void* s, const char* what) {
  const float* const* pp = reinterpret_cast<const float* const*>(s);
  for (int i = 0; i < 10; ++i)
    if (!pp[i]) return fail(NODE_ERR_NULL, "stem %s %d is NULL", what, i);
  return NODE_OK;
}

}  // namespace

extern "C" {

size_t node_ministem_workspace_bytes(const node_ministem_shape* shape, int keep_for_backward) {
  if (check_shape(shape) != NODE_OK) return 0;
  return make_plan(shape, keep_for_backward != 0, nullptr).bytes;
}

int node_ministem_fwd(const node_ministem_shape* shape, const node_ministem_params* prm, const float* x, float* out,
                      int keep_for_backward, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_shape(shape);
  if (rc != NODE_OK) return rc;
  if (!prm || !x || !out || !ws) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if ((rc = check_ten(prm, "parameter")) != NODE_OK) return rc;
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const MiniPlan p = make_plan(shape, keep_for_backward != 0, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "stem workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  launch_mini_conv0_fwd(x, prm->c0_w, prm->c0_b, p.h0, p.N, p.Cin, p.H, p.W, st);
  if ((rc = launch_ok("mini_conv0_fwd")) != NODE_OK) return rc;
  launch_mini_gn_fwd(p.h0, prm->n1_w, prm->n1_b, p.a0, p.stats[0], p.N, p.H0 * p.W0, p.eps, st);
  if ((rc = launch_ok("mini_gn_fwd")) != NODE_OK) return rc;
  launch_mini_conv4_fwd(p.a0, prm->c1_w, prm->c1_b, p.h1, p.N, p.H0, p.W0, p.H1, p.W1, MINI_C, 0, st);
  if ((rc = launch_ok("mini_conv4_fwd")) != NODE_OK) return rc;
  launch_mini_gn_fwd(p.h1, prm->n2_w, prm->n2_b, p.a1, p.stats[1], p.N, p.H1 * p.W1, p.eps, st);
  if ((rc = launch_ok("mini_gn_fwd")) != NODE_OK) return rc;
  launch_mini_conv4_fwd(p.a1, prm->c2_w, prm->c2_b, out, p.N, p.H1, p.W1, p.H2, p.W2, p.F, 1, st);
  return launch_ok("node_ministem_fwd");
}

int node_ministem_bwd(const node_ministem_shape* shape, const node_ministem_params* prm, const float* x, const float* grad_out,
                      const node_ministem_grads* gr, float* d_x, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_shape(shape);
  if (rc != NODE_OK) return rc;
  if (!prm || !x || !grad_out || !ws) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if (!gr && !d_x) return fail(NODE_ERR_NULL, "grads and d_x are both NULL: nothing to compute");
  if ((rc = check_ten(prm, "parameter")) != NODE_OK) return rc;
  if (gr && (rc = check_ten(gr, "gradient")) != NODE_OK) return rc;
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const MiniPlan p = make_plan(shape, true, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "stem workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int N = p.N, F = p.F;
  const int HW0 = p.H0 * p.W0, HW1 = p.H1 * p.W1, HW2 = p.H2 * p.W2;
  const MiniDy g2 = {grad_out, (long long)F * HW2, HW2, 1};
  const MiniDy g1 = {p.d1, (long long)MINI_C * HW1, 1, MINI_C};

  // the last convolution (4x4 / 2, 24 -> F): reads a1
  if (gr) {
    launch_mini_chansum(grad_out, gr->c2_b, N, F, HW2, st);
    if ((rc = launch_ok("mini_chansum")) != NODE_OK) return rc;
    launch_mini_conv4_wgrad(g2, p.a1, p.w2.slab, N, p.H1, p.W1, p.H2, p.W2, F, p.w2.nsplit, p.w2.rps, st);
    if ((rc = launch_ok("mini_conv4_wgrad")) != NODE_OK) return rc;
  }
  launch_mini_conv4_dgrad(g2, prm->c2_w, p.d1, N, p.H1, p.W1, p.H2, p.W2, F, st);
  if ((rc = launch_ok("mini_conv4_dgrad")) != NODE_OK) return rc;
  launch_mini_gn_bwd(p.h1, p.a1, prm->n2_w, p.stats[1], p.d1, p.gpart[1], p.bpart[1], N, HW1, st);
  if ((rc = launch_ok("mini_gn_bwd")) != NODE_OK) return rc;
  // the middle convolution (4x4 / 2, 24 -> 24): reads a0
  if (gr) {
    launch_mini_conv4_wgrad(g1, p.a0, p.w1.slab, N, p.H0, p.W0, p.H1, p.W1, MINI_C, p.w1.nsplit, p.w1.rps, st);
    if ((rc = launch_ok("mini_conv4_wgrad")) != NODE_OK) return rc;
  }
  launch_mini_conv4_dgrad(g1, prm->c1_w, p.d0, N, p.H0, p.W0, p.H1, p.W1, MINI_C, st);
  if ((rc = launch_ok("mini_conv4_dgrad")) != NODE_OK) return rc;
  launch_mini_gn_bwd(p.h0, p.a0, prm->n1_w, p.stats[0], p.d0, p.gpart[0], p.bpart[0], N, HW0, st);
  if ((rc = launch_ok("mini_gn_bwd")) != NODE_OK) return rc;
  if (d_x) {   // the transposed first layer: the gradient of h0 -> the image
    launch_mini_conv0_dgrad(p.d0, prm->c0_w, d_x, N, p.Cin, p.H, p.W, st);
    if ((rc = launch_ok("mini_conv0_dgrad")) != NODE_OK) return rc;
  }
  if (!gr) return launch_ok("node_ministem_bwd");
  launch_mini_conv0_wgrad(x, p.d0, p.slab0, N, p.Cin, p.H, p.W, st);
  if ((rc = launch_ok("mini_conv0_wgrad")) != NODE_OK) return rc;

  MiniSumArgs sa;
  memset(&sa, 0, sizeof(sa));
  int nj = 0;
  sa.job[nj++] = {p.w2.slab, gr->c2_w, p.w2.nsplit, (long long)F * MINI_C * 16, F * MINI_C * 16};
  sa.job[nj++] = {p.w1.slab, gr->c1_w, p.w1.nsplit, (long long)MINI_C * MINI_C * 16, MINI_C * MINI_C * 16};
  sa.job[nj++] = {p.slab0, gr->c0_w, N, (long long)MINI_C * 9 * p.Cin, MINI_C * 9 * p.Cin};
  sa.job[nj++] = {p.gpart[0], gr->n1_w, N, 2 * MINI_C, MINI_C};
  sa.job[nj++] = {p.gpart[0] + MINI_C, gr->n1_b, N, 2 * MINI_C, MINI_C};
  sa.job[nj++] = {p.gpart[1], gr->n2_w, N, 2 * MINI_C, MINI_C};
  sa.job[nj++] = {p.gpart[1] + MINI_C, gr->n2_b, N, 2 * MINI_C, MINI_C};
  sa.job[nj++] = {p.bpart[0], gr->c0_b, N, MINI_C, MINI_C};
  sa.job[nj++] = {p.bpart[1], gr->c1_b, N, MINI_C, MINI_C};
  sa.njobs = nj;
  launch_mini_sums(sa, st);
  return launch_ok("node_ministem_bwd");
}

}  // extern "C"
