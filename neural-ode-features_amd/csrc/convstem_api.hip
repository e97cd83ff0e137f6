// C ABI of the `convolution` stem (include/node_hip.h: node_convstem_fwd / node_convstem_bwd) -- model.py:148-164
// (`ConvDownsample`): Conv2d(in_ch, 64, 3, 1) | GN + ReLU | Conv2d(64, 64, 4, 2, 1) | GN + ReLU | Conv2d(64, filters, 4, 2, 1),
// every convolution with bias -- as a host-side plan of the stem's kernels (kernels_stem.hip).  NHWC inside the workspace.
//
// forward (7 launches):   filters -> triples + zero rows | conv0 | GN+ReLU | conv 4x4/2 | GN+ReLU | conv 4x4/2 | NHWC -> NCHW
// backward (10 launches): NCHW -> triples of dy (+ the last bias gradient's partial sums) | per 4x4 convolution, last first:
//                         weight gradient, data gradient, GN backward | the middle bias gradient's partial sums | conv0's weight
//                         and bias gradient | ONE reduction launch: three slab sets, two GroupNorm partials, two bias partials
// node_convstem_bwd_dx adds the transposed first layer behind dh0 (the image's gradient) and, with grads == NULL, runs the
// data-gradient chain alone: no weight-gradient, partial-sum or reduction launch.  Nothing is accumulated with atomics.
#include "host_common.h"
#include "stem.h"
#include "stem_plan.h"
#include <cstring>

using namespace node;

namespace {

constexpr int BIAS_ROWS = 256;      // rows per partial sum of the middle convolution's bias gradient

inline int down4(int h) { return (h + 2 - 4) / 2 + 1; }     // 4x4 stride 2 pad 1

struct ConvStemPlan {
  int N, Cin0, H, W, F;
  int H0, W0, H1, W1, H2, W2, R0, R1, R2;
  float eps;
  float* w0t;
  Filt c1, c2;
  float *h0, *h1, *outn;
  Trip a0, a1;
  float* stats[2];
  // backward
  Trip g2, dh1t;
  float *da1, *dh1, *da0, *dh0;
  float* gpart[2];
  float *bpart2, *bpart1;
  int nb2, nb1;
  Wg w2, w1, w0;
  size_t bytes;
};

ConvStemPlan make_convstem_plan(const node_convstem_shape* sh, bool keep, void* base) {
  ConvStemPlan p;
  memset(&p, 0, sizeof(p));
  p.N = sh->n; p.Cin0 = sh->in_ch; p.H = sh->h; p.W = sh->w; p.F = sh->filters; p.eps = sh->eps;
  p.H0 = p.H - 2; p.W0 = p.W - 2;
  p.H1 = down4(p.H0); p.W1 = down4(p.W0);
  p.H2 = down4(p.H1); p.W2 = down4(p.W1);
  p.R0 = p.N * p.H0 * p.W0; p.R1 = p.N * p.H1 * p.W1; p.R2 = p.N * p.H2 * p.W2;
  const int F = p.F;
  Bump b(base);
  p.w0t = b.take<float>(28 * 64);
  p.c1 = take_filt(b, 64, 64, 16);
  p.c2 = take_filt(b, F, 64, 16);
  p.h0 = b.take<float>((size_t)p.R0 * 64);
  p.a0 = take_trip(b, p.R0, 64);
  p.h1 = b.take<float>((size_t)p.R1 * 64);
  p.a1 = take_trip(b, p.R1, 64);
  p.outn = b.take<float>((size_t)p.R2 * F);
  p.stats[0] = b.take<float>((size_t)p.N * 32 * 2);
  p.stats[1] = b.take<float>((size_t)p.N * 32 * 2);
  if (keep) {
    p.g2 = take_trip(b, p.R2, F);
    p.da1 = b.take<float>((size_t)p.R1 * 64);
    p.dh1 = b.take<float>((size_t)p.R1 * 64);
    p.dh1t = take_trip(b, p.R1, 64);
    p.da0 = b.take<float>((size_t)p.R0 * 64);
    p.dh0 = b.take<float>((size_t)p.R0 * 64);
    p.gpart[0] = b.take<float>((size_t)p.N * 2 * 64);
    p.gpart[1] = b.take<float>((size_t)p.N * 2 * 64);
    p.nb2 = p.N * ((p.H2 * p.W2 + 63) / 64);
    p.bpart2 = b.take<float>((size_t)p.nb2 * F);
    p.nb1 = (p.R1 + BIAS_ROWS - 1) / BIAS_ROWS;
    p.bpart1 = b.take<float>((size_t)p.nb1 * 64);
    p.w2 = take_wg(b, p.R2, F, 64, 16, false);
    p.w1 = take_wg(b, p.R1, 64, 64, 16, false);
    {   // conv0: K steps of two pixels over R0 rows, one 64 x 32 slab per workgroup (as the residual stem's plan)
      int ns = p.R0 / 256;
      if (ns > 1024) ns = 1024;
      if (ns < 1) ns = 1;
      const int rps = ((p.R0 + ns - 1) / ns + 7) & ~7;
      p.w0.rps = rps;
      p.w0.nsplit = (p.R0 + rps - 1) / rps;
      p.w0.slab = b.take<float>((size_t)p.w0.nsplit * 64 * 32);
      p.w0.slab2 = nullptr;
    }
  }
  p.bytes = b.off + 256;
  return p;
}

int check_convstem_shape(const node_convstem_shape* sh) {
  if (!sh) return fail(NODE_ERR_NULL, "shape is NULL");
  if (sh->n <= 0 || sh->in_ch <= 0 || sh->h <= 0 || sh->w <= 0 || sh->filters <= 0) return fail(NODE_ERR_SHAPE, "bad stem shape");
  if (sh->h < 10 || sh->w < 10) return fail(NODE_ERR_SHAPE, "bad stem shape: the convolution stem takes images of 10 x 10 pixels and more (got %d x %d)", sh->h, sh->w);
  if (sh->in_ch > 3) return fail(NODE_ERR_UNSUPPORTED, "the stem's first layer takes in_ch <= 3 (got %d)", sh->in_ch);
  if (sh->filters < 64 || sh->filters > 4096 || (sh->filters & (sh->filters - 1)) != 0)
    return fail(NODE_ERR_UNSUPPORTED, "the stem's kernels take filters a power of two in [64, 4096]: 64-column GEMM tiles (got %d)", sh->filters);
  const size_t biggest = (size_t)sh->n * (sh->h - 2) * (sh->w - 2) * 64;
  if (biggest + 4096 >= ((size_t)1 << 31) || (size_t)sh->n * sh->h * sh->w * sh->filters >= ((size_t)1 << 31))
    return fail(NODE_ERR_UNSUPPORTED, "stem tensors must stay under 2^31 elements");
  if (stem_gn_cb((sh->h - 2) * (sh->w - 2), 64, 2) == 0)
    return fail(NODE_ERR_UNSUPPORTED, "the stem's GroupNorm passes hold (sample, 8 channels) blocks in LDS: images up to %d pixels "
                 "behind the first layer (got %d x %d)", 150 * 1024 / 64, sh->h - 2, sh->w - 2);
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

size_t node_convstem_workspace_bytes(const node_convstem_shape* shape, int keep_for_backward) {
  if (check_convstem_shape(shape) != NODE_OK) return 0;
  return make_convstem_plan(shape, keep_for_backward != 0, nullptr).bytes;
}

int node_convstem_fwd(const node_convstem_shape* shape, const node_convstem_params* prm, const float* x, float* out,
                      int keep_for_backward, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_convstem_shape(shape);
  if (rc != NODE_OK) return rc;
  if (!prm || !x || !out || !ws) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if ((rc = check_ten(prm, "parameter")) != NODE_OK) return rc;
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const ConvStemPlan p = make_convstem_plan(shape, keep_for_backward != 0, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "stem workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int N = p.N, F = p.F;

  SPrepArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.job[0] = {prm->c1_w, p.c1.wf, p.c1.wd, 64, 64, 16};
  pa.job[1] = {prm->c2_w, p.c2.wf, p.c2.wd, F, 64, 16};
  pa.njobs = 2;
  pa.w0 = prm->c0_w; pa.w0t = p.w0t; pa.k0 = 9 * p.Cin0;
  const Trip* tz[4] = {&p.a0, &p.a1, &p.g2, &p.dh1t};
  pa.nzero = keep_for_backward ? 4 : 2;
  for (int i = 0; i < pa.nzero; ++i) {
    pa.zero[i] = tz[i]->p + (size_t)tz[i]->rows * tz[i]->C;
    pa.zero_plane[i] = tz[i]->plane;
    pa.zero_c[i] = tz[i]->C;
  }
  launch_stem_prep(pa, st);
  if ((rc = launch_ok("stem_prep")) != NODE_OK) return rc;
  launch_stem_conv0_fwd(x, p.w0t, prm->c0_b, p.h0, N, p.Cin0, p.H, p.W, st);
  if ((rc = launch_ok("stem_conv0_fwd")) != NODE_OK) return rc;
  {
    SGnArgs g = gn_args(p.h0, prm->n1_w, prm->n1_b, p.stats[0], N, p.H0 * p.W0, 64, p.eps);
    g.a3 = p.a0.p; g.a_plane = p.a0.plane;
    launch_stem_gn_fwd(g, st);
    if ((rc = launch_ok("stem_gn_fwd")) != NODE_OK) return rc;
  }
  {
    SConvArgs c = conv_fwd_args(p.a0, p.c1, p.h1, N, p.H0, p.W0, p.H1, p.W1, 4, 2, 1);
    c.bias = prm->c1_b;
    launch_stem_conv(c, st);
    if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
  }
  {
    SGnArgs g = gn_args(p.h1, prm->n2_w, prm->n2_b, p.stats[1], N, p.H1 * p.W1, 64, p.eps);
    g.a3 = p.a1.p; g.a_plane = p.a1.plane;
    launch_stem_gn_fwd(g, st);
    if ((rc = launch_ok("stem_gn_fwd")) != NODE_OK) return rc;
  }
  {
    SConvArgs c = conv_fwd_args(p.a1, p.c2, p.outn, N, p.H1, p.W1, p.H2, p.W2, 4, 2, 1);
    c.bias = prm->c2_b;
    launch_stem_conv(c, st);
    if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
  }
  launch_stem_to_nchw(p.outn, out, N, F, p.H2 * p.W2, st);
  return launch_ok("node_convstem_fwd");
}

}  // extern "C"

namespace {
// node_convstem_bwd (d_x NULL, gr required) and node_convstem_bwd_dx (d_x required, gr nullable: the data-gradient chain alone)
int convstem_bwd(const node_convstem_shape* shape, const node_convstem_params* prm, const float* x, const float* grad_out,
                 const node_convstem_grads* gr, float* d_x, void* ws, size_t ws_bytes, void* stream, const char* who) {
  int rc = check_convstem_shape(shape);
  if (rc != NODE_OK) return rc;
  if (!prm || !x || !grad_out || (!gr && !d_x) || !ws) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if ((rc = check_ten(prm, "parameter")) != NODE_OK || (gr && (rc = check_ten(gr, "gradient")) != NODE_OK)) return rc;
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const ConvStemPlan p = make_convstem_plan(shape, true, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "stem workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int N = p.N, F = p.F;
  const int HW0 = p.H0 * p.W0, HW1 = p.H1 * p.W1, HW2 = p.H2 * p.W2;

  launch_stem_from_nchw(grad_out, nullptr, p.g2.p, p.g2.plane, N, F, HW2, st, gr ? p.bpart2 : nullptr);
  if ((rc = launch_ok("stem_from_nchw")) != NODE_OK) return rc;
  // the last convolution (4x4 / 2, 64 -> F): reads a1
  if (gr) {
    launch_stem_wgrad(wgrad_args(p.g2, nullptr, p.a1, p.w2, N, p.H1, p.W1, p.H2, p.W2, 64, F, 4, 2, 1), st);
    if ((rc = launch_ok("stem_wgrad")) != NODE_OK) return rc;
  }
  launch_stem_conv(conv_dgrad_args(p.g2, p.c2, p.da1, N, p.H2, p.W2, p.H1, p.W1, 4, 2, 1), st);
  if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
  {   // the gradient of h1 = the middle convolution's output: fp32 for its bias gradient, triples for the two GEMMs
    SGnArgs g = gn_args(p.h1, prm->n2_w, prm->n2_b, p.stats[1], N, HW1, 64, p.eps);
    g.da = p.da1; g.dh = p.dh1; g.dh3 = p.dh1t.p; g.dh_plane = p.dh1t.plane; g.gpart = p.gpart[1];
    launch_stem_gn_bwd(g, st);
    if ((rc = launch_ok("stem_gn_bwd")) != NODE_OK) return rc;
  }
  // the middle convolution (4x4 / 2, 64 -> 64): reads a0
  if (gr) {
    launch_stem_colsum(p.dh1, p.bpart1, p.R1, 64, BIAS_ROWS, st);
    if ((rc = launch_ok("stem_colsum")) != NODE_OK) return rc;
    launch_stem_wgrad(wgrad_args(p.dh1t, nullptr, p.a0, p.w1, N, p.H0, p.W0, p.H1, p.W1, 64, 64, 4, 2, 1), st);
    if ((rc = launch_ok("stem_wgrad")) != NODE_OK) return rc;
  }
  launch_stem_conv(conv_dgrad_args(p.dh1t, p.c1, p.da0, N, p.H1, p.W1, p.H0, p.W0, 4, 2, 1), st);
  if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
  {
    SGnArgs g = gn_args(p.h0, prm->n1_w, prm->n1_b, p.stats[0], N, HW0, 64, p.eps);
    g.da = p.da0; g.dh = p.dh0; g.dh3 = nullptr; g.gpart = p.gpart[0];
    launch_stem_gn_bwd(g, st);
    if ((rc = launch_ok("stem_gn_bwd")) != NODE_OK) return rc;
  }
  if (d_x) {   // the transposed first layer (the residual stem's Conv2d(in_ch, 64, 3, 1)): dh0 -> the image
    launch_stem_conv0_dgrad(p.dh0, prm->c0_w, d_x, N, p.Cin0, p.H, p.W, st);
    if ((rc = launch_ok("stem_conv0_dgrad")) != NODE_OK) return rc;
  }
  if (!gr) return launch_ok(who);
  launch_stem_conv0_wgrad(x, p.dh0, p.w0.slab, N, p.Cin0, p.H, p.W, p.w0.nsplit, p.w0.rps, st);
  if ((rc = launch_ok("stem_conv0_wgrad")) != NODE_OK) return rc;

  SReduceArgs ra;
  memset(&ra, 0, sizeof(ra));
  int nj = 0;
  ra.job[nj++] = {p.w2.slab, gr->c2_w, nullptr, 0, p.w2.nsplit, F, 64, 16};
  ra.job[nj++] = {p.w1.slab, gr->c1_w, nullptr, 0, p.w1.nsplit, 64, 64, 16};
  ra.job[nj++] = {p.w0.slab, gr->c0_w, gr->c0_b, 1, p.w0.nsplit, 64, 9 * p.Cin0, 1};
  ra.job[nj++] = {p.gpart[0], gr->n1_w, gr->n1_b, 2, N, 64, 0, 0};
  ra.job[nj++] = {p.gpart[1], gr->n2_w, gr->n2_b, 2, N, 64, 0, 0};
  ra.job[nj++] = {p.bpart1, gr->c1_b, nullptr, 3, p.nb1, 64, 0, 0};
  ra.job[nj++] = {p.bpart2, gr->c2_b, nullptr, 3, p.nb2, F, 0, 0};
  ra.njobs = nj;
  launch_stem_reduce(ra, st);
  if ((rc = launch_ok("stem_reduce")) != NODE_OK) return rc;
  return launch_ok(who);
}
}  // namespace

extern "C" {

int node_convstem_bwd(const node_convstem_shape* shape, const node_convstem_params* prm, const float* x, const float* grad_out,
                      const node_convstem_grads* gr, void* ws, size_t ws_bytes, void* stream) {
  if (!gr) {
    const int rc = check_convstem_shape(shape);
    return rc != NODE_OK ? rc : fail(NODE_ERR_NULL, "a required pointer is NULL");
  }
  return convstem_bwd(shape, prm, x, grad_out, gr, nullptr, ws, ws_bytes, stream, "node_convstem_bwd");
}

int node_convstem_bwd_dx(const node_convstem_shape* shape, const node_convstem_params* prm, const float* x, const float* grad_out,
                         const node_convstem_grads* gr, float* d_x, void* ws, size_t ws_bytes, void* stream) {
  if (!d_x) {
    const int rc = check_convstem_shape(shape);
    return rc != NODE_OK ? rc : fail(NODE_ERR_NULL, "a required pointer is NULL");
  }
  return convstem_bwd(shape, prm, x, grad_out, gr, d_x, ws, ws_bytes, stream, "node_convstem_bwd_dx");
}

}  // extern "C"
