// C ABI of the `ode2` stem's hand-off (include/node_hip.h: node_downconv_fwd / node_downconv_bwd): GroupNorm -> ReLU ->
// nn.Conv2d(cin, cout, 4, 2, 1) with bias, model.py:199-223 (`conv2(norm(x))`), as a host-side plan of the stem's kernels
// (kernels_stem.hip).  NHWC inside the workspace, NCHW at the boundary.
//
// forward (5 launches):  filter -> triples + zero rows | NCHW -> NHWC | GN+ReLU (-> triples) | conv 4x4/2 (+ bias) | NHWC -> NCHW
// backward (6 launches): NCHW -> triples of dy (+ the bias gradient's partial sums) | weight gradient (one kernel row per
//                        workgroup) | data gradient (four parity classes of four taps) | GN backward | NHWC -> NCHW into d_x |
//                        ONE reduction launch: slabs -> dW, GroupNorm partials -> dgamma / dbeta, bias partials -> db
// With grads == NULL the backward is the data-gradient chain alone (4 launches).  Nothing is accumulated with atomics.
#include "host_common.h"
#include "stem.h"
#include "stem_plan.h"
#include <cstring>

using namespace node;

namespace {

struct DownPlan {
  int N, Cin, Cout, H, W, OH, OW, R, RO;
  float eps;
  Filt f;
  float *xh, *yn, *stats;
  Trip a;
  // backward
  Trip g;
  float *da, *dh, *gpart, *bpart;
  int nbpart;              // partial sums per output channel: one per (sample, block of 64 output pixels)
  Wg wg;
  size_t bytes;
};

DownPlan make_down_plan(const node_downconv_shape* sh, bool keep, void* base) {
  DownPlan p;
  memset(&p, 0, sizeof(p));
  p.N = sh->n; p.Cin = sh->cin; p.Cout = sh->cout; p.H = sh->h; p.W = sh->w; p.eps = sh->eps;
  p.OH = (p.H + 2 - 4) / 2 + 1; p.OW = (p.W + 2 - 4) / 2 + 1;
  p.R = p.N * p.H * p.W; p.RO = p.N * p.OH * p.OW;
  const int G = p.Cin < 32 ? p.Cin : 32;
  Bump b(base);
  p.f = take_filt(b, p.Cout, p.Cin, 16);
  p.xh = b.take<float>((size_t)p.R * p.Cin);
  p.a = take_trip(b, p.R, p.Cin);
  p.yn = b.take<float>((size_t)p.RO * p.Cout);
  p.stats = b.take<float>((size_t)p.N * G * 2);
  if (keep) {
    p.g = take_trip(b, p.RO, p.Cout);
    p.da = b.take<float>((size_t)p.R * p.Cin);
    p.dh = b.take<float>((size_t)p.R * p.Cin);
    p.gpart = b.take<float>((size_t)p.N * 2 * p.Cin);
    p.nbpart = p.N * ((p.OH * p.OW + 63) / 64);
    p.bpart = b.take<float>((size_t)p.nbpart * p.Cout);
    p.wg = take_wg(b, p.RO, p.Cout, p.Cin, 16, false);
  }
  p.bytes = b.off + 256;
  return p;
}

bool pow2_from_64(int c) { return c >= 64 && c <= 4096 && (c & (c - 1)) == 0; }

int check_down_shape(const node_downconv_shape* sh) {
  if (!sh) return fail(NODE_ERR_NULL, "shape is NULL");
  if (sh->n <= 0 || sh->cin <= 0 || sh->cout <= 0 || sh->h <= 0 || sh->w <= 0) return fail(NODE_ERR_SHAPE, "bad hand-off shape");
  if (sh->h < 4 || sh->w < 4) return fail(NODE_ERR_SHAPE, "bad hand-off shape: a 4x4 stride-2 convolution takes images of 4x4 pixels and more");
  if (!pow2_from_64(sh->cin) || !pow2_from_64(sh->cout))
    return fail(NODE_ERR_UNSUPPORTED, "the hand-off's kernels take filters (cin, cout) that are powers of two in [64, 4096]: 64-column GEMM "
                 "tiles, whole GroupNorm groups per power-of-two channel block (got %d -> %d)", sh->cin, sh->cout);
  const size_t big = (size_t)sh->n * sh->h * sh->w * (sh->cin > sh->cout ? sh->cin : sh->cout);
  if (big + 4096 >= ((size_t)1 << 31)) return fail(NODE_ERR_UNSUPPORTED, "hand-off tensors must stay under 2^31 elements");
  if (stem_gn_cb(sh->h * sh->w, sh->cin, sh->cin / 32) == 0)
    return fail(NODE_ERR_UNSUPPORTED, "the GroupNorm passes hold a (sample, channel block) in LDS: %d x %d pixels of %d channels "
                 "per group do not fit", sh->h, sh->w, sh->cin / 32);
  return NODE_OK;
}

}  // namespace

extern "C" {

size_t node_downconv_workspace_bytes(const node_downconv_shape* shape, int keep_for_backward) {
  if (check_down_shape(shape) != NODE_OK) return 0;
  return make_down_plan(shape, keep_for_backward != 0, nullptr).bytes;
}

int node_downconv_fwd(const node_downconv_shape* shape, const node_downconv_params* prm, const float* x, float* y,
                      int keep_for_backward, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_down_shape(shape);
  if (rc != NODE_OK) return rc;
  if (!prm || !x || !y || !ws) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if (!prm->gn_w || !prm->gn_b || !prm->conv_w || !prm->conv_b) return fail(NODE_ERR_NULL, "a hand-off parameter is NULL");
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const DownPlan p = make_down_plan(shape, keep_for_backward != 0, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "hand-off workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;

  SPrepArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.job[0] = {prm->conv_w, p.f.wf, p.f.wd, p.Cout, p.Cin, 16};
  pa.njobs = 1;
  pa.zero[0] = p.a.p + (size_t)p.a.rows * p.a.C; pa.zero_plane[0] = p.a.plane; pa.zero_c[0] = p.a.C;
  pa.nzero = 1;
  if (keep_for_backward) {
    pa.zero[1] = p.g.p + (size_t)p.g.rows * p.g.C; pa.zero_plane[1] = p.g.plane; pa.zero_c[1] = p.g.C;
    pa.nzero = 2;
  }
  launch_stem_prep(pa, st);
  if ((rc = launch_ok("stem_prep")) != NODE_OK) return rc;
  launch_stem_from_nchw(x, p.xh, nullptr, 0, p.N, p.Cin, p.H * p.W, st);
  if ((rc = launch_ok("stem_from_nchw")) != NODE_OK) return rc;
  {
    SGnArgs g = gn_args(p.xh, prm->gn_w, prm->gn_b, p.stats, p.N, p.H * p.W, p.Cin, p.eps);
    g.a3 = p.a.p; g.a_plane = p.a.plane;
    launch_stem_gn_fwd(g, st);
    if ((rc = launch_ok("stem_gn_fwd")) != NODE_OK) return rc;
  }
  {
    SConvArgs c = conv_fwd_args(p.a, p.f, p.yn, p.N, p.H, p.W, p.OH, p.OW, 4, 2, 1);
    c.bias = prm->conv_b;
    launch_stem_conv(c, st);
    if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
  }
  launch_stem_to_nchw(p.yn, y, p.N, p.Cout, p.OH * p.OW, st);
  return launch_ok("node_downconv_fwd");
}

int node_downconv_bwd(const node_downconv_shape* shape, const node_downconv_params* prm, const float* grad_y,
                      const node_downconv_grads* gr, float* d_x, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_down_shape(shape);
  if (rc != NODE_OK) return rc;
  if (!prm || !grad_y || !d_x || !ws) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if (!prm->gn_w || !prm->gn_b || !prm->conv_w || !prm->conv_b) return fail(NODE_ERR_NULL, "a hand-off parameter is NULL");
  if (gr && (!gr->gn_w || !gr->gn_b || !gr->conv_w || !gr->conv_b)) return fail(NODE_ERR_NULL, "a hand-off gradient is NULL");
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const DownPlan p = make_down_plan(shape, true, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "hand-off workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int HW = p.H * p.W, OHW = p.OH * p.OW;

  launch_stem_from_nchw(grad_y, nullptr, p.g.p, p.g.plane, p.N, p.Cout, OHW, st, gr ? p.bpart : nullptr);
  if ((rc = launch_ok("stem_from_nchw")) != NODE_OK) return rc;
  if (gr) {
    launch_stem_wgrad(wgrad_args(p.g, nullptr, p.a, p.wg, p.N, p.H, p.W, p.OH, p.OW, p.Cin, p.Cout, 4, 2, 1), st);
    if ((rc = launch_ok("stem_wgrad")) != NODE_OK) return rc;
  }
  launch_stem_conv(conv_dgrad_args(p.g, p.f, p.da, p.N, p.OH, p.OW, p.H, p.W, 4, 2, 1), st);
  if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
  {
    SGnArgs g = gn_args(p.xh, prm->gn_w, prm->gn_b, p.stats, p.N, HW, p.Cin, p.eps);
    g.da = p.da; g.dh = p.dh; g.dh3 = nullptr; g.gpart = p.gpart;
    launch_stem_gn_bwd(g, st);
    if ((rc = launch_ok("stem_gn_bwd")) != NODE_OK) return rc;
  }
  launch_stem_to_nchw(p.dh, d_x, p.N, p.Cin, HW, st);
  if ((rc = launch_ok("stem_to_nchw")) != NODE_OK) return rc;
  if (!gr) return launch_ok("node_downconv_bwd");

  SReduceArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.job[0] = {p.wg.slab, gr->conv_w, nullptr, 0, p.wg.nsplit, p.Cout, p.Cin, 16};
  ra.job[1] = {p.gpart, gr->gn_w, gr->gn_b, 2, p.N, p.Cin, 0, 0};
  ra.job[2] = {p.bpart, gr->conv_b, nullptr, 3, p.nbpart, p.Cout, 0, 0};
  ra.njobs = 3;
  launch_stem_reduce(ra, st);
  if ((rc = launch_ok("stem_reduce")) != NODE_OK) return rc;
  return launch_ok("node_downconv_bwd");
}

}  // extern "C"
