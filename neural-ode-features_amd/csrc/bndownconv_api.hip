// C ABI of the `ode2` stem's hand-off with norm = 'batch' (include/node_hip.h: node_bndownconv_fwd / node_bndownconv_bwd):
// BatchNorm (model.py:274: nn.BatchNorm2d(C, track_running_stats=False)) -> ReLU -> nn.Conv2d(cin, cout, 4, 2, 1) with bias,
// model.py:199-223 (`conv2(norm(x))`), as a host-side plan: downconv_api.hip's with the BatchNorm passes of kernels_batchnorm.hip
// in place of the GroupNorm passes.  NHWC inside the workspace, NCHW at the boundary.
//
// forward (6 launches):  filter -> triples + zero rows | NCHW -> NHWC | stats, apply (norm + ReLU -> triples) | conv 4x4/2 (+ bias) |
//                        NHWC -> NCHW
// backward (7 launches): NCHW -> triples of dy (+ the bias gradient's partial sums) | weight gradient | data gradient (four parity
//                        classes of four taps) | BatchNorm sums, dx | NHWC -> NCHW into d_x | ONE reduction launch: slabs -> dW, bias
//                        partials -> db (dgamma / dbeta leave the dx pass's chunk-0 workgroups)
// With grads == NULL the backward is the data-gradient chain alone (5 launches).  Nothing is accumulated with atomics.
//
// slices > 1 (the forward with keep_for_backward = 0 only): n = T * (n / T) samples are the T slices of a trajectory, which
// model.py:214-216 sends through the norm slice by slice -- BatchNorm's statistics are per slice, so the GroupNorm hand-off's
// trick (T N samples as one batch) would be wrong here.  The two forward passes take the slice count instead (batchnorm.h): chunks
// that never straddle a slice, statistics per (slice, channel), chunk_rows what ONE slice's plan takes -- every slice has the bits
// of its own unsliced call.  The convolution is per sample and sees one batch of T N samples.
//
// The 16-tap geometry of k_stem_conv / k_stem_wgrad takes any cin, cout % 64 == 0 (bnconvstem_api.hip says where that was read),
// and no pass here holds an image in LDS: neither the GroupNorm hand-off's power-of-two rule nor its image limit applies.
#include "bnfunc.h"
#include <cstring>

using namespace node;

namespace {

struct BnDownPlan {
  int N, Cin, Cout, H, W, OH, OW, R, RO;
  int slices, rps, cr, cps, nchunk;      // rows per slice, rows per chunk, chunks per slice, slices * cps
  float eps;
  Filt f;
  float *xh, *yn, *stats, *part;
  Trip a;
  // backward
  Trip g;
  float *da, *dh, *bpart;
  double* gpart;
  int nbpart;              // partial sums per output channel: one per (sample, block of 64 output pixels)
  Wg wg;
  size_t bytes;
};

BnDownPlan make_plan(const node_bndownconv_shape* sh, bool keep, void* base) {
  BnDownPlan p;
  memset(&p, 0, sizeof(p));
  p.N = sh->n; p.Cin = sh->cin; p.Cout = sh->cout; p.H = sh->h; p.W = sh->w; p.eps = sh->eps;
  p.OH = (p.H + 2 - 4) / 2 + 1; p.OW = (p.W + 2 - 4) / 2 + 1;
  p.R = p.N * p.H * p.W; p.RO = p.N * p.OH * p.OW;
  p.slices = sh->slices;
  p.rps = p.R / p.slices;
  p.cr = bnstem_chunk_rows(p.rps, p.Cin);      // the policy of the stems' tensors, for ONE slice
  p.cps = (p.rps + p.cr - 1) / p.cr;
  p.nchunk = p.slices * p.cps;
  Bump b(base);
  p.f = take_filt(b, p.Cout, p.Cin, 16);
  p.xh = b.take<float>((size_t)p.R * p.Cin);
  p.a = take_trip(b, p.R, p.Cin);
  p.yn = b.take<float>((size_t)p.RO * p.Cout);
  p.stats = b.take<float>((size_t)p.slices * 2 * p.Cin);
  p.part = b.take<float>((size_t)p.nchunk * 2 * p.Cin);
  if (keep) {
    p.g = take_trip(b, p.RO, p.Cout);
    p.da = b.take<float>((size_t)p.R * p.Cin);
    p.dh = b.take<float>((size_t)p.R * p.Cin);
    p.gpart = b.take<double>((size_t)p.nchunk * 2 * p.Cin);
    p.nbpart = p.N * ((p.OH * p.OW + 63) / 64);
    p.bpart = b.take<float>((size_t)p.nbpart * p.Cout);
    p.wg = take_wg(b, p.RO, p.Cout, p.Cin, 16, false);
  }
  p.bytes = b.off + 256;
  return p;
}

bool mult64(int c) { return c >= 64 && c <= 4096 && c % 64 == 0; }

int check_shape(const node_bndownconv_shape* sh) {
  if (!sh) return fail(NODE_ERR_NULL, "shape is NULL");
  if (sh->n <= 0 || sh->cin <= 0 || sh->cout <= 0 || sh->h <= 0 || sh->w <= 0) return fail(NODE_ERR_SHAPE, "bad hand-off shape");
  if (sh->h < 4 || sh->w < 4) return fail(NODE_ERR_SHAPE, "bad hand-off shape: a 4x4 stride-2 convolution takes images of 4x4 pixels and more");
  if (sh->slices < 1 || sh->n % sh->slices != 0)
    return fail(NODE_ERR_SHAPE, "bad hand-off shape: n = %d samples are not %d slices of equal size", sh->n, sh->slices);
  if (!mult64(sh->cin) || !mult64(sh->cout))
    return fail(NODE_ERR_UNSUPPORTED, "the batch-norm hand-off takes filters (cin, cout) that are multiples of 64 in [64, 4096]: 64-column "
                 "GEMM tiles, 64-channel BatchNorm blocks (got %d -> %d)", sh->cin, sh->cout);
  const size_t big = (size_t)sh->n * sh->h * sh->w * (sh->cin > sh->cout ? sh->cin : sh->cout);
  if (big + 4096 >= ((size_t)1 << 31)) return fail(NODE_ERR_UNSUPPORTED, "hand-off tensors must stay under 2^31 elements");
  return NODE_OK;
}

int sliced_is_forward_only(const node_bndownconv_shape* sh) {
  return fail(NODE_ERR_UNSUPPORTED, "the sliced batch-norm hand-off (slices = %d) is the forward without a backward to come: "
               "keep_for_backward = 0 only (with gradients, make one slices = 1 call per slice)", sh->slices);
}

int check_ptr(const void* p, const char* what, bool required) {
  if (!p) return required ? fail(NODE_ERR_NULL, "%s is NULL", what) : NODE_OK;
  if (((uintptr_t)p) & 15) return fail(NODE_ERR_ARG, "%s must be 16-byte aligned", what);
  return NODE_OK;
}

// node_downconv_params / node_downconv_grads: four non-NULL, 16-byte aligned pointers
int check_tensors(const void* s, const char* what) {
  if (!s) return fail(NODE_ERR_NULL, "%s is NULL", what);
  const void* const* pp = reinterpret_cast<const void* const*>(s);
  for (int i = 0; i < 4; ++i) {
    if (!pp[i]) return fail(NODE_ERR_NULL, "tensor %d of %s is NULL", i, what);
    if (((uintptr_t)pp[i]) & 15) return fail(NODE_ERR_ARG, "tensor %d of %s must be 16-byte aligned", i, what);
  }
  return NODE_OK;
}

SBnArgs bn_args(const BnDownPlan& p, const node_downconv_params* prm) {
  SBnArgs a;
  memset(&a, 0, sizeof(a));
  a.h = p.xh; a.gamma = prm->gn_w; a.beta = prm->gn_b; a.stats = p.stats;
  a.rows = p.R; a.C = p.Cin; a.H = p.H; a.W = p.W; a.chunk_rows = p.cr; a.nchunk = p.nchunk; a.relu = 1; a.eps = p.eps;
  a.out_scale = 1.0f; a.da_scale = 1.0f;
  a.slices = p.slices; a.rows_per_slice = p.rps; a.chunks_per_slice = p.cps;
  return a;
}

#define LAUNCHED(what)                                  \
  do {                                                  \
    if ((rc = launch_ok(what)) != NODE_OK) return rc;   \
  } while (0)

}  // namespace

extern "C" {

size_t node_bndownconv_workspace_bytes(const node_bndownconv_shape* shape, int keep_for_backward) {
  if (check_shape(shape) != NODE_OK) return 0;
  if (keep_for_backward && shape->slices > 1) {
    sliced_is_forward_only(shape);
    return 0;
  }
  return make_plan(shape, keep_for_backward != 0, nullptr).bytes;
}

int node_bndownconv_describe(const node_bndownconv_shape* shape, node_bnfunc_info* out) {
  if (!out) return fail(NODE_ERR_NULL, "out is NULL");
  memset(out, 0, sizeof(*out));
  const int rc = check_shape(shape);
  if (rc != NODE_OK) return rc;
  const BnDownPlan p = make_plan(shape, true, nullptr);      // (arithmetic only: the weight gradient's split is what slices = 1 runs)
  out->rows = p.R; out->chunk_rows = p.cr; out->nchunk = p.nchunk;
  out->last_chunk_rows = p.rps - (p.cps - 1) * p.cr;
  out->column_tiles = p.Cin >> 6;
  out->wgrad_nsplit = p.wg.nsplit; out->wgrad_rows_per_split = p.wg.rps;
  return NODE_OK;
}

int node_bndownconv_fwd(const node_bndownconv_shape* shape, const node_downconv_params* prm, const float* x, float* y,
                        int keep_for_backward, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_shape(shape);
  if (rc != NODE_OK) return rc;
  if (keep_for_backward && shape->slices > 1) return sliced_is_forward_only(shape);
  if ((rc = check_tensors(prm, "params")) != NODE_OK) return rc;
  if ((rc = check_ptr(x, "x", true)) != NODE_OK || (rc = check_ptr(y, "y", true)) != NODE_OK) return rc;
  if (!ws) return fail(NODE_ERR_NULL, "workspace is NULL");
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const BnDownPlan p = make_plan(shape, keep_for_backward != 0, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "bndownconv workspace too small: %zu < %zu", ws_bytes, p.bytes);
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
  LAUNCHED("stem_prep");
  launch_stem_from_nchw(x, p.xh, nullptr, 0, p.N, p.Cin, p.H * p.W, st);
  LAUNCHED("stem_from_nchw");
  {
    SBnArgs a = bn_args(p, prm);
    a.part = p.part;
    launch_bn_stats(a, st);
    LAUNCHED("bn_stats");
    a.a3 = p.a.p; a.a_plane = p.a.plane;
    launch_bn_apply(a, st);
    LAUNCHED("bn_apply");
  }
  {
    SConvArgs c = conv_fwd_args(p.a, p.f, p.yn, p.N, p.H, p.W, p.OH, p.OW, 4, 2, 1);
    c.bias = prm->conv_b;
    launch_stem_conv(c, st);
    LAUNCHED("stem_conv");
  }
  launch_stem_to_nchw(p.yn, y, p.N, p.Cout, p.OH * p.OW, st);
  return launch_ok("node_bndownconv_fwd");
}

int node_bndownconv_bwd(const node_bndownconv_shape* shape, const node_downconv_params* prm, const float* grad_y,
                        const node_downconv_grads* gr, float* d_x, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_shape(shape);
  if (rc != NODE_OK) return rc;
  if (shape->slices > 1) return sliced_is_forward_only(shape);
  if ((rc = check_tensors(prm, "params")) != NODE_OK) return rc;
  if ((rc = check_ptr(grad_y, "grad_y", true)) != NODE_OK || (rc = check_ptr(d_x, "d_x", true)) != NODE_OK) return rc;
  if (gr && (rc = check_tensors(gr, "grads")) != NODE_OK) return rc;
  if (!ws) return fail(NODE_ERR_NULL, "workspace is NULL");
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const BnDownPlan p = make_plan(shape, true, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "bndownconv workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int HW = p.H * p.W, OHW = p.OH * p.OW;

  launch_stem_from_nchw(grad_y, nullptr, p.g.p, p.g.plane, p.N, p.Cout, OHW, st, gr ? p.bpart : nullptr);
  LAUNCHED("stem_from_nchw");
  if (gr) {
    launch_stem_wgrad(wgrad_args(p.g, nullptr, p.a, p.wg, p.N, p.H, p.W, p.OH, p.OW, p.Cin, p.Cout, 4, 2, 1), st);
    LAUNCHED("stem_wgrad");
  }
  launch_stem_conv(conv_dgrad_args(p.g, p.f, p.da, p.N, p.OH, p.OW, p.H, p.W, 4, 2, 1), st);
  LAUNCHED("stem_conv");
  {
    SBnArgs a = bn_args(p, prm);
    a.da = p.da; a.gpart = p.gpart;
    launch_bn_bwd_stats(a, st);
    LAUNCHED("bn_bwd_stats");
    a.dh = p.dh;
    a.dgamma = gr ? gr->gn_w : nullptr; a.dbeta = gr ? gr->gn_b : nullptr;
    launch_bn_bwd_dx(a, st);
    LAUNCHED("bn_bwd_dx");
  }
  launch_stem_to_nchw(p.dh, d_x, p.N, p.Cin, HW, st);
  LAUNCHED("stem_to_nchw");
  if (!gr) return launch_ok("node_bndownconv_bwd");

  SReduceArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.job[0] = {p.wg.slab, gr->conv_w, nullptr, 0, p.wg.nsplit, p.Cout, p.Cin, 16};
  ra.job[1] = {p.bpart, gr->conv_b, nullptr, 3, p.nbpart, p.Cout, 0, 0};
  ra.njobs = 2;
  launch_stem_reduce(ra, st);
  LAUNCHED("stem_reduce");
  return launch_ok("node_bndownconv_bwd");
}

}  // extern "C"
