// C ABI of the `norm='batch'` dynamics (include/node_hip.h: node_bnfunc_fwd / node_bnfunc_bwd):
//     f(t, x) = norm3(conv2(t, relu(norm2(conv1(t, relu(norm1(x)))))))        model.py:326-348
// with norm = nn.BatchNorm2d(C, track_running_stats=False) (model.py:274) and conv = ConcatConv2d (model.py:313-323), as a
// host-side plan of the BatchNorm passes (kernels_batchnorm.hip) around the stem's gather-GEMM convolutions, data gradients
// and split-K weight gradients (kernels_stem.hip, used as they are).  NHWC inside the workspace, NCHW at the boundary.
//
// forward:   filters' x part -> triples, time tables, zero rows | NCHW -> NHWC | stats, apply (norm1 + ReLU -> triples) |
//            conv1 (+ bias) | stats, apply (norm2 + ReLU -> triples; the time term of conv1 is added as h1 is read) | conv2 |
//            stats, apply (norm3 -> fp32) | NHWC -> NCHW
// backward:  NCHW -> NHWC | norm3': sums, dx (-> triples; class sums of the time channel) | wgrad conv2 | dgrad conv2 |
//            norm2': sums, dx (-> triples; class sums) | wgrad conv1 | dgrad conv1 | norm1': sums, dx (fp32) | NHWC -> NCHW |
//            one reduction launch: slabs -> dW[:, 1:], class sums -> dW[:, 0] and db, d_t
// The gradient of a convolution's bias in front of a BatchNorm is zero identically; what is returned is the computed sum
// (rounding noise around zero), not a literal zero.  Nothing is accumulated with atomics: every sum runs in a fixed order.
//
// The two entry points are preparation + layout launch + evaluation + layout launch; the evaluations themselves (bn_prepare,
// bn_eval_fwd, bn_eval_bwd: NHWC to NHWC, bnfunc.h) are what a whole solve calls per stage without the other three
// (bnsolve_api.hip).
#include "bnfunc.h"
#include <cstring>

namespace node {

BnPlan make_bn_plan(const node_bnfunc_shape* sh, bool keep, void* base, bool boundary) {
  BnPlan p;
  p.N = sh->n; p.C = sh->channels; p.H = sh->h; p.W = sh->w; p.eps = sh->eps;
  p.R = p.N * p.H * p.W;
  p.cr = bn_chunk_rows(p.R, p.C);
  p.nchunk = (p.R + p.cr - 1) / p.cr;
  const int C = p.C;
  const size_t RC = (size_t)p.R * C;
  Bump b(base);
  p.c1 = take_filt(b, C, C, 9);
  p.c2 = take_filt(b, C, C, 9);
  p.T1 = b.take<float>((size_t)9 * C);
  p.T2 = b.take<float>((size_t)9 * C);
  p.xh = boundary ? b.take<float>(RC) : nullptr;
  p.a1 = take_trip(b, p.R, C);
  p.h1 = b.take<float>(RC);
  p.a2 = take_trip(b, p.R, C);
  p.h2 = b.take<float>(RC);
  p.y = (boundary || keep) ? b.take<float>(RC) : nullptr;
  p.part = b.take<float>((size_t)p.nchunk * 2 * C);
  p.stats1 = b.take<float>((size_t)2 * C);
  p.stats2 = b.take<float>((size_t)2 * C);
  p.stats3 = b.take<float>((size_t)2 * C);
  if (keep) {
    p.gf = p.y;                    // the forward's last NHWC tensor is free once it has left as NCHW
    p.da = b.take<float>(RC);
    p.dht = take_trip(b, p.R, C);
    p.gpart = b.take<double>((size_t)p.nchunk * 2 * C);
    p.clsp1 = b.take<float>((size_t)p.nchunk * 9 * C);
    p.clsp2 = b.take<float>((size_t)p.nchunk * 9 * C);
    p.dtp1 = b.take<double>((size_t)p.nchunk * (C / 64));
    p.dtp2 = b.take<double>((size_t)p.nchunk * (C / 64));
    p.w1 = take_wg(b, p.R, C, C, 9, false);
    p.w2 = take_wg(b, p.R, C, C, 9, false);
  }
  p.bytes = b.off + 256;
  return p;
}

int check_bn_shape(const node_bnfunc_shape* sh) {
  if (!sh) return fail(NODE_ERR_NULL, "shape is NULL");
  if (sh->n <= 0 || sh->h <= 0 || sh->w <= 0 || sh->channels <= 0) return fail(NODE_ERR_SHAPE, "bad bnfunc shape");
  const int C = sh->channels;
  if (C < 64 || C % 64 != 0 || C > 4096)
    return fail(NODE_ERR_UNSUPPORTED, "the batch-norm dynamics take channels a multiple of 64 in [64, 4096]: 64-column GEMM tiles, "
                 "64-channel BatchNorm blocks (got %d)", C);
  if (sh->h < 3 || sh->w < 3)
    return fail(NODE_ERR_UNSUPPORTED, "the batch-norm dynamics take images of h, w >= 3: the time channel's nine border classes "
                 "(got %d x %d)", sh->h, sh->w);
  const size_t elems = (size_t)sh->n * sh->h * sh->w * C;
  if (elems + C >= ((size_t)1 << 31)) return fail(NODE_ERR_UNSUPPORTED, "bnfunc tensors must stay under 2^31 elements");
  return NODE_OK;
}

int check_bn_tensors(const void* s, const char* what) {
  if (!s) return fail(NODE_ERR_NULL, "%s is NULL", what);
  const void* const* pp = reinterpret_cast<const void* const*>(s);
  for (int k = 0; k < 10; ++k) {
    if (!pp[k]) return fail(NODE_ERR_NULL, "tensor %d of %s is NULL", k, what);
    if (((uintptr_t)pp[k]) & 15) return fail(NODE_ERR_ARG, "tensor %d of %s must be 16-byte aligned", k, what);
  }
  return NODE_OK;
}
namespace {
SBnArgs bn_args(const BnPlan& p, const float* h, const float* T, const float* t, const float* gamma, const float* beta, float* part,
                float* stats, bool relu) {
  SBnArgs a;
  memset(&a, 0, sizeof(a));
  a.h = h; a.T = T; a.t = t; a.gamma = gamma; a.beta = beta; a.part = part; a.stats = stats;
  a.rows = p.R; a.C = p.C; a.H = p.H; a.W = p.W; a.chunk_rows = p.cr; a.nchunk = p.nchunk; a.relu = relu ? 1 : 0; a.eps = p.eps;
  a.out_scale = 1.0f; a.da_scale = 1.0f;
  return a;
}

#define LAUNCHED(what)                                  \
  do {                                                  \
    if ((rc = launch_ok(what)) != NODE_OK) return rc;   \
  } while (0)

}  // namespace

int bn_prepare(const BnPlan& p, const node_bnfunc_params* prm, bool keep, hipStream_t st) {
  SBnPrepArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.w[0] = prm->conv1_w; pa.wf[0] = p.c1.wf; pa.wd[0] = p.c1.wd; pa.T[0] = p.T1;
  pa.w[1] = prm->conv2_w; pa.wf[1] = p.c2.wf; pa.wd[1] = p.c2.wd; pa.T[1] = p.T2;
  pa.C = p.C;
  const Trip* tz[3] = {&p.a1, &p.a2, &p.dht};
  pa.nzero = keep ? 3 : 2;
  for (int i = 0; i < pa.nzero; ++i) {
    pa.zero[i] = tz[i]->p + (size_t)tz[i]->rows * p.C;
    pa.zero_plane[i] = tz[i]->plane;
  }
  launch_bn_prep(pa, st);
  return launch_ok("bn_prep");
}

int bn_eval_fwd(const BnPlan& p, const node_bnfunc_params* prm, const float* t, const float* x, float* out, float out_scale, hipStream_t st) {
  int rc;
  const int N = p.N, H = p.H, W = p.W;
  {   // a1 = relu(norm1(x))
    SBnArgs a = bn_args(p, x, nullptr, nullptr, prm->norm1_w, prm->norm1_b, p.part, p.stats1, true);
    launch_bn_stats(a, st);
    LAUNCHED("bn_stats");
    a.a3 = p.a1.p; a.a_plane = p.a1.plane;
    launch_bn_apply(a, st);
    LAUNCHED("bn_apply");
  }
  {
    SConvArgs c = conv_fwd_args(p.a1, p.c1, p.h1, N, H, W, H, W, 3, 1, 1);
    c.bias = prm->conv1_b;
    launch_stem_conv(c, st);
    LAUNCHED("stem_conv");
  }
  {   // a2 = relu(norm2(h1 + t T1))
    SBnArgs a = bn_args(p, p.h1, p.T1, t, prm->norm2_w, prm->norm2_b, p.part, p.stats2, true);
    launch_bn_stats(a, st);
    LAUNCHED("bn_stats");
    a.a3 = p.a2.p; a.a_plane = p.a2.plane;
    launch_bn_apply(a, st);
    LAUNCHED("bn_apply");
  }
  {
    SConvArgs c = conv_fwd_args(p.a2, p.c2, p.h2, N, H, W, H, W, 3, 1, 1);
    c.bias = prm->conv2_b;
    launch_stem_conv(c, st);
    LAUNCHED("stem_conv");
  }
  {   // out = out_scale * norm3(h2 + t T2)
    SBnArgs a = bn_args(p, p.h2, p.T2, t, prm->norm3_w, prm->norm3_b, p.part, p.stats3, false);
    launch_bn_stats(a, st);
    LAUNCHED("bn_stats");
    a.y = out; a.out_scale = out_scale;
    launch_bn_apply(a, st);
    LAUNCHED("bn_apply");
  }
  return NODE_OK;
}

int bn_eval_bwd(const BnPlan& p, const node_bnfunc_params* prm, const float* t, const float* x, const float* da, float da_scale,
                const node_bnfunc_grads* grads, float* dx, bool want_dx, float* d_t, hipStream_t st) {
  int rc;
  const int N = p.N, C = p.C, H = p.H, W = p.W;
  const bool want_p = grads != nullptr, want_time = want_p || d_t != nullptr;
  {   // norm3: du2 -> triples
    SBnArgs a = bn_args(p, p.h2, p.T2, t, prm->norm3_w, prm->norm3_b, nullptr, p.stats3, false);
    a.da = da; a.da_scale = da_scale; a.gpart = p.gpart;
    launch_bn_bwd_stats(a, st);
    LAUNCHED("bn_bwd_stats");
    a.dh3 = p.dht.p; a.dh_plane = p.dht.plane;
    if (want_p) { a.dgamma = grads->norm3_w; a.dbeta = grads->norm3_b; }
    if (want_time) { a.clsp = p.clsp2; a.dtp = p.dtp2; }
    launch_bn_bwd_dx(a, st);
    LAUNCHED("bn_bwd_dx");
  }
  if (want_p) {
    launch_stem_wgrad(wgrad_args(p.dht, nullptr, p.a2, p.w2, N, H, W, H, W, C, C, 3, 1, 1), st);
    LAUNCHED("stem_wgrad");
  }
  launch_stem_conv(conv_dgrad_args(p.dht, p.c2, p.da, N, H, W, H, W, 3, 1, 1), st);
  LAUNCHED("stem_conv");
  {   // norm2 + ReLU: du1 -> triples
    SBnArgs a = bn_args(p, p.h1, p.T1, t, prm->norm2_w, prm->norm2_b, nullptr, p.stats2, true);
    a.da = p.da; a.gpart = p.gpart;
    launch_bn_bwd_stats(a, st);
    LAUNCHED("bn_bwd_stats");
    a.dh3 = p.dht.p; a.dh_plane = p.dht.plane;
    if (want_p) { a.dgamma = grads->norm2_w; a.dbeta = grads->norm2_b; }
    if (want_time) { a.clsp = p.clsp1; a.dtp = p.dtp1; }
    launch_bn_bwd_dx(a, st);
    LAUNCHED("bn_bwd_dx");
  }
  if (want_p) {
    launch_stem_wgrad(wgrad_args(p.dht, nullptr, p.a1, p.w1, N, H, W, H, W, C, C, 3, 1, 1), st);
    LAUNCHED("stem_wgrad");
  }
  if (want_p || want_dx) {
    launch_stem_conv(conv_dgrad_args(p.dht, p.c1, p.da, N, H, W, H, W, 3, 1, 1), st);
    LAUNCHED("stem_conv");
    // norm1 + ReLU: dx (fp32)
    SBnArgs a = bn_args(p, x, nullptr, nullptr, prm->norm1_w, prm->norm1_b, nullptr, p.stats1, true);
    a.da = p.da; a.gpart = p.gpart;
    launch_bn_bwd_stats(a, st);
    LAUNCHED("bn_bwd_stats");
    a.dh = dx;
    if (want_p) { a.dgamma = grads->norm1_w; a.dbeta = grads->norm1_b; }
    launch_bn_bwd_dx(a, st);
    LAUNCHED("bn_bwd_dx");
  }
  if (want_time) {
    SBnReduceArgs r;
    memset(&r, 0, sizeof(r));
    r.slab0 = p.w1.slab; r.slab1 = p.w2.slab; r.ns0 = p.w1.nsplit; r.ns1 = p.w2.nsplit;
    if (want_p) { r.dw0 = grads->conv1_w; r.dw1 = grads->conv2_w; r.db0 = grads->conv1_b; r.db1 = grads->conv2_b; }
    r.clsp0 = p.clsp1; r.clsp1 = p.clsp2; r.dtp0 = p.dtp1; r.dtp1 = p.dtp2;
    r.nchunk = p.nchunk; r.C = C; r.t = t; r.d_t = d_t; r.want_params = want_p ? 1 : 0;
    launch_bn_reduce(r, st);
    LAUNCHED("bn_reduce");
  }
  return NODE_OK;
}

}  // namespace node

using namespace node;

namespace {
int check_ptr(const void* p, const char* what, bool required) {
  if (!p) return required ? fail(NODE_ERR_NULL, "%s is NULL", what) : NODE_OK;
  if (((uintptr_t)p) & 15) return fail(NODE_ERR_ARG, "%s must be 16-byte aligned", what);
  return NODE_OK;
}

}  // namespace

extern "C" {

size_t node_bnfunc_workspace_bytes(const node_bnfunc_shape* shape, int keep_for_backward) {
  if (check_bn_shape(shape) != NODE_OK) return 0;
  return make_bn_plan(shape, keep_for_backward != 0, nullptr).bytes;
}

int node_bnfunc_describe(const node_bnfunc_shape* shape, node_bnfunc_info* out) {
  if (!out) return fail(NODE_ERR_NULL, "out is NULL");
  memset(out, 0, sizeof(*out));
  const int rc = check_bn_shape(shape);
  if (rc != NODE_OK) return rc;
  const BnPlan p = make_bn_plan(shape, true, nullptr);      // the backward's plan: the same chunks as the forward's, plus the two weight gradients
  out->rows = p.R; out->chunk_rows = p.cr; out->nchunk = p.nchunk;
  out->last_chunk_rows = p.R - (p.nchunk - 1) * p.cr;
  out->column_tiles = p.C >> 6;
  out->wgrad_nsplit = p.w1.nsplit; out->wgrad_rows_per_split = p.w1.rps;      // (w2 is taken with the same arguments)
  return NODE_OK;
}

int node_bnfunc_fwd(const node_bnfunc_shape* shape, const node_bnfunc_params* prm, const float* t, const float* x, float* out,
                    int keep_for_backward, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_bn_shape(shape);
  if (rc != NODE_OK) return rc;
  if ((rc = check_bn_tensors(prm, "params")) != NODE_OK) return rc;
  if (!t) return fail(NODE_ERR_NULL, "t is NULL (a device scalar)");
  if (((uintptr_t)t) & 3) return fail(NODE_ERR_ARG, "t must be 4-byte aligned");
  if ((rc = check_ptr(x, "x", true)) != NODE_OK || (rc = check_ptr(out, "out", true)) != NODE_OK) return rc;
  if (!ws) return fail(NODE_ERR_NULL, "workspace is NULL");
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const BnPlan p = make_bn_plan(shape, keep_for_backward != 0, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "bnfunc workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int N = p.N, C = p.C, HW = p.H * p.W;

  if ((rc = bn_prepare(p, prm, keep_for_backward != 0, st)) != NODE_OK) return rc;
  launch_stem_from_nchw(x, p.xh, nullptr, 0, N, C, HW, st);
  LAUNCHED("stem_from_nchw");
  // (the output gradient's NHWC copy of the backward goes where this forward's NHWC output was: p.gf = p.y)
  if ((rc = bn_eval_fwd(p, prm, t, p.xh, p.y, 1.0f, st)) != NODE_OK) return rc;
  launch_stem_to_nchw(p.y, out, N, C, HW, st);
  return launch_ok("node_bnfunc_fwd");
}

int node_bnfunc_bwd(const node_bnfunc_shape* shape, const node_bnfunc_params* prm, const float* t, const float* grad_out,
                    const node_bnfunc_grads* grads, float* d_x, float* d_t, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_bn_shape(shape);
  if (rc != NODE_OK) return rc;
  if ((rc = check_bn_tensors(prm, "params")) != NODE_OK) return rc;
  if (grads && (rc = check_bn_tensors(grads, "grads")) != NODE_OK) return rc;
  if (!t) return fail(NODE_ERR_NULL, "t is NULL (a device scalar)");
  if ((((uintptr_t)t) & 3) || (((uintptr_t)d_t) & 3)) return fail(NODE_ERR_ARG, "t and d_t must be 4-byte aligned");
  if ((rc = check_ptr(grad_out, "grad_out", true)) != NODE_OK || (rc = check_ptr(d_x, "d_x", false)) != NODE_OK) return rc;
  if (!ws) return fail(NODE_ERR_NULL, "workspace is NULL");
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const BnPlan p = make_bn_plan(shape, true, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "bnfunc workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int N = p.N, C = p.C, HW = p.H * p.W;

  launch_stem_from_nchw(grad_out, p.gf, nullptr, 0, N, C, HW, st);
  LAUNCHED("stem_from_nchw");
  // norm1's dx goes over the output gradient's NHWC copy, which nothing reads any more by then
  if ((rc = bn_eval_bwd(p, prm, t, p.xh, p.gf, 1.0f, grads, p.gf, d_x != nullptr, d_t, st)) != NODE_OK) return rc;
  if (d_x) {
    launch_stem_to_nchw(p.gf, d_x, N, C, HW, st);
    LAUNCHED("stem_to_nchw");
  }
  return NODE_OK;
}

}  // extern "C"
