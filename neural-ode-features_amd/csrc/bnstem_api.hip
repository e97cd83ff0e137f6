// C ABI of the residual stem with norm = 'batch' (include/node_hip.h: node_bnstem_fwd / node_bnstem_bwd): ResDownsample,
// model.py:167-178, of ResBlocks (model.py:284-310) whose norms are model.py:274 (nn.BatchNorm2d(C, track_running_stats=False)) --
// as a host-side plan.  It is stem_api.hip's plan with the other norm: the BatchNorm passes of kernels_batchnorm.hip (two-stage
// statistics, Chan's formula, fp64 backward partials; T = nullptr, relu = 1, scales 1.0f: there is no time channel here, and no
// skip variant either -- the shortcut of these blocks reads relu(norm1(x)), so no norm's input has a second consumer) around the
// stem's first-layer kernels, gather-GEMM convolutions, data gradients and split-K weight gradients (kernels_stem.hip, used as
// they are).  NHWC inside the workspace, NCHW at the boundary.
//
// forward (14 launches):  prep (six filters, conv0's filter, the zero rows) | conv0 | stats, apply (norm1 + ReLU -> triples) |
//                         conv 3x3/2 with the 1x1/2 shortcut in the same launch | stats, apply | conv 3x3 (+ shortcut) |
//                         the same seven for block 2 | NHWC -> NCHW
// backward: NCHW -> triples | per convolution: weight gradient (the shortcut's rides in the 3x3/2's launch), data gradient (the
//           shortcut's one more K segment) | per BatchNorm: sums, dx (-> triples; the first norm's -> fp32 dh0) | [d_x] the
//           transposed first layer | [grads] conv0's weight gradient, ONE reduction launch for the seven slab jobs
// dgamma / dbeta leave the dx passes directly (their chunk-0 workgroups), as in bnfunc_api.hip: the reduction launch carries no
// norm jobs.  Nothing is accumulated with atomics: every sum runs in a fixed order.
//
// The last convolution (filters -> filters at the last resolution) stays on the gather GEMM: the F(4x4,3x3) route the GroupNorm
// stem takes at 8 x 8 has GroupNorm inside its passes, so NODE_TUNE_STEM_W4 has no effect on this node.
//
// Chunks of the BatchNorm passes: bnstem_chunk_rows below, this node's own policy (bn_chunk_rows, which the dynamics, the solves and
// the trunk plan with, is not touched).  Its cap on the chunks of a 64-channel tensor is NODE_TUNE_BNSTEM_MAXCHUNK, read once per
// call; unset or 0: the built-in default, 128, at which it IS bn_chunk_rows.
#include "bnfunc.h"
#include <cstring>

using namespace node;

namespace node {

constexpr int BNSTEM_MAXCHUNK_DEFAULT = 128;

// the cap in force: NODE_TUNE_BNSTEM_MAXCHUNK, read again by every plan (so once per call, like NODE_TUNE_STEM_W4); unset or 0: the default
static int bnstem_cap() {
  int cap = env_int("NODE_TUNE_BNSTEM_MAXCHUNK", 0);
  if (cap <= 0) cap = BNSTEM_MAXCHUNK_DEFAULT;
  if (cap < 16) cap = 16;
  return cap > 65536 ? 65536 : cap;
}

// rows per chunk for a stem tensor of `rows` x C: at most `cap` chunks at C = 64, 2 cap / (C / 64) for wider tensors (never under
// 16), whole 32-row trips.  cap = 128: bn_chunk_rows.
int bnstem_chunk_rows(int rows, int C) {
  const int cap = bnstem_cap();
  int maxchunk = 2 * cap / (C >> 6);
  if (maxchunk > cap) maxchunk = cap;
  if (maxchunk < 16) maxchunk = 16;
  int cr = (rows + maxchunk - 1) / maxchunk;
  cr = (cr + 31) & ~31;
  return cr < 32 ? 32 : cr;
}

}  // namespace node

namespace {

inline int down2(int h) { return (h - 1) / 2 + 1; }     // 3x3 stride 2 pad 1 and 1x1 stride 2 pad 0 alike

struct Norm {                     // one BatchNorm of the plan: its input tensor's geometry and chunks
  int rows, C, H, W, cr, nchunk;
  float* stats;
};
struct BnStemPlan {
  int N, Cin0, H, W, F;
  int H0, W0, H1, W1, H2, W2, R0, R1, R2;
  float eps;
  bool keep;
  float* w0t;
  Filt c1, c2, d1, c3, c4, d2;
  float *h0, *h1, *s1, *x1, *h3, *s2, *outn;
  Trip a0, a1, a2, a3;
  Norm n[4];                      // of h0, h1, x1, h3
  float* part;                    // forward partials of the pass in flight
  // backward
  Trip g3, dh3t, dx1t, dh1t;
  float *da, *dh0;                // da: the data gradient in front of the norm in flight (the largest of the four)
  double* gpart;
  Wg w4, w3, w2, w1, w0;
  size_t bytes;
};

// keep = false (the no-grad forward): tensors whose lives do not overlap share storage -- x1 lies on h1, the triples of block 2's
// first activation on those of block 1's second (the same shape, so the same zero row), the four statistics on one
BnStemPlan make_plan(const node_stem_shape* sh, bool keep, void* base) {
  BnStemPlan p;
  memset(&p, 0, sizeof(p));
  p.N = sh->n; p.Cin0 = sh->in_ch; p.H = sh->h; p.W = sh->w; p.F = sh->filters; p.eps = sh->eps; p.keep = keep;
  p.H0 = p.H - 2; p.W0 = p.W - 2;
  p.H1 = down2(p.H0); p.W1 = down2(p.W0);
  p.H2 = down2(p.H1); p.W2 = down2(p.W1);
  p.R0 = p.N * p.H0 * p.W0; p.R1 = p.N * p.H1 * p.W1; p.R2 = p.N * p.H2 * p.W2;
  const int F = p.F;
  p.n[0] = {p.R0, 64, p.H0, p.W0, 0, 0, nullptr};
  p.n[1] = {p.R1, 64, p.H1, p.W1, 0, 0, nullptr};
  p.n[2] = {p.R1, 64, p.H1, p.W1, 0, 0, nullptr};
  p.n[3] = {p.R2, F, p.H2, p.W2, 0, 0, nullptr};
  size_t npart = 0;
  for (Norm& k : p.n) {
    k.cr = bnstem_chunk_rows(k.rows, k.C);
    k.nchunk = (k.rows + k.cr - 1) / k.cr;
    const size_t need = (size_t)k.nchunk * 2 * k.C;
    if (need > npart) npart = need;
  }
  Bump b(base);
  p.w0t = b.take<float>(28 * 64);
  p.c1 = take_filt(b, 64, 64, 9);
  p.c2 = take_filt(b, 64, 64, 9);
  p.d1 = take_filt(b, 64, 64, 1);
  p.c3 = take_filt(b, F, 64, 9);
  p.c4 = take_filt(b, F, F, 9);
  p.d2 = take_filt(b, F, 64, 1);
  p.h0 = b.take<float>((size_t)p.R0 * 64);
  p.a0 = take_trip(b, p.R0, 64);
  p.h1 = b.take<float>((size_t)p.R1 * 64);
  p.s1 = b.take<float>((size_t)p.R1 * 64);
  p.a1 = take_trip(b, p.R1, 64);
  p.x1 = keep ? b.take<float>((size_t)p.R1 * 64) : p.h1;
  p.a2 = keep ? take_trip(b, p.R1, 64) : p.a1;
  p.h3 = b.take<float>((size_t)p.R2 * F);
  p.s2 = b.take<float>((size_t)p.R2 * F);
  p.a3 = take_trip(b, p.R2, F);
  p.outn = b.take<float>((size_t)p.R2 * F);
  p.n[0].stats = b.take<float>((size_t)2 * (F > 64 ? F : 64));
  for (int i = 1; i < 4; ++i) p.n[i].stats = keep ? b.take<float>((size_t)2 * p.n[i].C) : p.n[0].stats;
  p.part = b.take<float>(npart);
  if (keep) {
    p.g3 = take_trip(b, p.R2, F);
    p.dh3t = take_trip(b, p.R2, F);
    p.dx1t = take_trip(b, p.R1, 64);
    p.dh1t = take_trip(b, p.R1, 64);
    const size_t e0 = (size_t)p.R0 * 64, e3 = (size_t)p.R2 * F;
    p.da = b.take<float>(e0 > e3 ? e0 : e3);
    p.dh0 = b.take<float>(e0);
    p.gpart = b.take<double>(npart);
    p.w4 = take_wg(b, p.R2, F, F, 9, false);
    p.w3 = take_wg(b, p.R2, F, 64, 9, true);
    p.w2 = take_wg(b, p.R1, 64, 64, 9, false);
    p.w1 = take_wg(b, p.R1, 64, 64, 9, true);
    {   // conv0: K steps of two pixels over R0 rows, one 64 x 32 slab per workgroup (stem_api.hip's plan)
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

int check_shape(const node_stem_shape* sh) {
  if (!sh) return fail(NODE_ERR_NULL, "shape is NULL");
  if (sh->n <= 0 || sh->in_ch <= 0 || sh->h < 5 || sh->w < 5 || sh->filters <= 0) return fail(NODE_ERR_SHAPE, "bad stem shape");
  if (sh->in_ch > 3) return fail(NODE_ERR_UNSUPPORTED, "the stem's first layer takes in_ch <= 3 (got %d)", sh->in_ch);
  const int F = sh->filters;
  if (F < 64 || F % 64 != 0 || F > 4096)
    return fail(NODE_ERR_UNSUPPORTED, "the batch-norm stem takes filters a multiple of 64 in [64, 4096]: 64-column GEMM tiles, "
                 "64-channel BatchNorm blocks (got %d)", F);
  const int h0 = sh->h - 2, w0 = sh->w - 2, h2 = down2(down2(h0)), w2 = down2(down2(w0));
  if ((long long)h0 * w0 > 2400)
    return fail(NODE_ERR_UNSUPPORTED, "the stem's first-layer kernels have run on images of up to 2400 pixels behind the first "
                 "layer (got %d x %d)", h0, w0);
  const size_t e0 = (size_t)sh->n * h0 * w0 * 64, e3 = (size_t)sh->n * h2 * w2 * F;
  if (e0 + 64 >= ((size_t)1 << 31) || e3 + F >= ((size_t)1 << 31) || (size_t)sh->n * sh->in_ch * sh->h * sh->w >= ((size_t)1 << 31))
    return fail(NODE_ERR_UNSUPPORTED, "stem tensors must stay under 2^31 elements");
  if ((long long)sh->n * h2 * w2 <= 1)
    return fail(NODE_ERR_UNSUPPORTED, "the last BatchNorm needs more than one value per channel (n h2 w2 = %lld)", (long long)sh->n * h2 * w2);
  return NODE_OK;
}

int check_ptr(const void* p, const char* what, bool required) {
  if (!p) return required ? fail(NODE_ERR_NULL, "%s is NULL", what) : NODE_OK;
  if (((uintptr_t)p) & 15) return fail(NODE_ERR_ARG, "%s must be 16-byte aligned", what);
  return NODE_OK;
}

// node_stem_params / node_stem_grads: sixteen non-NULL, 16-byte aligned pointers
int check_tensors(const void* s, const char* what) {
  if (!s) return fail(NODE_ERR_NULL, "%s is NULL", what);
  const void* const* pp = reinterpret_cast<const void* const*>(s);
  for (int i = 0; i < 16; ++i) {
    if (!pp[i]) return fail(NODE_ERR_NULL, "tensor %d of %s is NULL", i, what);
    if (((uintptr_t)pp[i]) & 15) return fail(NODE_ERR_ARG, "tensor %d of %s must be 16-byte aligned", i, what);
  }
  return NODE_OK;
}

SBnArgs bn_args(const BnStemPlan& p, const Norm& k, const float* h, const float* gamma, const float* beta) {
  SBnArgs a;
  memset(&a, 0, sizeof(a));
  a.h = h; a.gamma = gamma; a.beta = beta; a.stats = k.stats;
  a.rows = k.rows; a.C = k.C; a.H = k.H; a.W = k.W; a.chunk_rows = k.cr; a.nchunk = k.nchunk; a.relu = 1; a.eps = p.eps;
  a.out_scale = 1.0f; a.da_scale = 1.0f;
  return a;
}

#define LAUNCHED(what)                                  \
  do {                                                  \
    if ((rc = launch_ok(what)) != NODE_OK) return rc;   \
  } while (0)

// a3 = relu(norm(h)) as triples; leaves the batch statistics in the norm's `stats`
int norm_relu(const BnStemPlan& p, const Norm& k, const float* h, const float* gamma, const float* beta, const Trip& a3, hipStream_t st) {
  int rc;
  SBnArgs a = bn_args(p, k, h, gamma, beta);
  a.part = p.part;
  launch_bn_stats(a, st);
  LAUNCHED("bn_stats");
  a.a3 = a3.p; a.a_plane = a3.plane;
  launch_bn_apply(a, st);
  LAUNCHED("bn_apply");
  return NODE_OK;
}

// the gradient of the norm's input from p.da: as triples (dh3) or fp32 (dh); dgamma / dbeta nullable
int norm_relu_bwd(const BnStemPlan& p, const Norm& k, const float* h, const float* gamma, const float* beta, const Trip* dh3, float* dh,
                  float* dgamma, float* dbeta, hipStream_t st) {
  int rc;
  SBnArgs a = bn_args(p, k, h, gamma, beta);
  a.da = p.da; a.gpart = p.gpart;
  launch_bn_bwd_stats(a, st);
  LAUNCHED("bn_bwd_stats");
  if (dh3) { a.dh3 = dh3->p; a.dh_plane = dh3->plane; }
  a.dh = dh;
  a.dgamma = dgamma; a.dbeta = dbeta;
  launch_bn_bwd_dx(a, st);
  LAUNCHED("bn_bwd_dx");
  return NODE_OK;
}

}  // namespace

extern "C" {

size_t node_bnstem_workspace_bytes(const node_stem_shape* shape, int keep_for_backward) {
  if (check_shape(shape) != NODE_OK) return 0;
  return make_plan(shape, keep_for_backward != 0, nullptr).bytes;
}

int node_bnstem_describe(const node_stem_shape* shape, node_bnfunc_info out[4]) {
  if (!out) return fail(NODE_ERR_NULL, "out is NULL");
  memset(out, 0, 4 * sizeof(*out));
  const int rc = check_shape(shape);
  if (rc != NODE_OK) return rc;
  const BnStemPlan p = make_plan(shape, true, nullptr);
  const Wg* reader[4] = {&p.w1, &p.w2, &p.w3, &p.w4};      // the weight gradient of the convolution that reads the norm's output
  for (int i = 0; i < 4; ++i) {
    const Norm& k = p.n[i];
    out[i].rows = k.rows; out[i].chunk_rows = k.cr; out[i].nchunk = k.nchunk;
    out[i].last_chunk_rows = k.rows - (k.nchunk - 1) * k.cr;
    out[i].column_tiles = k.C >> 6;
    out[i].wgrad_nsplit = reader[i]->nsplit; out[i].wgrad_rows_per_split = reader[i]->rps;
  }
  return NODE_OK;
}

int node_bnstem_fwd(const node_stem_shape* shape, const node_stem_params* prm, const float* x, float* out, int keep_for_backward,
                    void* ws, size_t ws_bytes, void* stream) {
  int rc = check_shape(shape);
  if (rc != NODE_OK) return rc;
  if ((rc = check_tensors(prm, "params")) != NODE_OK) return rc;
  if ((rc = check_ptr(x, "x", true)) != NODE_OK || (rc = check_ptr(out, "out", true)) != NODE_OK) return rc;
  if (!ws) return fail(NODE_ERR_NULL, "workspace is NULL");
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const BnStemPlan p = make_plan(shape, keep_for_backward != 0, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "bnstem workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int N = p.N;

  SPrepArgs pa;
  memset(&pa, 0, sizeof(pa));
  const Filt* fl[6] = {&p.c1, &p.c2, &p.d1, &p.c3, &p.c4, &p.d2};
  const float* fw[6] = {prm->b1_c1_w, prm->b1_c2_w, prm->b1_ds_w, prm->b2_c1_w, prm->b2_c2_w, prm->b2_ds_w};
  for (int i = 0; i < 6; ++i) pa.job[i] = {fw[i], fl[i]->wf, fl[i]->wd, fl[i]->Cout, fl[i]->Cin, fl[i]->taps};
  pa.njobs = 6;
  pa.w0 = prm->conv0_w; pa.w0t = p.w0t; pa.k0 = 9 * p.Cin0;
  const Trip* tz[8] = {&p.a0, &p.a1, &p.a3, &p.a2, &p.g3, &p.dh3t, &p.dx1t, &p.dh1t};     // (keep = 0: the first three are all there is)
  const int nz = p.keep ? 8 : 3;
  for (int i = 0; i < nz; ++i) {
    pa.zero[i] = tz[i]->p + (size_t)tz[i]->rows * tz[i]->C;
    pa.zero_plane[i] = tz[i]->plane;
    pa.zero_c[i] = tz[i]->C;
  }
  pa.nzero = nz;
  launch_stem_prep(pa, st);
  LAUNCHED("stem_prep");

  launch_stem_conv0_fwd(x, p.w0t, prm->conv0_b, p.h0, N, p.Cin0, p.H, p.W, st);
  LAUNCHED("stem_conv0_fwd");
  // block 1: a0 = relu(norm1(h0)); h1 = conv1(a0) (3x3 / 2), s1 = shortcut(a0) (1x1 / 2) in one launch
  if ((rc = norm_relu(p, p.n[0], p.h0, prm->b1_n1_w, prm->b1_n1_b, p.a0, st)) != NODE_OK) return rc;
  {
    SConvArgs c = conv_fwd_args(p.a0, p.c1, p.h1, N, p.H0, p.W0, p.H1, p.W1, 3, 2, 1);
    c.w2 = p.d1.wf; c.w2_plane = p.d1.plane; c.out2 = p.s1;
    launch_stem_conv(c, st);
    LAUNCHED("stem_conv");
  }
  if ((rc = norm_relu(p, p.n[1], p.h1, prm->b1_n2_w, prm->b1_n2_b, p.a1, st)) != NODE_OK) return rc;
  {   // x1 = conv2(a1) + s1
    SConvArgs c = conv_fwd_args(p.a1, p.c2, p.x1, N, p.H1, p.W1, p.H1, p.W1, 3, 1, 1);
    c.res = p.s1;
    launch_stem_conv(c, st);
    LAUNCHED("stem_conv");
  }
  // block 2
  if ((rc = norm_relu(p, p.n[2], p.x1, prm->b2_n1_w, prm->b2_n1_b, p.a2, st)) != NODE_OK) return rc;
  {
    SConvArgs c = conv_fwd_args(p.a2, p.c3, p.h3, N, p.H1, p.W1, p.H2, p.W2, 3, 2, 1);
    c.w2 = p.d2.wf; c.w2_plane = p.d2.plane; c.out2 = p.s2;
    launch_stem_conv(c, st);
    LAUNCHED("stem_conv");
  }
  if ((rc = norm_relu(p, p.n[3], p.h3, prm->b2_n2_w, prm->b2_n2_b, p.a3, st)) != NODE_OK) return rc;
  {
    SConvArgs c = conv_fwd_args(p.a3, p.c4, p.outn, N, p.H2, p.W2, p.H2, p.W2, 3, 1, 1);
    c.res = p.s2;
    launch_stem_conv(c, st);
    LAUNCHED("stem_conv");
  }
  launch_stem_to_nchw(p.outn, out, N, p.F, p.H2 * p.W2, st);
  return launch_ok("node_bnstem_fwd");
}

int node_bnstem_bwd(const node_stem_shape* shape, const node_stem_params* prm, const float* x, const float* grad_out,
                    const node_stem_grads* gr, float* d_x, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_shape(shape);
  if (rc != NODE_OK) return rc;
  if ((rc = check_tensors(prm, "params")) != NODE_OK) return rc;
  if ((rc = check_ptr(x, "x", true)) != NODE_OK || (rc = check_ptr(grad_out, "grad_out", true)) != NODE_OK) return rc;
  if (!gr && !d_x) return fail(NODE_ERR_NULL, "neither grads nor d_x is given: nothing to compute");
  if (gr && (rc = check_tensors(gr, "grads")) != NODE_OK) return rc;
  if ((rc = check_ptr(d_x, "d_x", false)) != NODE_OK) return rc;
  if (!ws) return fail(NODE_ERR_NULL, "workspace is NULL");
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const BnStemPlan p = make_plan(shape, true, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "bnstem workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int N = p.N, F = p.F;

  // dL/d out: also the gradient of the second block's shortcut s2
  launch_stem_from_nchw(grad_out, nullptr, p.g3.p, p.g3.plane, N, F, p.H2 * p.W2, st);
  LAUNCHED("stem_from_nchw");
  // block 2, conv2 (3x3, F -> F): weight gradient, data gradient -> da
  if (gr) {
    launch_stem_wgrad(wgrad_args(p.g3, nullptr, p.a3, p.w4, N, p.H2, p.W2, p.H2, p.W2, F, F, 3, 1, 1), st);
    LAUNCHED("stem_wgrad");
  }
  launch_stem_conv(conv_dgrad_args(p.g3, p.c4, p.da, N, p.H2, p.W2, p.H2, p.W2, 3, 1, 1), st);
  LAUNCHED("stem_conv");
  if ((rc = norm_relu_bwd(p, p.n[3], p.h3, prm->b2_n2_w, prm->b2_n2_b, &p.dh3t, nullptr, gr ? gr->b2_n2_w : nullptr,
                          gr ? gr->b2_n2_b : nullptr, st)) != NODE_OK)
    return rc;
  // block 2, conv1 (3x3 / 2, 64 -> F) + shortcut (1x1 / 2, 64 -> F): both read a2
  if (gr) {
    launch_stem_wgrad(wgrad_args(p.dh3t, &p.g3, p.a2, p.w3, N, p.H1, p.W1, p.H2, p.W2, 64, F, 3, 2, 1), st);
    LAUNCHED("stem_wgrad");
  }
  {   // data gradient of conv1 (3x3 / 2) + the shortcut's (1x1 / 2: one more K segment of the (even, even) pixels)
    SConvArgs c = conv_dgrad_args(p.dh3t, p.c3, p.da, N, p.H2, p.W2, p.H1, p.W1, 3, 2, 1);
    c.in2 = p.g3.p; c.w2 = p.d2.wd; c.w2_plane = p.d2.plane;
    launch_stem_conv(c, st);
    LAUNCHED("stem_conv");
  }
  if ((rc = norm_relu_bwd(p, p.n[2], p.x1, prm->b2_n1_w, prm->b2_n1_b, &p.dx1t, nullptr, gr ? gr->b2_n1_w : nullptr,
                          gr ? gr->b2_n1_b : nullptr, st)) != NODE_OK)
    return rc;
  // block 1, conv2 (3x3, 64 -> 64): dx1 is the gradient of its output AND of the shortcut s1
  if (gr) {
    launch_stem_wgrad(wgrad_args(p.dx1t, nullptr, p.a1, p.w2, N, p.H1, p.W1, p.H1, p.W1, 64, 64, 3, 1, 1), st);
    LAUNCHED("stem_wgrad");
  }
  launch_stem_conv(conv_dgrad_args(p.dx1t, p.c2, p.da, N, p.H1, p.W1, p.H1, p.W1, 3, 1, 1), st);
  LAUNCHED("stem_conv");
  if ((rc = norm_relu_bwd(p, p.n[1], p.h1, prm->b1_n2_w, prm->b1_n2_b, &p.dh1t, nullptr, gr ? gr->b1_n2_w : nullptr,
                          gr ? gr->b1_n2_b : nullptr, st)) != NODE_OK)
    return rc;
  // block 1, conv1 (3x3 / 2) + shortcut (1x1 / 2): both read a0
  if (gr) {
    launch_stem_wgrad(wgrad_args(p.dh1t, &p.dx1t, p.a0, p.w1, N, p.H0, p.W0, p.H1, p.W1, 64, 64, 3, 2, 1), st);
    LAUNCHED("stem_wgrad");
  }
  {
    SConvArgs c = conv_dgrad_args(p.dh1t, p.c1, p.da, N, p.H1, p.W1, p.H0, p.W0, 3, 2, 1);
    c.in2 = p.dx1t.p; c.w2 = p.d1.wd; c.w2_plane = p.d1.plane;
    launch_stem_conv(c, st);
    LAUNCHED("stem_conv");
  }
  if ((rc = norm_relu_bwd(p, p.n[0], p.h0, prm->b1_n1_w, prm->b1_n1_b, nullptr, p.dh0, gr ? gr->b1_n1_w : nullptr,
                          gr ? gr->b1_n1_b : nullptr, st)) != NODE_OK)
    return rc;
  if (d_x) {   // the transposed first layer: dh0 -> the image
    launch_stem_conv0_dgrad(p.dh0, prm->conv0_w, d_x, N, p.Cin0, p.H, p.W, st);
    LAUNCHED("stem_conv0_dgrad");
  }
  if (!gr) return launch_ok("node_bnstem_bwd");
  launch_stem_conv0_wgrad(x, p.dh0, p.w0.slab, N, p.Cin0, p.H, p.W, p.w0.nsplit, p.w0.rps, st);
  LAUNCHED("stem_conv0_wgrad");

  SReduceArgs ra;
  memset(&ra, 0, sizeof(ra));
  int nj = 0;
  ra.job[nj++] = {p.w4.slab, gr->b2_c2_w, nullptr, 0, p.w4.nsplit, F, F, 9};
  ra.job[nj++] = {p.w3.slab, gr->b2_c1_w, nullptr, 0, p.w3.nsplit, F, 64, 9};
  ra.job[nj++] = {p.w3.slab2, gr->b2_ds_w, nullptr, 0, p.w3.nsplit, F, 64, 1};
  ra.job[nj++] = {p.w2.slab, gr->b1_c2_w, nullptr, 0, p.w2.nsplit, 64, 64, 9};
  ra.job[nj++] = {p.w1.slab, gr->b1_c1_w, nullptr, 0, p.w1.nsplit, 64, 64, 9};
  ra.job[nj++] = {p.w1.slab2, gr->b1_ds_w, nullptr, 0, p.w1.nsplit, 64, 64, 1};
  ra.job[nj++] = {p.w0.slab, gr->conv0_w, gr->conv0_b, 1, p.w0.nsplit, 64, 9 * p.Cin0, 1};
  ra.njobs = nj;
  launch_stem_reduce(ra, st);
  LAUNCHED("stem_reduce");
  return launch_ok("node_bnstem_bwd");
}

}  // extern "C"
