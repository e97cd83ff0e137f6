// C ABI of the `convolution` stem with norm = 'batch' (include/node_hip.h: node_bnconvstem_fwd / _bwd / _bwd_dx): ConvDownsample,
// model.py:148-164, whose norms are model.py:274 (nn.BatchNorm2d(64, track_running_stats=False)) -- as a host-side plan.  It is
// convstem_api.hip's plan with the other norm, as bnstem_api.hip is stem_api.hip's: the BatchNorm passes of kernels_batchnorm.hip
// (two-stage statistics, Chan's formula, fp64 backward partials; T = nullptr, relu = 1, scales 1.0f) around the stem's first-layer
// kernels, 4x4 / stride 2 gather GEMMs, four-class data gradients and split-K weight gradients (kernels_stem.hip, used as they
// are).  NHWC inside the workspace, NCHW at the boundary.
//
// forward (9 launches):  prep (two filters, conv0's filter, the zero rows) | conv0 | stats, apply (norm + ReLU -> triples) |
//                        conv 4x4/2 + bias | stats, apply | conv 4x4/2 + bias | NHWC -> NCHW
// backward: NCHW -> triples of dy (+ the last bias gradient's partial sums) | per 4x4 convolution, last first: weight gradient,
//           data gradient, BatchNorm sums + dx (the middle norm's -> fp32 dh1 and triples, the first norm's -> fp32 dh0) | the
//           middle bias gradient's partial sums | [d_x] the transposed first layer | [grads] conv0's weight and bias gradient, ONE
//           reduction launch: three slab jobs, two bias-partial jobs
// dgamma / dbeta leave the dx passes directly (their chunk-0 workgroups), so the reduction launch carries no norm job.  The biases
// of conv0 and the middle convolution stand in front of a BatchNorm: their gradients are zero identically and are computed the
// way the GroupNorm plan computes them (column sums of dh), rounding noise around zero.  Nothing is accumulated with atomics.
//
// The 16-tap geometry of k_stem_conv / k_stem_wgrad takes any Cin, Cout % 64 == 0 (column tiles of 64, K chunks of 32 or 64
// channels, one 64 x 64 tile pair per weight-gradient workgroup): the GroupNorm stem's power-of-two rule is its GroupNorm passes'
// (stem_gn_cb), not the GEMMs', so filters = 192, 384, ... are taken here.
#include "bnfunc.h"
#include <cstring>

using namespace node;

namespace {

constexpr int BIAS_ROWS = 256;      // rows per partial sum of the middle convolution's bias gradient

inline int down4(int h) { return (h + 2 - 4) / 2 + 1; }     // 4x4 stride 2 pad 1

struct Norm {                     // one BatchNorm of the plan: its input tensor's geometry and chunks
  int rows, C, H, W, cr, nchunk;
  float* stats;
};
struct BnConvStemPlan {
  int N, Cin0, H, W, F;
  int H0, W0, H1, W1, H2, W2, R0, R1, R2;
  float eps;
  float* w0t;
  Filt c1, c2;
  float *h0, *h1, *outn;
  Trip a0, a1;
  Norm n[2];                      // of h0, h1
  float* part;                    // forward partials of the pass in flight
  // backward
  Trip g2, dh1t;
  float *da, *dh1, *dh0;          // da: the data gradient in front of the norm in flight (the first norm's is the larger)
  double* gpart;
  float *bpart2, *bpart1;
  int nb2, nb1;
  Wg w2, w1, w0;
  size_t bytes;
};

// keep = false (the no-grad forward): h1 lies on h0 (h0 is dead once the first apply pass has written a0), both statistics on one
BnConvStemPlan make_plan(const node_convstem_shape* sh, bool keep, void* base) {
  BnConvStemPlan p;
  memset(&p, 0, sizeof(p));
  p.N = sh->n; p.Cin0 = sh->in_ch; p.H = sh->h; p.W = sh->w; p.F = sh->filters; p.eps = sh->eps;
  p.H0 = p.H - 2; p.W0 = p.W - 2;
  p.H1 = down4(p.H0); p.W1 = down4(p.W0);
  p.H2 = down4(p.H1); p.W2 = down4(p.W1);
  p.R0 = p.N * p.H0 * p.W0; p.R1 = p.N * p.H1 * p.W1; p.R2 = p.N * p.H2 * p.W2;
  const int F = p.F;
  p.n[0] = {p.R0, 64, p.H0, p.W0, 0, 0, nullptr};
  p.n[1] = {p.R1, 64, p.H1, p.W1, 0, 0, nullptr};
  size_t npart = 0;
  for (Norm& k : p.n) {
    k.cr = bnstem_chunk_rows(k.rows, k.C);
    k.nchunk = (k.rows + k.cr - 1) / k.cr;
    const size_t need = (size_t)k.nchunk * 2 * k.C;
    if (need > npart) npart = need;
  }
  Bump b(base);
  p.w0t = b.take<float>(28 * 64);
  p.c1 = take_filt(b, 64, 64, 16);
  p.c2 = take_filt(b, F, 64, 16);
  p.h0 = b.take<float>((size_t)p.R0 * 64);
  p.a0 = take_trip(b, p.R0, 64);
  p.h1 = keep ? b.take<float>((size_t)p.R1 * 64) : p.h0;
  p.a1 = take_trip(b, p.R1, 64);
  p.outn = b.take<float>((size_t)p.R2 * F);
  p.n[0].stats = b.take<float>(2 * 64);
  p.n[1].stats = keep ? b.take<float>(2 * 64) : p.n[0].stats;
  p.part = b.take<float>(npart);
  if (keep) {
    p.g2 = take_trip(b, p.R2, F);
    p.da = b.take<float>((size_t)p.R0 * 64);
    p.dh1 = b.take<float>((size_t)p.R1 * 64);
    p.dh1t = take_trip(b, p.R1, 64);
    p.dh0 = b.take<float>((size_t)p.R0 * 64);
    p.gpart = b.take<double>(npart);
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

int check_shape(const node_convstem_shape* sh) {
  if (!sh) return fail(NODE_ERR_NULL, "shape is NULL");
  if (sh->n <= 0 || sh->in_ch <= 0 || sh->h <= 0 || sh->w <= 0 || sh->filters <= 0) return fail(NODE_ERR_SHAPE, "bad stem shape");
  if (sh->h < 10 || sh->w < 10)
    return fail(NODE_ERR_SHAPE, "bad stem shape: the convolution stem takes images of 10 x 10 pixels and more (got %d x %d)", sh->h, sh->w);
  if (sh->in_ch > 3) return fail(NODE_ERR_UNSUPPORTED, "the stem's first layer takes in_ch <= 3 (got %d)", sh->in_ch);
  const int F = sh->filters;
  if (F < 64 || F % 64 != 0 || F > 4096)
    return fail(NODE_ERR_UNSUPPORTED, "the batch-norm convolution stem takes filters a multiple of 64 in [64, 4096]: 64-column GEMM "
                 "tiles (got %d)", F);
  const int h0 = sh->h - 2, w0 = sh->w - 2;
  if ((long long)h0 * w0 > 2400)
    return fail(NODE_ERR_UNSUPPORTED, "the stem's first-layer kernels have run on images of up to 2400 pixels behind the first "
                 "layer (got %d x %d)", h0, w0);
  const size_t biggest = (size_t)sh->n * h0 * w0 * 64;
  if (biggest + 4096 >= ((size_t)1 << 31) || (size_t)sh->n * sh->h * sh->w * F >= ((size_t)1 << 31))
    return fail(NODE_ERR_UNSUPPORTED, "stem tensors must stay under 2^31 elements");
  return NODE_OK;
}

int check_ptr(const void* p, const char* what, bool required) {
  if (!p) return required ? fail(NODE_ERR_NULL, "%s is NULL", what) : NODE_OK;
  if (((uintptr_t)p) & 15) return fail(NODE_ERR_ARG, "%s must be 16-byte aligned", what);
  return NODE_OK;
}

// node_convstem_params / node_convstem_grads: ten non-NULL, 16-byte aligned pointers
int check_tensors(const void* s, const char* what) {
  if (!s) return fail(NODE_ERR_NULL, "%s is NULL", what);
  const void* const* pp = reinterpret_cast<const void* const*>(s);
  for (int i = 0; i < 10; ++i) {
    if (!pp[i]) return fail(NODE_ERR_NULL, "tensor %d of %s is NULL", i, what);
    if (((uintptr_t)pp[i]) & 15) return fail(NODE_ERR_ARG, "tensor %d of %s must be 16-byte aligned", i, what);
  }
  return NODE_OK;
}

SBnArgs bn_args(const BnConvStemPlan& p, const Norm& k, const float* h, const float* gamma, const float* beta) {
  SBnArgs a;
  memset(&a, 0, sizeof(a));
  a.h = h; a.gamma = gamma; a.beta = beta; a.stats = k.stats;
  a.rows = k.rows; a.C = k.C; a.H = k.H; a.W = k.W; a.chunk_rows = k.cr; a.nchunk = k.nchunk; a.relu = 1; a.eps = p.eps;
  a.out_scale = 1.0f; a.da_scale = 1.0f;
  a.slices = 1;
  return a;
}

#define LAUNCHED(what)                                  \
  do {                                                  \
    if ((rc = launch_ok(what)) != NODE_OK) return rc;   \
  } while (0)

// a3 = relu(norm(h)) as triples; leaves the batch statistics in the norm's `stats`
int norm_relu(const BnConvStemPlan& p, const Norm& k, const float* h, const float* gamma, const float* beta, const Trip& a3, hipStream_t st) {
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

// the gradient of the norm's input from p.da: fp32 (dh) and / or triples (dh3); dgamma / dbeta nullable
int norm_relu_bwd(const BnConvStemPlan& p, const Norm& k, const float* h, const float* gamma, const float* beta, const Trip* dh3, float* dh,
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

// the checks of every entry point that runs: all of them before any launch
int check_call(const node_convstem_shape* shape, const node_convstem_params* prm, const void* ws) {
  int rc = check_shape(shape);
  if (rc != NODE_OK) return rc;
  if ((rc = check_tensors(prm, "params")) != NODE_OK) return rc;
  if (!ws) return fail(NODE_ERR_NULL, "workspace is NULL");
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  return NODE_OK;
}

// node_bnconvstem_bwd (d_x NULL, gr required) and node_bnconvstem_bwd_dx (d_x required, gr nullable: the data-gradient chain alone)
int bnconvstem_bwd(const node_convstem_shape* shape, const node_convstem_params* prm, const float* x, const float* grad_out,
                   const node_convstem_grads* gr, float* d_x, void* ws, size_t ws_bytes, void* stream, const char* who) {
  int rc = check_call(shape, prm, ws);
  if (rc != NODE_OK) return rc;
  if ((rc = check_ptr(x, "x", true)) != NODE_OK || (rc = check_ptr(grad_out, "grad_out", true)) != NODE_OK) return rc;
  if (!gr && !d_x) return fail(NODE_ERR_NULL, "neither grads nor d_x is given: nothing to compute");
  if (gr && (rc = check_tensors(gr, "grads")) != NODE_OK) return rc;
  if ((rc = check_ptr(d_x, "d_x", false)) != NODE_OK) return rc;
  const BnConvStemPlan p = make_plan(shape, true, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "bnconvstem workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int N = p.N, F = p.F;

  launch_stem_from_nchw(grad_out, nullptr, p.g2.p, p.g2.plane, N, F, p.H2 * p.W2, st, gr ? p.bpart2 : nullptr);
  LAUNCHED("stem_from_nchw");
  // the last convolution (4x4 / 2, 64 -> F): reads a1
  if (gr) {
    launch_stem_wgrad(wgrad_args(p.g2, nullptr, p.a1, p.w2, N, p.H1, p.W1, p.H2, p.W2, 64, F, 4, 2, 1), st);
    LAUNCHED("stem_wgrad");
  }
  launch_stem_conv(conv_dgrad_args(p.g2, p.c2, p.da, N, p.H2, p.W2, p.H1, p.W1, 4, 2, 1), st);
  LAUNCHED("stem_conv");
  // the gradient of h1 = the middle convolution's output: fp32 for its bias gradient, triples for the two GEMMs
  if ((rc = norm_relu_bwd(p, p.n[1], p.h1, prm->n2_w, prm->n2_b, &p.dh1t, gr ? p.dh1 : nullptr, gr ? gr->n2_w : nullptr,
                          gr ? gr->n2_b : nullptr, st)) != NODE_OK)
    return rc;
  // the middle convolution (4x4 / 2, 64 -> 64): reads a0
  if (gr) {
    launch_stem_colsum(p.dh1, p.bpart1, p.R1, 64, BIAS_ROWS, st);
    LAUNCHED("stem_colsum");
    launch_stem_wgrad(wgrad_args(p.dh1t, nullptr, p.a0, p.w1, N, p.H0, p.W0, p.H1, p.W1, 64, 64, 4, 2, 1), st);
    LAUNCHED("stem_wgrad");
  }
  launch_stem_conv(conv_dgrad_args(p.dh1t, p.c1, p.da, N, p.H1, p.W1, p.H0, p.W0, 4, 2, 1), st);
  LAUNCHED("stem_conv");
  if ((rc = norm_relu_bwd(p, p.n[0], p.h0, prm->n1_w, prm->n1_b, nullptr, p.dh0, gr ? gr->n1_w : nullptr, gr ? gr->n1_b : nullptr,
                          st)) != NODE_OK)
    return rc;
  if (d_x) {   // the transposed first layer: dh0 -> the image
    launch_stem_conv0_dgrad(p.dh0, prm->c0_w, d_x, N, p.Cin0, p.H, p.W, st);
    LAUNCHED("stem_conv0_dgrad");
  }
  if (!gr) return launch_ok(who);
  launch_stem_conv0_wgrad(x, p.dh0, p.w0.slab, N, p.Cin0, p.H, p.W, p.w0.nsplit, p.w0.rps, st);
  LAUNCHED("stem_conv0_wgrad");

  SReduceArgs ra;
  memset(&ra, 0, sizeof(ra));
  int nj = 0;
  ra.job[nj++] = {p.w2.slab, gr->c2_w, nullptr, 0, p.w2.nsplit, F, 64, 16};
  ra.job[nj++] = {p.w1.slab, gr->c1_w, nullptr, 0, p.w1.nsplit, 64, 64, 16};
  ra.job[nj++] = {p.w0.slab, gr->c0_w, gr->c0_b, 1, p.w0.nsplit, 64, 9 * p.Cin0, 1};
  ra.job[nj++] = {p.bpart1, gr->c1_b, nullptr, 3, p.nb1, 64, 0, 0};
  ra.job[nj++] = {p.bpart2, gr->c2_b, nullptr, 3, p.nb2, F, 0, 0};
  ra.njobs = nj;
  launch_stem_reduce(ra, st);
  LAUNCHED("stem_reduce");
  return launch_ok(who);
}

}  // namespace

extern "C" {

size_t node_bnconvstem_workspace_bytes(const node_convstem_shape* shape, int keep_for_backward) {
  if (check_shape(shape) != NODE_OK) return 0;
  return make_plan(shape, keep_for_backward != 0, nullptr).bytes;
}

int node_bnconvstem_describe(const node_convstem_shape* shape, node_bnfunc_info out[2]) {
  if (!out) return fail(NODE_ERR_NULL, "out is NULL");
  memset(out, 0, 2 * sizeof(*out));
  const int rc = check_shape(shape);
  if (rc != NODE_OK) return rc;
  const BnConvStemPlan p = make_plan(shape, true, nullptr);
  const Wg* reader[2] = {&p.w1, &p.w2};      // the weight gradient of the convolution that reads the norm's output
  for (int i = 0; i < 2; ++i) {
    const Norm& k = p.n[i];
    out[i].rows = k.rows; out[i].chunk_rows = k.cr; out[i].nchunk = k.nchunk;
    out[i].last_chunk_rows = k.rows - (k.nchunk - 1) * k.cr;
    out[i].column_tiles = k.C >> 6;
    out[i].wgrad_nsplit = reader[i]->nsplit; out[i].wgrad_rows_per_split = reader[i]->rps;
  }
  return NODE_OK;
}

int node_bnconvstem_fwd(const node_convstem_shape* shape, const node_convstem_params* prm, const float* x, float* out,
                        int keep_for_backward, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_call(shape, prm, ws);
  if (rc != NODE_OK) return rc;
  if ((rc = check_ptr(x, "x", true)) != NODE_OK || (rc = check_ptr(out, "out", true)) != NODE_OK) return rc;
  const BnConvStemPlan p = make_plan(shape, keep_for_backward != 0, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "bnconvstem workspace too small: %zu < %zu", ws_bytes, p.bytes);
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
  LAUNCHED("stem_prep");
  launch_stem_conv0_fwd(x, p.w0t, prm->c0_b, p.h0, N, p.Cin0, p.H, p.W, st);
  LAUNCHED("stem_conv0_fwd");
  if ((rc = norm_relu(p, p.n[0], p.h0, prm->n1_w, prm->n1_b, p.a0, st)) != NODE_OK) return rc;
  {
    SConvArgs c = conv_fwd_args(p.a0, p.c1, p.h1, N, p.H0, p.W0, p.H1, p.W1, 4, 2, 1);
    c.bias = prm->c1_b;
    launch_stem_conv(c, st);
    LAUNCHED("stem_conv");
  }
  if ((rc = norm_relu(p, p.n[1], p.h1, prm->n2_w, prm->n2_b, p.a1, st)) != NODE_OK) return rc;
  {
    SConvArgs c = conv_fwd_args(p.a1, p.c2, p.outn, N, p.H1, p.W1, p.H2, p.W2, 4, 2, 1);
    c.bias = prm->c2_b;
    launch_stem_conv(c, st);
    LAUNCHED("stem_conv");
  }
  launch_stem_to_nchw(p.outn, out, N, F, p.H2 * p.W2, st);
  return launch_ok("node_bnconvstem_fwd");
}

int node_bnconvstem_bwd(const node_convstem_shape* shape, const node_convstem_params* prm, const float* x, const float* grad_out,
                        const node_convstem_grads* gr, void* ws, size_t ws_bytes, void* stream) {
  if (!gr) {
    const int rc = check_shape(shape);
    return rc != NODE_OK ? rc : fail(NODE_ERR_NULL, "grads is NULL");
  }
  return bnconvstem_bwd(shape, prm, x, grad_out, gr, nullptr, ws, ws_bytes, stream, "node_bnconvstem_bwd");
}

int node_bnconvstem_bwd_dx(const node_convstem_shape* shape, const node_convstem_params* prm, const float* x, const float* grad_out,
                           const node_convstem_grads* gr, float* d_x, void* ws, size_t ws_bytes, void* stream) {
  if (!d_x) {
    const int rc = check_shape(shape);
    return rc != NODE_OK ? rc : fail(NODE_ERR_NULL, "d_x is NULL");
  }
  return bnconvstem_bwd(shape, prm, x, grad_out, gr, d_x, ws, ws_bytes, stream, "node_bnconvstem_bwd_dx");
}

}  // extern "C"
