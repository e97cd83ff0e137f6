// C ABI of the residual stem (include/node_hip.h: node_stem_fwd / node_stem_bwd / node_stem_conv): host-side plan of
// the launches in kernels_stem.hip.  Reference: model.py:167-178 (ResDownsample), model.py:284-310 (ResBlock).
//
// forward (11 launches):  prep | conv0 | GN+ReLU | conv 3x3/2 | conv 1x1/2 | GN+ReLU | conv 3x3 (+ shortcut) | GN+ReLU |
//                         conv 3x3/2 | conv 1x1/2 | GN+ReLU | conv 3x3 (+ shortcut) | NHWC -> NCHW
// backward: NCHW -> NHWC (+ triples) | per convolution: data gradient (+ the shortcut's on top) and weight gradient (the
//           shortcut's rides in the 3x3's launch) | per GroupNorm: backward pass | ONE reduction launch for every slab
// node_stem_banded_*: the same plan and the same bodies without the pixel ceiling; a GroupNorm pass whose (sample, channel block)
// does not fit the LDS is the banded pair of launches of kernels_stem_banded.hip, its band partials behind the plan's other pieces.
#include "host_common.h"
#include "stem.h"
#include "stem_plan.h"
#include "wino4.h"
#include <cstring>

using namespace node;

namespace {

inline int down2(int h) { return (h - 1) / 2 + 1; }     // 3x3 stride 2 pad 1 and 1x1 stride 2 pad 0 alike

struct StemPlan {
  int N, Cin0, H, W, F;
  int H0, W0, H1, W1, H2, W2, R0, R1, R2;
  float eps;
  float* w0t;
  Filt c1, c2, d1, c3, c4, d2;
  float *h0, *h1, *s1, *x1, *h3, *s2, *outn;
  Trip a0, a1, a2, a3;
  float* stats[4];
  // backward
  float *da3, *da2, *da1, *da0, *dh0;
  Trip g3, dh3t, dx1t, dh1t;
  float* gpart[4];
  Wg w4, w3, w2, w1, w0;
  // the last convolution (3x3, filters -> filters on an 8x8 image: the ODE conv's own shape) through the F(4x4,3x3)
  // pipeline of the ODE block (wino4.h): component GEMMs k_w4_gemm64b, weight gradient k_w4_wgrad
  bool f4;
  bool f4_b16;
  float *xh4, *rs4, *Va, *Vg, *M4, *Z4, *dU4, *U4[2], *dh3n;
  unsigned short* Ub4[2];
  // the banded family (node_stem_banded_*): per norm, whether its two passes are the banded ones of kernels_stem_banded.hip, and
  // their band partials.  node_stem_*: all false, nothing taken.
  bool banded[4];
  int band_px, nbands[4];
  float *fpart[4], *bpart[4];
  size_t bytes;
};

// NODE_TUNE_STEM_BANDED=all: every GroupNorm pass of the banded family is banded (tests, A/B); unset: only those whose block does not
// fit the LDS.  NODE_TUNE_STEM_BAND_PX: pixels per band.  Both are read per call and are part of the workspace layout: a backward
// runs under the values its forward ran under.
bool stem_band_all() {
  const char* e = getenv("NODE_TUNE_STEM_BANDED");
  return e && strcmp(e, "all") == 0;
}
int stem_band_px() {
  const int p = env_int("NODE_TUNE_STEM_BAND_PX", 128);
  return p < 1 ? 1 : p > (1 << 20) ? (1 << 20) : p;
}

bool stem_takes_w4(const node_stem_shape* sh) {
  if (env_int("NODE_TUNE_STEM_W4", 1) == 0) return false;       // 0: the stem's own gather-GEMM kernels for the last convolution too (A/B, tests)
  const int h2 = ((sh->h - 2 - 1) / 2 + 1 - 1) / 2 + 1, w2 = ((sh->w - 2 - 1) / 2 + 1 - 1) / 2 + 1;
  return h2 == 8 && w2 == 8 && sh->filters % 128 == 0 && sh->n % 8 == 0 && 16 % (sh->filters / 32) == 0;
}

StemPlan make_stem_plan(const node_stem_shape* sh, void* base, bool banded_family = false) {
  StemPlan p;
  memset(&p, 0, sizeof(p));
  p.N = sh->n; p.Cin0 = sh->in_ch; p.H = sh->h; p.W = sh->w; p.F = sh->filters; p.eps = sh->eps;
  p.H0 = p.H - 2; p.W0 = p.W - 2;
  p.H1 = down2(p.H0); p.W1 = down2(p.W0);
  p.H2 = down2(p.H1); p.W2 = down2(p.W1);
  p.R0 = p.N * p.H0 * p.W0; p.R1 = p.N * p.H1 * p.W1; p.R2 = p.N * p.H2 * p.W2;
  const int F = p.F, G64 = 32, GF = F < 32 ? F : 32;
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
  p.x1 = b.take<float>((size_t)p.R1 * 64);
  p.a2 = take_trip(b, p.R1, 64);
  p.h3 = b.take<float>((size_t)p.R2 * F);
  p.s2 = b.take<float>((size_t)p.R2 * F);
  p.a3 = take_trip(b, p.R2, F);
  p.outn = b.take<float>((size_t)p.R2 * F);
  p.stats[0] = b.take<float>((size_t)p.N * G64 * 2);
  p.stats[1] = b.take<float>((size_t)p.N * G64 * 2);
  p.stats[2] = b.take<float>((size_t)p.N * G64 * 2);
  p.stats[3] = b.take<float>((size_t)p.N * GF * 2);
  // backward
  p.g3 = take_trip(b, p.R2, F);
  p.da3 = b.take<float>((size_t)p.R2 * F);
  p.dh3t = take_trip(b, p.R2, F);
  p.da2 = b.take<float>((size_t)p.R1 * 64);
  p.dx1t = take_trip(b, p.R1, 64);
  p.da1 = b.take<float>((size_t)p.R1 * 64);
  p.dh1t = take_trip(b, p.R1, 64);
  p.da0 = b.take<float>((size_t)p.R0 * 64);
  p.dh0 = b.take<float>((size_t)p.R0 * 64);
  p.gpart[0] = b.take<float>((size_t)p.N * 2 * 64);
  p.gpart[1] = b.take<float>((size_t)p.N * 2 * 64);
  p.gpart[2] = b.take<float>((size_t)p.N * 2 * 64);
  p.gpart[3] = b.take<float>((size_t)p.N * 2 * F);
  p.w4 = take_wg(b, p.R2, F, F, 9, false);
  p.w3 = take_wg(b, p.R2, F, 64, 9, true);
  p.w2 = take_wg(b, p.R1, 64, 64, 9, false);
  p.w1 = take_wg(b, p.R1, 64, 64, 9, true);
  {   // conv0: K steps of two pixels over R0 rows, one 64 x 32 slab per workgroup
    int ns = p.R0 / 256;
    if (ns > 1024) ns = 1024;
    if (ns < 1) ns = 1;
    int rps = ((p.R0 + ns - 1) / ns + 7) & ~7;
    p.w0.rps = rps;
    p.w0.nsplit = (p.R0 + rps - 1) / rps;
    p.w0.slab = b.take<float>((size_t)p.w0.nsplit * 64 * 32);
    p.w0.slab2 = nullptr;
  }
  p.f4 = stem_takes_w4(sh);
  if (p.f4) {
    const int Nv = p.N;
    p.f4_b16 = w4_uses_bf16(Nv, F);
    p.xh4 = b.take<float>((size_t)p.R2 * F);
    p.rs4 = b.take<float>((size_t)p.N * GF);
    p.Va = b.take<float>(w4_v_elems(Nv, F));
    p.Vg = b.take<float>(w4_v_elems(Nv, F));
    p.M4 = b.take<float>(w4_v_elems(Nv, F));
    p.Z4 = b.take<float>(w4_z_elems(Nv, F));
    p.dU4 = b.take<float>((size_t)W4_COMPS * F * F);
    for (int i = 0; i < 2; ++i) {
      p.U4[i] = b.take<float>(w4_u_elems(F));
      p.Ub4[i] = b.take<unsigned short>(w4_ub_elems(F));
    }
    p.dh3n = b.take<float>((size_t)p.R2 * F);
  }
  if (banded_family) {     // (behind everything else: the other pieces lie where node_stem_* has them)
    const bool all = stem_band_all();
    p.band_px = stem_band_px();
    const int hw[4] = {p.H0 * p.W0, p.H1 * p.W1, p.H1 * p.W1, p.H2 * p.W2}, ch[4] = {64, 64, 64, F};
    for (int i = 0; i < 4; ++i) {
      const int groups = ch[i] < 32 ? ch[i] : 32;
      p.banded[i] = (all || stem_gn_cb(hw[i], ch[i], ch[i] / groups) == 0) && !(i == 3 && p.f4);
      if (!p.banded[i]) continue;
      p.nbands[i] = (hw[i] + p.band_px - 1) / p.band_px;
      p.fpart[i] = b.take<float>((size_t)p.N * p.nbands[i] * groups * 2);
      p.bpart[i] = b.take<float>((size_t)p.N * p.nbands[i] * 2 * ch[i]);
    }
  }
  p.bytes = b.off + 256;
  return p;
}

int check_stem_shape(const node_stem_shape* sh) {
  if (!sh) return fail(NODE_ERR_NULL, "shape is NULL");
  if (sh->n <= 0 || sh->in_ch <= 0 || sh->h < 5 || sh->w < 5 || sh->filters <= 0) return fail(NODE_ERR_SHAPE, "bad stem shape");
  if (sh->in_ch > 3) return fail(NODE_ERR_UNSUPPORTED, "the stem's first layer takes in_ch <= 3 (got %d)", sh->in_ch);
  if (sh->filters % 64 != 0) return fail(NODE_ERR_UNSUPPORTED, "the stem's kernels take filters %% 64 == 0 (got %d)", sh->filters);
  const size_t biggest = (size_t)sh->n * (sh->h - 2) * (sh->w - 2) * 64;
  if (biggest >= ((size_t)1 << 31)) return fail(NODE_ERR_UNSUPPORTED, "stem tensors must stay under 2^31 elements");
  if (stem_gn_cb((sh->h - 2) * (sh->w - 2), 64, 2) == 0)
    return fail(NODE_ERR_UNSUPPORTED, "the stem's GroupNorm passes hold (sample, 8 channels) blocks in LDS: images up to %d pixels "
                 "behind the first layer (got %d x %d)", 150 * 1024 / 64, sh->h - 2, sh->w - 2);
  {   // the last block's GroupNorm passes run on `filters` channels in min(32, filters) groups (model.py:268-271)
    const int cpg = sh->filters / (sh->filters < 32 ? sh->filters : 32);
    const int h1 = (sh->h - 2 - 1) / 2 + 1, w1 = (sh->w - 2 - 1) / 2 + 1, h2 = (h1 - 1) / 2 + 1, w2 = (w1 - 1) / 2 + 1;
    if ((sh->filters & (sh->filters - 1)) != 0 || stem_gn_cb(h2 * w2, sh->filters, cpg) == 0)
      return fail(NODE_ERR_UNSUPPORTED, "the stem's GroupNorm passes take power-of-two filter counts (whole groups per "
                   "power-of-two channel block); got %d", sh->filters);
  }
  return NODE_OK;
}

// node_stem_banded_*: check_stem_shape without the pixel ceiling -- a GroupNorm pass whose block does not fit the LDS is banded --
// and with every tensor of the plan under 2^31 elements
int check_stem_banded_shape(const node_stem_shape* sh) {
  if (!sh) return fail(NODE_ERR_NULL, "shape is NULL");
  if (sh->n <= 0 || sh->in_ch <= 0 || sh->h < 5 || sh->w < 5 || sh->filters <= 0) return fail(NODE_ERR_SHAPE, "bad stem shape");
  if (sh->in_ch > 3) return fail(NODE_ERR_UNSUPPORTED, "the stem's first layer takes in_ch <= 3 (got %d)", sh->in_ch);
  const int F = sh->filters;
  if (F < 64 || F > 4096 || (F & (F - 1)) != 0)
    return fail(NODE_ERR_UNSUPPORTED, "the stem's GroupNorm passes take power-of-two filter counts in [64, 4096]; got %d", F);
  const size_t n = (size_t)sh->n, lim = (size_t)1 << 31;
  const size_t hw0 = (size_t)(sh->h - 2) * (sh->w - 2);
  const size_t hw1 = (size_t)down2(sh->h - 2) * down2(sh->w - 2);
  const size_t hw2 = (size_t)down2(down2(sh->h - 2)) * down2(down2(sh->w - 2));
  // the largest of each family: the input, fp32 tensors and one plane of the triples (rows + 1) behind each of the three resolutions
  if (hw0 >= lim || n * hw0 >= lim || n * sh->in_ch * sh->h * sh->w >= lim || (n * hw0 + 1) * 64 >= lim || (n * hw1 + 1) * 64 >= lim ||
      (n * hw2 + 1) * F >= lim)
    return fail(NODE_ERR_UNSUPPORTED, "stem tensors must stay under 2^31 elements");
  return NODE_OK;
}

SGnBandArgs band_args(const StemPlan& p, int i, const SGnArgs& g) {
  SGnBandArgs a;
  memset(&a, 0, sizeof(a));
  a.g = g;
  a.band_px = p.band_px; a.nbands = p.nbands[i]; a.CB = stem_gn_band_cb(g.C, g.cpg);
  a.fpart = p.fpart[i]; a.bpart = p.bpart[i];
  return a;
}
// norm i of the plan (block 1 norm1, norm2, block 2 norm1, norm2): resident where its block fits, banded otherwise
int run_gn_fwd(const StemPlan& p, int i, const SGnArgs& g, hipStream_t st) {
  if (p.banded[i]) {
    launch_stem_gn_banded_fwd(band_args(p, i, g), st);
    return launch_ok("stem_gn_banded_fwd");
  }
  launch_stem_gn_fwd(g, st);
  return launch_ok("stem_gn_fwd");
}
int run_gn_bwd(const StemPlan& p, int i, const SGnArgs& g, hipStream_t st) {
  if (p.banded[i]) {
    launch_stem_gn_banded_bwd(band_args(p, i, g), st);
    return launch_ok("stem_gn_banded_bwd");
  }
  launch_stem_gn_bwd(g, st);
  return launch_ok("stem_gn_bwd");
}

// node_stem_fwd (banded_family false) and node_stem_banded_fwd (true): one body, the shape check and the plan's per-norm decision differ
int stem_fwd(const node_stem_shape* shape, const node_stem_params* prm, const float* x, float* out, void* ws, size_t ws_bytes,
             void* stream, bool banded_family, const char* who) {
  w4_refresh_tuning();     // (NODE_TUNE_W4_*: once per call)
  int rc = banded_family ? check_stem_banded_shape(shape) : check_stem_shape(shape);
  if (rc != NODE_OK) return rc;
  if (!prm || !x || !out || !ws) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  const float* const* pp = reinterpret_cast<const float* const*>(prm);
  for (int i = 0; i < 16; ++i)
    if (!pp[i]) return fail(NODE_ERR_NULL, "stem parameter %d is NULL", i);
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  StemPlan p = make_stem_plan(shape, ws, banded_family);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "stem workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int N = p.N, F = p.F;

  SPrepArgs pa;
  memset(&pa, 0, sizeof(pa));
  const Filt* fl[6] = {&p.c1, &p.c2, &p.d1, &p.c3, &p.c4, &p.d2};
  const float* fw[6] = {prm->b1_c1_w, prm->b1_c2_w, prm->b1_ds_w, prm->b2_c1_w, prm->b2_c2_w, prm->b2_ds_w};
  for (int i = 0; i < 6; ++i) pa.job[i] = {fw[i], fl[i]->wf, fl[i]->wd, fl[i]->Cout, fl[i]->Cin, fl[i]->taps};
  pa.njobs = 6;
  pa.w0 = prm->conv0_w; pa.w0t = p.w0t; pa.k0 = 9 * p.Cin0;
  const Trip* tz[8] = {&p.a0, &p.a1, &p.a2, &p.a3, &p.g3, &p.dh3t, &p.dx1t, &p.dh1t};
  for (int i = 0; i < 8; ++i) {
    pa.zero[i] = tz[i]->p + (size_t)tz[i]->rows * tz[i]->C;
    pa.zero_plane[i] = tz[i]->plane;
    pa.zero_c[i] = tz[i]->C;
  }
  pa.nzero = 8;
  if (F > 4096) return fail(NODE_ERR_UNSUPPORTED, "filters > 4096");
  launch_stem_prep(pa, st);
  if ((rc = launch_ok("stem_prep")) != NODE_OK) return rc;

  launch_stem_conv0_fwd(x, p.w0t, prm->conv0_b, p.h0, N, p.Cin0, p.H, p.W, st);
  if ((rc = launch_ok("stem_conv0_fwd")) != NODE_OK) return rc;
  {   // block 1: relu(norm1(h0)) -> a0
    SGnArgs g = gn_args(p.h0, prm->b1_n1_w, prm->b1_n1_b, p.stats[0], N, p.H0 * p.W0, 64, p.eps);
    g.a3 = p.a0.p; g.a_plane = p.a0.plane;
    if ((rc = run_gn_fwd(p, 0, g, st)) != NODE_OK) return rc;
  }
  {   // conv1 (3x3 / 2) and the shortcut (1x1 / 2) in one launch
    SConvArgs c = conv_fwd_args(p.a0, p.c1, p.h1, N, p.H0, p.W0, p.H1, p.W1, 3, 2, 1);
    c.w2 = p.d1.wf; c.w2_plane = p.d1.plane; c.out2 = p.s1;
    launch_stem_conv(c, st);
    if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
  }
  {
    SGnArgs g = gn_args(p.h1, prm->b1_n2_w, prm->b1_n2_b, p.stats[1], N, p.H1 * p.W1, 64, p.eps);
    g.a3 = p.a1.p; g.a_plane = p.a1.plane;
    if ((rc = run_gn_fwd(p, 1, g, st)) != NODE_OK) return rc;
  }
  {
    SConvArgs c = conv_fwd_args(p.a1, p.c2, p.x1, N, p.H1, p.W1, p.H1, p.W1, 3, 1, 1);
    c.res = p.s1;
    launch_stem_conv(c, st);
    if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
  }
  {   // block 2
    SGnArgs g = gn_args(p.x1, prm->b2_n1_w, prm->b2_n1_b, p.stats[2], N, p.H1 * p.W1, 64, p.eps);
    g.a3 = p.a2.p; g.a_plane = p.a2.plane;
    if ((rc = run_gn_fwd(p, 2, g, st)) != NODE_OK) return rc;
  }
  {
    SConvArgs c = conv_fwd_args(p.a2, p.c3, p.h3, N, p.H1, p.W1, p.H2, p.W2, 3, 2, 1);
    c.w2 = p.d2.wf; c.w2_plane = p.d2.plane; c.out2 = p.s2;
    launch_stem_conv(c, st);
    if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
  }
  if (p.f4) {
    W4PackJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    for (int i = 0; i < 2; ++i) {
      jobs.w[i] = prm->b2_c2_w; jobs.u[i] = p.U4[i]; jobs.ub[i] = p.f4_b16 ? p.Ub4[i] : nullptr; jobs.dgrad[i] = i; jobs.plain[i] = 1;
    }
    launch_w4_pack(jobs, 2, F, st);
    if ((rc = launch_ok("w4_pack")) != NODE_OK) return rc;
    launch_w4s_stem_in(p.h3, prm->b2_n2_w, prm->b2_n2_b, p.eps, F / 32, p.xh4, p.rs4, p.Va, N, F, N, st);
    if ((rc = launch_ok("w4s_stem_in")) != NODE_OK) return rc;
    launch_w4_gemm(p.Va, p.U4[0], p.M4, nullptr, N, F, st, p.f4_b16 ? p.Ub4[0] : nullptr);
    if ((rc = launch_ok("w4_gemm")) != NODE_OK) return rc;
    launch_w4s_stem_out(p.M4, p.s2, out, N, F, st);
    return launch_ok(who);
  }
  {
    SGnArgs g = gn_args(p.h3, prm->b2_n2_w, prm->b2_n2_b, p.stats[3], N, p.H2 * p.W2, F, p.eps);
    g.a3 = p.a3.p; g.a_plane = p.a3.plane;
    if ((rc = run_gn_fwd(p, 3, g, st)) != NODE_OK) return rc;
  }
  {
    SConvArgs c = conv_fwd_args(p.a3, p.c4, p.outn, N, p.H2, p.W2, p.H2, p.W2, 3, 1, 1);
    c.res = p.s2;
    launch_stem_conv(c, st);
    if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
  }
  launch_stem_to_nchw(p.outn, out, N, F, p.H2 * p.W2, st);
  if ((rc = launch_ok("stem_to_nchw")) != NODE_OK) return rc;
  return launch_ok(who);
}

}  // namespace

extern "C" {

size_t node_stem_workspace_bytes(const node_stem_shape* shape) {
  if (check_stem_shape(shape) != NODE_OK) return 0;
  return make_stem_plan(shape, nullptr).bytes;
}

int node_stem_describe(const node_stem_shape* shape, node_stem_info* out) {
  if (!out) return fail(NODE_ERR_NULL, "out is NULL");
  memset(out, 0, sizeof(*out));
  const int rc = check_stem_shape(shape);
  if (rc != NODE_OK) return rc;
  const StemPlan p = make_stem_plan(shape, nullptr);
  out->gn[0] = gn_info(p.N, p.H0 * p.W0, 64);      // the gn_args of node_stem_fwd / stem_bwd, in the forward's order
  out->gn[1] = gn_info(p.N, p.H1 * p.W1, 64);
  out->gn[2] = gn_info(p.N, p.H1 * p.W1, 64);
  out->gn[3] = gn_info(p.N, p.H2 * p.W2, p.F);
  out->takes_w4 = p.f4 ? 1 : 0;
  const Wg* wg[4] = {&p.w1, &p.w2, &p.w3, &p.w4};
  for (int i = 0; i < 4; ++i) {
    out->wgrad_nsplit[i] = wg[i]->nsplit;
    out->wgrad_rows_per_split[i] = wg[i]->rps;
  }
  return NODE_OK;
}

int node_stem_fwd(const node_stem_shape* shape, const node_stem_params* prm, const float* x, float* out, void* ws, size_t ws_bytes,
                  void* stream) {
  return stem_fwd(shape, prm, x, out, ws, ws_bytes, stream, false, "node_stem_fwd");
}

}  // extern "C"

namespace {
// node_stem_bwd (gr given, d_x NULL) and node_stem_bwd_dx (d_x given; gr NULL: the data-gradient chain alone -- no weight-gradient,
// no slab-reduction launch)
int stem_bwd(const node_stem_shape* shape, const node_stem_params* prm, const float* x, const float* grad_out,
             const node_stem_grads* gr, float* d_x, void* ws, size_t ws_bytes, void* stream, const char* who, bool banded_family = false) {
  w4_refresh_tuning();     // (NODE_TUNE_W4_*: once per call)
  int rc = banded_family ? check_stem_banded_shape(shape) : check_stem_shape(shape);
  if (rc != NODE_OK) return rc;
  if (!prm || !x || !grad_out || !ws) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  const float* const* pp = reinterpret_cast<const float* const*>(prm);
  float* const* gp = reinterpret_cast<float* const*>(gr);
  for (int i = 0; i < 16; ++i)
    if (!pp[i] || (gr && !gp[i])) return fail(NODE_ERR_NULL, "stem parameter / gradient %d is NULL", i);
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  StemPlan p = make_stem_plan(shape, ws, banded_family);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "stem workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int N = p.N, F = p.F;
  const int HW0 = p.H0 * p.W0, HW1 = p.H1 * p.W1, HW2 = p.H2 * p.W2;

  // dL/d out: also the gradient of the second block's shortcut s2
  launch_stem_from_nchw(grad_out, nullptr, p.g3.p, p.g3.plane, N, F, HW2, st);
  if ((rc = launch_ok("stem_from_nchw")) != NODE_OK) return rc;
  if (p.f4) {
    // block 2, conv2 through the F(4x4,3x3) pipeline: V and Z of dL/d out, data-gradient GEMM, then ONE pass for the ReLU mask and
    // GroupNorm's backward (k_w4s_pass<2, 0>, the ODE block's own), the weight gradient in the transform domain
    launch_w4s_stem_gin(grad_out, p.Vg, p.Z4, N, F, N, st);
    if ((rc = launch_ok("w4s_stem_gin")) != NODE_OK) return rc;
    launch_w4_gemm(p.Vg, p.U4[1], p.M4, nullptr, N, F, st, p.f4_b16 ? p.Ub4[1] : nullptr);
    if ((rc = launch_ok("w4_gemm")) != NODE_OK) return rc;
    W4sArgs a;
    memset(&a, 0, sizeof(a));
    a.N = N; a.Q = 1; a.Nv = N; a.C = F; a.cpg = F / 32; a.eps = p.eps;
    a.h.M = p.M4; a.h.gamma = prm->b2_n2_w; a.h.beta = prm->b2_n2_b; a.h.xhat_s = p.xh4; a.h.rstd = p.rs4; a.h.osign = 1.f;
    a.h.gpart = p.gpart[3]; a.h.out_nhwc = p.dh3n;
    launch_w4s_pass(2, 0, a, st);
    if ((rc = launch_ok("w4s_pass")) != NODE_OK) return rc;
    launch_stem_split(p.dh3n, p.dh3t.p, p.dh3t.plane, (size_t)p.R2 * F, st);
    if ((rc = launch_ok("stem_split")) != NODE_OK) return rc;
    if (gr) {
      W4WgradArgs wa;
      memset(&wa, 0, sizeof(wa));
      wa.V1 = p.Va; wa.Z1 = p.Z4; wa.dU = p.dU4; wa.N = N; wa.C = F;
      launch_w4_wgrad(wa, st);
      if ((rc = launch_ok("w4_wgrad")) != NODE_OK) return rc;
      launch_w4_du_to_dw(p.dU4, gr->b2_c2_w, F, st);
      if ((rc = launch_ok("w4_du_to_dw")) != NODE_OK) return rc;
    }
  } else {
  // block 2, conv2 (3x3, F -> F) : weight gradient, data gradient -> da3
    if (gr) {
      launch_stem_wgrad(wgrad_args(p.g3, nullptr, p.a3, p.w4, N, p.H2, p.W2, p.H2, p.W2, F, F, 3, 1, 1), st);
      if ((rc = launch_ok("stem_wgrad")) != NODE_OK) return rc;
    }
    launch_stem_conv(conv_dgrad_args(p.g3, p.c4, p.da3, N, p.H2, p.W2, p.H2, p.W2, 3, 1, 1), st);
    if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
    {
      SGnArgs g = gn_args(p.h3, prm->b2_n2_w, prm->b2_n2_b, p.stats[3], N, HW2, F, p.eps);
      g.da = p.da3; g.dh = nullptr; g.dh3 = p.dh3t.p; g.dh_plane = p.dh3t.plane; g.gpart = p.gpart[3];
      if ((rc = run_gn_bwd(p, 3, g, st)) != NODE_OK) return rc;
    }
  }
  // block 2, conv1 (3x3 / 2, 64 -> F) + shortcut (1x1 / 2, 64 -> F): both read a2
  if (gr) {
    launch_stem_wgrad(wgrad_args(p.dh3t, &p.g3, p.a2, p.w3, N, p.H1, p.W1, p.H2, p.W2, 64, F, 3, 2, 1), st);
    if ((rc = launch_ok("stem_wgrad")) != NODE_OK) return rc;
  }
  {   // data gradient of conv1 (3x3 / 2) + the shortcut's (1x1 / 2: one more K segment of the (even, even) pixels)
    SConvArgs c = conv_dgrad_args(p.dh3t, p.c3, p.da2, N, p.H2, p.W2, p.H1, p.W1, 3, 2, 1);
    c.in2 = p.g3.p; c.w2 = p.d2.wd; c.w2_plane = p.d2.plane;
    launch_stem_conv(c, st);
    if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
  }
  {
    SGnArgs g = gn_args(p.x1, prm->b2_n1_w, prm->b2_n1_b, p.stats[2], N, HW1, 64, p.eps);
    g.da = p.da2; g.dh = nullptr; g.dh3 = p.dx1t.p; g.dh_plane = p.dx1t.plane; g.gpart = p.gpart[2];
    if ((rc = run_gn_bwd(p, 2, g, st)) != NODE_OK) return rc;
  }
  // block 1, conv2 (3x3, 64 -> 64): dx1 is the gradient of its output AND of the shortcut s1
  if (gr) {
    launch_stem_wgrad(wgrad_args(p.dx1t, nullptr, p.a1, p.w2, N, p.H1, p.W1, p.H1, p.W1, 64, 64, 3, 1, 1), st);
    if ((rc = launch_ok("stem_wgrad")) != NODE_OK) return rc;
  }
  launch_stem_conv(conv_dgrad_args(p.dx1t, p.c2, p.da1, N, p.H1, p.W1, p.H1, p.W1, 3, 1, 1), st);
  if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
  {
    SGnArgs g = gn_args(p.h1, prm->b1_n2_w, prm->b1_n2_b, p.stats[1], N, HW1, 64, p.eps);
    g.da = p.da1; g.dh = nullptr; g.dh3 = p.dh1t.p; g.dh_plane = p.dh1t.plane; g.gpart = p.gpart[1];
    if ((rc = run_gn_bwd(p, 1, g, st)) != NODE_OK) return rc;
  }
  // block 1, conv1 (3x3 / 2) + shortcut (1x1 / 2): both read a0
  if (gr) {
    launch_stem_wgrad(wgrad_args(p.dh1t, &p.dx1t, p.a0, p.w1, N, p.H0, p.W0, p.H1, p.W1, 64, 64, 3, 2, 1), st);
    if ((rc = launch_ok("stem_wgrad")) != NODE_OK) return rc;
  }
  {
    SConvArgs c = conv_dgrad_args(p.dh1t, p.c1, p.da0, N, p.H1, p.W1, p.H0, p.W0, 3, 2, 1);
    c.in2 = p.dx1t.p; c.w2 = p.d1.wd; c.w2_plane = p.d1.plane;
    launch_stem_conv(c, st);
    if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
  }
  {
    SGnArgs g = gn_args(p.h0, prm->b1_n1_w, prm->b1_n1_b, p.stats[0], N, HW0, 64, p.eps);
    g.da = p.da0; g.dh = p.dh0; g.dh3 = nullptr; g.gpart = p.gpart[0];
    if ((rc = run_gn_bwd(p, 0, g, st)) != NODE_OK) return rc;
  }
  if (d_x) {   // the transposed first layer: dh0 -> the image
    launch_stem_conv0_dgrad(p.dh0, prm->conv0_w, d_x, N, p.Cin0, p.H, p.W, st);
    if ((rc = launch_ok("stem_conv0_dgrad")) != NODE_OK) return rc;
  }
  if (!gr) return launch_ok(who);
  launch_stem_conv0_wgrad(x, p.dh0, p.w0.slab, N, p.Cin0, p.H, p.W, p.w0.nsplit, p.w0.rps, st);
  if ((rc = launch_ok("stem_conv0_wgrad")) != NODE_OK) return rc;

  SReduceArgs ra;
  memset(&ra, 0, sizeof(ra));
  int nj = 0;
  if (!p.f4) ra.job[nj++] = {p.w4.slab, gr->b2_c2_w, nullptr, 0, p.w4.nsplit, F, F, 9};
  ra.job[nj++] = {p.w3.slab, gr->b2_c1_w, nullptr, 0, p.w3.nsplit, F, 64, 9};
  ra.job[nj++] = {p.w3.slab2, gr->b2_ds_w, nullptr, 0, p.w3.nsplit, F, 64, 1};
  ra.job[nj++] = {p.w2.slab, gr->b1_c2_w, nullptr, 0, p.w2.nsplit, 64, 64, 9};
  ra.job[nj++] = {p.w1.slab, gr->b1_c1_w, nullptr, 0, p.w1.nsplit, 64, 64, 9};
  ra.job[nj++] = {p.w1.slab2, gr->b1_ds_w, nullptr, 0, p.w1.nsplit, 64, 64, 1};
  ra.job[nj++] = {p.w0.slab, gr->conv0_w, gr->conv0_b, 1, p.w0.nsplit, 64, 9 * p.Cin0, 1};
  ra.job[nj++] = {p.gpart[0], gr->b1_n1_w, gr->b1_n1_b, 2, N, 64, 0, 0};
  ra.job[nj++] = {p.gpart[1], gr->b1_n2_w, gr->b1_n2_b, 2, N, 64, 0, 0};
  ra.job[nj++] = {p.gpart[2], gr->b2_n1_w, gr->b2_n1_b, 2, N, 64, 0, 0};
  ra.job[nj++] = {p.gpart[3], gr->b2_n2_w, gr->b2_n2_b, 2, N, F, 0, 0};
  ra.njobs = nj;
  launch_stem_reduce(ra, st);
  if ((rc = launch_ok("stem_reduce")) != NODE_OK) return rc;
  return launch_ok(who);
}
}  // namespace

extern "C" {

int node_stem_bwd(const node_stem_shape* shape, const node_stem_params* prm, const float* x, const float* grad_out,
                  const node_stem_grads* gr, void* ws, size_t ws_bytes, void* stream) {
  if (!gr) {
    const int rc = check_stem_shape(shape);
    return rc != NODE_OK ? rc : fail(NODE_ERR_NULL, "a required pointer is NULL");
  }
  return stem_bwd(shape, prm, x, grad_out, gr, nullptr, ws, ws_bytes, stream, "node_stem_bwd");
}

int node_stem_bwd_dx(const node_stem_shape* shape, const node_stem_params* prm, const float* x, const float* grad_out,
                     const node_stem_grads* gr, float* d_x, void* ws, size_t ws_bytes, void* stream) {
  if (!d_x) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  return stem_bwd(shape, prm, x, grad_out, gr, d_x, ws, ws_bytes, stream, "node_stem_bwd_dx");
}

// ---------------------------------------------------------------------------------------------------------------
// node_stem_banded_*: the same plan and bodies; a GroupNorm pass whose block does not fit the LDS runs banded
// ---------------------------------------------------------------------------------------------------------------
size_t node_stem_banded_workspace_bytes(const node_stem_shape* shape) {
  if (check_stem_banded_shape(shape) != NODE_OK) return 0;
  return make_stem_plan(shape, nullptr, true).bytes;
}

int node_stem_banded_describe(const node_stem_shape* shape, node_stem_banded_info* out) {
  if (!out) return fail(NODE_ERR_NULL, "out is NULL");
  memset(out, 0, sizeof(*out));
  const int rc = check_stem_banded_shape(shape);
  if (rc != NODE_OK) return rc;
  const StemPlan p = make_stem_plan(shape, nullptr, true);
  const int hw[4] = {p.H0 * p.W0, p.H1 * p.W1, p.H1 * p.W1, p.H2 * p.W2}, ch[4] = {64, 64, 64, p.F};
  for (int i = 0; i < 4; ++i) {
    node_stem_banded_gn_info& o = out->gn[i];
    if (!p.banded[i]) {      // the resident launch: node_stem_describe's record
      o.gn = gn_info(p.N, hw[i], ch[i]);
      continue;
    }
    const int cpg = ch[i] / (ch[i] < 32 ? ch[i] : 32), cb = stem_gn_band_cb(ch[i], cpg);
    o.gn.hw = hw[i]; o.gn.channels = ch[i]; o.gn.cpg = cpg; o.gn.cb = cb;
    o.gn.blocks_per_sample = ch[i] / cb;
    o.gn.grid = p.N * p.nbands[i] * (ch[i] / cb);
    o.banded = 1;
    o.band_px = p.band_px;
    o.bands_per_sample = p.nbands[i];
    o.grid_first = o.grid_second = o.gn.grid;
  }
  out->takes_w4 = p.f4 ? 1 : 0;
  const Wg* wg[4] = {&p.w1, &p.w2, &p.w3, &p.w4};
  for (int i = 0; i < 4; ++i) {
    out->wgrad_nsplit[i] = wg[i]->nsplit;
    out->wgrad_rows_per_split[i] = wg[i]->rps;
  }
  return NODE_OK;
}

int node_stem_banded_fwd(const node_stem_shape* shape, const node_stem_params* prm, const float* x, float* out, void* ws,
                         size_t ws_bytes, void* stream) {
  return stem_fwd(shape, prm, x, out, ws, ws_bytes, stream, true, "node_stem_banded_fwd");
}

int node_stem_banded_bwd(const node_stem_shape* shape, const node_stem_params* prm, const float* x, const float* grad_out,
                         const node_stem_grads* gr, void* ws, size_t ws_bytes, void* stream) {
  if (!gr) {
    const int rc = check_stem_banded_shape(shape);
    return rc != NODE_OK ? rc : fail(NODE_ERR_NULL, "a required pointer is NULL");
  }
  return stem_bwd(shape, prm, x, grad_out, gr, nullptr, ws, ws_bytes, stream, "node_stem_banded_bwd", true);
}

int node_stem_banded_bwd_dx(const node_stem_shape* shape, const node_stem_params* prm, const float* x, const float* grad_out,
                            const node_stem_grads* gr, float* d_x, void* ws, size_t ws_bytes, void* stream) {
  if (!d_x) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  return stem_bwd(shape, prm, x, grad_out, gr, d_x, ws, ws_bytes, stream, "node_stem_banded_bwd_dx", true);
}

// ---------------------------------------------------------------------------------------------------------------
// diagnostics: one convolution of the family on NCHW tensors
// ---------------------------------------------------------------------------------------------------------------
namespace {
struct OnePlan {
  int YH, YW;
  Filt f;
  Trip xin, dyt;
  float *xn, *dyn, *resn;
  Wg wg;
  size_t bytes;
};
OnePlan make_one(const node_conv_geom* g, void* base) {
  OnePlan p;
  memset(&p, 0, sizeof(p));
  p.YH = (g->x_h + 2 * g->pad - g->k) / g->stride + 1;
  p.YW = (g->x_w + 2 * g->pad - g->k) / g->stride + 1;
  Bump b(base);
  p.f = take_filt(b, g->cout, g->cin, g->k * g->k);
  p.xin = take_trip(b, g->n * g->x_h * g->x_w, g->cin);
  p.dyt = take_trip(b, g->n * p.YH * p.YW, g->cout);
  p.xn = b.take<float>((size_t)g->n * g->x_h * g->x_w * g->cin);
  p.dyn = b.take<float>((size_t)g->n * p.YH * p.YW * g->cout);
  p.resn = b.take<float>((size_t)g->n * (g->x_h * g->x_w * g->cin > p.YH * p.YW * g->cout ? g->x_h * g->x_w * g->cin : p.YH * p.YW * g->cout));
  p.wg = take_wg(b, g->n * p.YH * p.YW, g->cout, g->cin, g->k * g->k, false);
  p.bytes = b.off + 256;
  return p;
}
int check_geom(const node_conv_geom* g) {
  if (!g) return fail(NODE_ERR_NULL, "geometry is NULL");
  if (g->n <= 0 || g->x_h <= 0 || g->x_w <= 0) return fail(NODE_ERR_SHAPE, "bad geometry");
  if (g->cin % 64 != 0 || g->cout % 64 != 0 || g->cin <= 0 || g->cout <= 0) return fail(NODE_ERR_UNSUPPORTED, "cin, cout must be multiples of 64");
  if (g->k == 4) {     // the down-sampling convolution of the `convolution` / `ode2` stems: 4x4, stride 2, padding 1 and nothing else
    if (g->stride != 2 || g->pad != 1) return fail(NODE_ERR_UNSUPPORTED, "4x4 filters run with stride 2 and padding 1 only (got stride %d, pad %d)", g->stride, g->pad);
    if (g->x_h < 4 || g->x_w < 4) return fail(NODE_ERR_SHAPE, "a 4x4 stride-2 convolution takes images of 4x4 pixels and more");
    return NODE_OK;
  }
  if (!((g->k == 3 && g->pad == 1) || (g->k == 1 && g->pad == 0)) || (g->stride != 1 && g->stride != 2))
    return fail(NODE_ERR_UNSUPPORTED, "3x3 pad 1 or 1x1 pad 0, stride 1 or 2; 4x4 pad 1 stride 2");
  return NODE_OK;
}
}  // namespace

// the transposed first layer alone, on NCHW tensors: dy -> NHWC in the workspace, then k_stem_conv0_dgrad
static int check_dgrad0(const node_stem_shape* sh) {
  if (!sh) return fail(NODE_ERR_NULL, "shape is NULL");
  if (sh->n <= 0 || sh->in_ch <= 0 || sh->h < 3 || sh->w < 3) return fail(NODE_ERR_SHAPE, "bad shape");
  if (sh->in_ch > 3) return fail(NODE_ERR_UNSUPPORTED, "the stem's first layer takes in_ch <= 3 (got %d)", sh->in_ch);
  if ((size_t)sh->n * sh->h * sh->w * 64 >= ((size_t)1 << 31)) return fail(NODE_ERR_UNSUPPORTED, "stem tensors must stay under 2^31 elements");
  return NODE_OK;
}

size_t node_stem_conv0_dgrad_workspace_bytes(const node_stem_shape* shape) {
  if (check_dgrad0(shape) != NODE_OK) return 0;
  return (size_t)shape->n * (shape->h - 2) * (shape->w - 2) * 64 * sizeof(float) + 256;
}

int node_stem_conv0_dgrad(const node_stem_shape* shape, const float* w0, const float* dy, float* d_x, void* ws, size_t ws_bytes,
                          void* stream) {
  int rc = check_dgrad0(shape);
  if (rc != NODE_OK) return rc;
  if (!w0 || !dy || !d_x || !ws) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  if (ws_bytes < node_stem_conv0_dgrad_workspace_bytes(shape)) return fail(NODE_ERR_WORKSPACE, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  launch_stem_from_nchw(dy, (float*)ws, nullptr, 0, shape->n, 64, (shape->h - 2) * (shape->w - 2), st);
  if ((rc = launch_ok("stem_from_nchw")) != NODE_OK) return rc;
  launch_stem_conv0_dgrad((const float*)ws, w0, d_x, shape->n, shape->in_ch, shape->h, shape->w, st);
  return launch_ok("node_stem_conv0_dgrad");
}

size_t node_stem_conv_workspace_bytes(const node_conv_geom* g) {
  if (check_geom(g) != NODE_OK) return 0;
  return make_one(g, nullptr).bytes;
}

int node_stem_conv(const node_conv_geom* g, int what, const float* x, const float* w, const float* dy, float* result, void* ws,
                   size_t ws_bytes, void* stream) {
  w4_refresh_tuning();     // (NODE_TUNE_W4_*: once per call)
  int rc = check_geom(g);
  if (rc != NODE_OK) return rc;
  if (!result || !ws || (what != 1 && !x) || (what != 2 && !w) || (what != 0 && !dy)) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  OnePlan p = make_one(g, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int XHW = g->x_h * g->x_w, YHW = p.YH * p.YW;
  SPrepArgs pa;
  memset(&pa, 0, sizeof(pa));
  if (what != 2) { pa.job[0] = {w, p.f.wf, p.f.wd, g->cout, g->cin, g->k * g->k}; pa.njobs = 1; }
  pa.zero[0] = p.xin.p + (size_t)p.xin.rows * p.xin.C; pa.zero_plane[0] = p.xin.plane; pa.zero_c[0] = p.xin.C;
  pa.zero[1] = p.dyt.p + (size_t)p.dyt.rows * p.dyt.C; pa.zero_plane[1] = p.dyt.plane; pa.zero_c[1] = p.dyt.C;
  pa.nzero = 2;
  launch_stem_prep(pa, st);
  if (what == 0) {
    launch_stem_from_nchw(x, nullptr, p.xin.p, p.xin.plane, g->n, g->cin, XHW, st);
    launch_stem_conv(conv_fwd_args(p.xin, p.f, p.resn, g->n, g->x_h, g->x_w, p.YH, p.YW, g->k, g->stride, g->pad), st);
    launch_stem_to_nchw(p.resn, result, g->n, g->cout, YHW, st);
  } else if (what == 1) {
    launch_stem_from_nchw(dy, nullptr, p.dyt.p, p.dyt.plane, g->n, g->cout, YHW, st);
    SConvArgs c = conv_dgrad_args(p.dyt, p.f, p.resn, g->n, p.YH, p.YW, g->x_h, g->x_w, g->k, g->stride, g->pad);
    if (g->k == 1 && g->stride == 2) {   // pixels no tap reaches keep a zero gradient
      if (hipMemsetAsync(p.resn, 0, (size_t)g->n * XHW * g->cin * sizeof(float), st) != hipSuccess) return fail(NODE_ERR_HIP, "memset failed");
    }
    launch_stem_conv(c, st);
    launch_stem_to_nchw(p.resn, result, g->n, g->cin, XHW, st);
  } else {
    launch_stem_from_nchw(x, nullptr, p.xin.p, p.xin.plane, g->n, g->cin, XHW, st);
    launch_stem_from_nchw(dy, nullptr, p.dyt.p, p.dyt.plane, g->n, g->cout, YHW, st);
    launch_stem_wgrad(wgrad_args(p.dyt, nullptr, p.xin, p.wg, g->n, g->x_h, g->x_w, p.YH, p.YW, g->cin, g->cout, g->k, g->stride, g->pad), st);
    SReduceArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.job[0] = {p.wg.slab, result, nullptr, 0, p.wg.nsplit, g->cout, g->cin, g->k * g->k};
    ra.njobs = 1;
    launch_stem_reduce(ra, st);
  }
  return launch_ok("node_stem_conv");
}

}  // extern "C"
