// The tiling geometry of a shape: which kernels serve it, with which tiles, and what no kernel is instantiated for.
// Every NODE_TUNE_* switch that moves the geometry is read here.
#include "host_common.h"

#include <cstring>

namespace node {

static int gcd_i(int a, int b) { return b ? gcd_i(b, a % b) : a; }

int dims_for(const node_shape* sh, Dims* out) {
  if (!sh) return fail(NODE_ERR_NULL, "shape is NULL");
  Dims d;
  memset(&d, 0, sizeof(d));
  d.N = sh->n; d.C = sh->c; d.H = sh->h; d.W = sh->w; d.G = sh->groups; d.eps = sh->eps;
  if (d.N <= 0 || d.C <= 0 || d.H <= 0 || d.W <= 0 || d.G <= 0) return fail(NODE_ERR_SHAPE, "non-positive dimension");
  if (d.C % d.G != 0) return fail(NODE_ERR_SHAPE, "groups (%d) must divide channels (%d)", d.G, d.C);
  if (!(d.eps > 0.f)) return fail(NODE_ERR_SHAPE, "eps must be > 0");
  if (d.C % 4 != 0) return fail(NODE_ERR_UNSUPPORTED, "channels (%d) must be a multiple of 4", d.C);
  d.HW = d.H * d.W;
  d.cpg = d.C / d.G;
  d.Wp = d.W + 2; d.Hp = d.H + 2; d.SLOTS = d.Hp * d.Wp; d.MARGIN = d.Wp + 1;
  if (d.cpg > 64) return fail(NODE_ERR_UNSUPPORTED, "channels per group (%d) > 64", d.cpg);
  d.BNE = (64 / d.cpg) * d.cpg;
  d.ntile = (d.C + d.BNE - 1) / d.BNE;
  d.nchunk = (d.C + KCH - 1) / KCH;
  d.csplit = 0;
  // images larger than 256 pixels (the reference's one-shot / ODE stems on 64x64 inputs give 32x32 states, model.py:119-126,
  // 181-196, utils.py:168-195) run the 2-D Winograd conv in bands of 128 pixels (csplit below) with GroupNorm as a pass
  const bool banded = d.HW > 256 && d.HW <= 1024 && d.HW % 128 == 0 && d.H % 2 == 0 && d.W % 2 == 0 && 32 % (d.W / 2) == 0 && d.C % 32 == 0;
  if (d.HW <= 128) d.BM = 128;
  else if (d.HW <= 256) d.BM = 256;
  else if (banded) d.BM = 128;
  else return fail(NODE_ERR_UNSUPPORTED, "H*W = %d > 256: only even-sided images of up to 1024 pixels whose tile rows divide 32 "
                   "(16x16, 32x32, 16x32) with C %% 32 == 0 are tiled", d.HW);
  if (d.HW <= 64) {
    // grids that cannot fill the chip with 128-row tiles (MNIST-sized states, bs=1 census) use 64-row
    // tiles in four-wave workgroups: twice the workgroups (measured [32,64,7,7]: 31 -> 22.6 us).  Once
    // the 128-row grid reaches one workgroup per CU it is the faster one (cfg 2: 91.5 vs 95 us): two
    // co-resident 64-row workgroups run in lockstep and hide nothing of each other.
    const int s128 = 128 / d.HW < d.N ? 128 / d.HW : d.N;
    const long wg128 = (long)((d.N + s128 - 1) / s128) * d.ntile;
    static const int bm_env = env_int("NODE_TUNE_CONV_BM", -1);   // 64 | 128 forces the M tile (tests: the 2-D Winograd kernel on small batches)
    const int force_bm = g_conv_bm > 0 ? g_conv_bm : bm_env;
    const bool want64 = force_bm > 0 ? force_bm == 64 : wg128 < 256;
    if (want64) d.BM = 64;
  }
  if (d.W > 64) return fail(NODE_ERR_UNSUPPORTED, "W = %d > 64", d.W);
  {
    static const int wino_env = env_int("NODE_TUNE_CONV_WINO", -1);
    const int want = g_conv_wino >= 0 ? g_conv_wino : wino_env;
    d.wino = (d.W % 2 == 0) ? (want < 0 ? 2 : want) : 0;   // even widths: Winograd kernels (2-D where the tile fits, else 1-D); odd: direct kernel
    if (d.wino == 2 && !(d.H % 2 == 0 && d.BM == 128 && 128 % d.HW == 0 && d.HW >= 16 && d.C % 32 == 0 &&
                      ((size_t)d.N * d.HW * d.C + d.C) * sizeof(float) < ((size_t)1 << 32)))
      d.wino = 1;   // 2-D variant: whole samples in 32 tiles
    // ... or, for 256-pixel images, two workgroups per sample (32 tiles = whole tile rows = 128 consecutive
    // pixels each) with the GroupNorm as a pointwise pass behind the conv: 16x16 at C = 256 runs the 1-D kernel
    // at 109 algorithmic TFLOP/s (one sample per 256-pixel tile), the 2-D kernel + pass is ~1.5x faster
    if ((want < 0 || want == 2 || banded) && (d.HW == 256 || banded) && d.H % 2 == 0 && d.W % 2 == 0 && 32 % (d.W / 2) == 0 && d.C % 32 == 0 &&
        ((size_t)d.N * d.HW * d.C + d.C) * sizeof(float) < ((size_t)1 << 32)) {
      d.wino = 2;
      d.BM = 128;
      d.csplit = d.HW / 128;
    }
  }
  if (d.HW > 256 && !d.csplit)   // banded geometry whose tensors pass 2^32 bytes: the 128-row tile holds no whole sample (S = 0)
    return fail(NODE_ERR_UNSUPPORTED, "H*W = %d with N*H*W*C = %zu elements: the banded convolution addresses at most 2^32 bytes per tensor",
                d.HW, (size_t)d.N * d.HW * d.C);
  d.S = d.csplit ? 1 : d.BM / d.HW;
  if (d.S > d.N) d.S = d.N;
  while (d.wino != 2 && d.S > 1 && conv_lds_bytes(d, 0) > 150 * 1024) d.S--;
  if (conv_lds_bytes(d, 0) > 160 * 1024) return fail(NODE_ERR_UNSUPPORTED, "conv tile does not fit LDS");
  d.mtiles = d.csplit ? d.N * d.csplit : (d.N + d.S - 1) / d.S;
  {
    // latency regime: the throughput tiles leave most of the chip idle (bs = 1 at C = 256: four workgroups)
    static const int small_env = env_int("NODE_TUNE_SMALL", -1);   // 0 / 1 forces the choice (A/B measurements)
    const bool fits = d.C % 32 == 0 && d.C >= 128 && ((size_t)d.N * d.HW * d.C + d.C) * sizeof(float) < ((size_t)1 << 32);
    // measured at C = 256, 8x8 (tools/latency_bs1.py, us per function evaluation, small / throughput tiles): bs 1: 74.7 /
    // 87.6, bs 4: 99.3 / 90.8, bs 16: 99.3 / 93.0 -- the extra GroupNorm launches cost more than the parallelism
    // buys as soon as the throughput grid has eight workgroups, so only single-digit grids take the small kernel
    d.small = fits && (small_env >= 0 ? small_env != 0 : (long)d.mtiles * d.ntile < 8);
  }
  {
    // latency path (kernels_tiny.hip): forward solves of batches of up to 256 pixels (bs = 1 .. 4 at 8x8, bs = 1 at 16x16).  NODE_TUNE_TINY =
    // 0 never / 1 wherever the geometry fits (A/B measurements, tests); results are fp32-exact products either way
    static const int tiny_env = env_int("NODE_TUNE_TINY", -1);
    d.numel = (size_t)d.N * d.C * d.HW;
    d.tiny = 0;
    if (tiny_env != 0 && (tiny_env == 1 || (size_t)d.N * d.HW <= 256)) d.tiny = tiny_slice_channels(d);
  }
  const int unit = d.cpg / gcd_i(d.cpg, 4) * 4;  // lcm(cpg, 4)
  constexpr int slab_elems = 2048;   // elements of one (sample, channel slab) workgroup of the combine / GN kernels
  int mult = (slab_elems / d.HW) / unit;
  if (mult < 1) mult = 1;
  d.cs = unit * mult;
  if (d.cs > d.C) d.cs = d.C;
  if ((size_t)d.HW * d.cs > 16384) return fail(NODE_ERR_UNSUPPORTED, "GroupNorm slab does not fit LDS");
  d.nslab = (d.C + d.cs - 1) / d.cs;
  {
    // F(4x4,3x3) pipeline (wino4.h): geometry only; a solve uses it when its tolerance allows (Solver::w4)
    // NODE_TUNE_WINO4 = 0 never / 1 by tolerance (default) / 2 wherever the geometry fits.  Read on every call (unlike
    // the other switches) so that one test process can run both conv paths on the same inputs.
    const int w4_env = env_int("NODE_TUNE_WINO4", 1);
    // 16x16 images: four 8x8 quadrants per image (w4q), each a virtual sample of the GEMM-side layouts; the passes
    // hold a GroupNorm group in one workgroup (cpg | 16 or cpg == 32) and only the F(4x4,3x3)-domain weight gradient
    // (C % 128 == 0) is wired behind them
    const bool fit8 = d.H == 8 && d.W == 8 && d.C % 64 == 0 && 16 % d.cpg == 0;
    const bool fit16 = d.H == 16 && d.W == 16 && d.C % 128 == 0 && (16 % d.cpg == 0 || d.cpg == 32);
    d.wino4 = (w4_env != 0 && (fit8 || fit16)) ? w4_env : 0;
    d.w4q = fit16 ? 4 : 1;
    d.N8 = (d.N * d.w4q + 7) & ~7;
  }
  d.RB = 64 / d.W;
  if (d.W >= 32) d.RB = 1;      // (the generic weight-gradient kernel stages RB + 2 rows in registers: 3 x 32 pixels is its limit)
  if (d.RB < 1) d.RB = 1;
  if (d.RB > d.H) d.RB = d.H;
  {
    // weight gradient in the Winograd domain where an instance of k_wgrad_w exists (W % 4 == 0)
    static const int ww_env = env_int("NODE_TUNE_WGRAD_WINO", -1);
    const int want = g_wgrad_wino >= 0 ? g_wgrad_wino : (ww_env >= 0 ? ww_env : 2);
    d.wgrad_wino = 0;
    d.wut = 0;
    if (want && ((d.W == 8 && d.H % 8 == 0) || (d.W == 16 && d.H % 2 == 0) || (d.W == 4 && d.H % 4 == 0))) {
      d.wgrad_wino = 1;
      d.RB = d.W == 8 ? 8 : d.W == 16 ? 2 : 4;
    }
    // 2-D Winograd domain: units of 8 (or 4) tiles that are whole tile rows of one sample
    if (want >= 2 && d.H % 2 == 0 && d.W % 2 == 0 && ((size_t)d.N * d.HW * d.C + 2 * (size_t)d.C * (d.W + 2)) * sizeof(float) < ((size_t)1 << 32)) {
      const int TW = d.W / 2, TPS = (d.H / 2) * TW;
      const int ut = (TPS % 8 == 0 && 8 % TW == 0) ? 8 : (TPS % 4 == 0 && 4 % TW == 0) ? 4 : 0;
      if (ut) { d.wgrad_wino = 2; d.wut = ut; }
    }
  }
  d.nbands = (d.H + d.RB - 1) / d.RB;
  if ((d.RB + 2) * d.W * 16 > 6 * WG_THREADS || d.RB * d.W * 16 > 4 * WG_THREADS)
    return fail(NODE_ERR_UNSUPPORTED, "W = %d: wgrad staging does not fit its registers", d.W);
  if (wgrad_lds_bytes(d) > 160 * 1024) return fail(NODE_ERR_UNSUPPORTED, "wgrad tile does not fit LDS");
  {
    const int U = d.wgrad_wino == 2 ? d.N * ((d.H / 2) * (d.W / 2) / d.wut) : d.N * d.nbands;
    const int ntc = (d.C + 63) / 64;
    // both conv layers' weight gradients go out in ONE launch where the 2-D Winograd kernel serves them
    d.wgrad_pair = d.wgrad_wino == 2 ? 1 : 0;
    int ns = (d.wgrad_pair ? 128 : 256) / (ntc * ntc);   // one workgroup per CU (307 VGPR+AGPR: one wave per SIMD)
    if (ns < 1) ns = 1;
    if (ns > 32) ns = 32;
    if (ns > U) ns = U;
    d.nsplit = ns;
  }
  d.P = 18 * (size_t)d.C * d.C + 26 * (size_t)d.C;
  d.numel = (size_t)d.N * d.C * d.HW;
  *out = d;
  return NODE_OK;
}

}  // namespace node

using namespace node;

extern "C" {

size_t node_param_count(const node_shape* shape) {
  if (!shape) return 0;
  return 18 * (size_t)shape->c * shape->c + 26 * (size_t)shape->c;
}

int node_solve_is_resident(const node_shape* shape) {
  Dims d;
  if (dims_for(shape, &d) != NODE_OK) return 0;
  return d.tiny != 0 && tiny_resident_ok(d) ? 1 : 0;
}

int node_describe_dims(const node_shape* shape, node_dims_info* out) {
  if (!out) return fail(NODE_ERR_NULL, "out is NULL");
  memset(out, 0, sizeof(*out));
  Dims d;
  const int rc = dims_for(shape, &d);
  if (rc != NODE_OK) return rc;
  out->wgrad_kernel = wgrad_kernel_for(d, wgrad_variant());
  out->conv_kernel = conv_kernel_for(d);
  out->wino = d.wino; out->bm = d.BM; out->s = d.S; out->csplit = d.csplit; out->mtiles = d.mtiles; out->ntile = d.ntile;
  out->small = d.small ? 1 : 0; out->tiny = d.tiny; out->wino4 = d.wino4; out->w4q = d.w4q;
  out->wgrad_wino = d.wgrad_wino; out->wut = d.wut; out->rb = d.RB; out->nbands = d.nbands; out->nsplit = d.nsplit;
  out->wgrad_pair = d.wgrad_pair;
  return NODE_OK;
}

}  // extern "C"
