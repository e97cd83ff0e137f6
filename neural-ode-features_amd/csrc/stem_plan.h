// Host-side building blocks shared by the plans of the stem's kernel family (stem_api.hip: the residual stem;
// trunk_api.hip: the ResNet baseline's residual trunk): workspace pieces (triples, filters, split-K slabs) and the
// geometry -> kernel-argument helpers of kernels_stem.hip.
#pragma once
#include "host_common.h"
#include "stem.h"
#include <cstring>

namespace node {

struct Trip {            // a triples tensor [3][rows + 1][C]
  bf16_t* p;
  size_t plane;
  int rows, C;
};
inline Trip take_trip(Bump& b, int rows, int C) {
  Trip t;
  t.rows = rows; t.C = C;
  t.plane = (size_t)(rows + 1) * C;
  t.p = b.take<bf16_t>(3 * t.plane);
  return t;
}
struct Filt {            // a filter as triples in both operand layouts
  bf16_t* wf; bf16_t* wd;
  size_t plane;
  int Cout, Cin, taps;
};
inline Filt take_filt(Bump& b, int Cout, int Cin, int taps) {
  Filt f;
  f.Cout = Cout; f.Cin = Cin; f.taps = taps;
  f.plane = (size_t)taps * Cout * Cin;
  f.wf = b.take<bf16_t>(3 * f.plane);
  f.wd = b.take<bf16_t>(3 * f.plane);
  return f;
}
struct Wg {              // split-K plan + slabs of one weight gradient
  int nsplit, rps;
  float* slab; float* slab2;
};
inline Wg take_wg(Bump& b, int rows, int Cout, int Cin, int taps, bool extra) {
  // workgroups = (64 x 64 tiles) x (kernel rows) x splits: aim at ~1.5 workgroups per CU, shares of >= 64 pixels,
  // and keep the slabs (written once, read once by k_stem_reduce) under ~16 MB
  Wg w;
  const int pairs = (Cout / 64) * (Cin / 64) * stem_wgrad_rows(taps);
  int ns = (384 + pairs - 1) / pairs;
  if (ns > rows / 64) ns = rows / 64;
  const size_t per = (size_t)(taps + (extra ? 1 : 0)) * Cout * Cin * sizeof(float);
  while (ns > 4 && ns * per > ((size_t)16 << 20)) ns = (ns + 1) / 2;
  if (ns < 1) ns = 1;
  int rps = (rows + ns - 1) / ns;
  rps = (rps + 15) & ~15;
  w.rps = rps;
  w.nsplit = (rows + rps - 1) / rps;
  w.slab = b.take<float>((size_t)w.nsplit * taps * Cout * Cin);
  w.slab2 = extra ? b.take<float>((size_t)w.nsplit * Cout * Cin) : nullptr;
  return w;
}

// ---------------------------------------------------------------------------------------------------------------
// geometry -> SConvArgs
// ---------------------------------------------------------------------------------------------------------------
inline void set_single_class(SConvArgs& a, int taps) {
  a.nclass = 1; a.step = 1;
  a.cls_py[0] = a.cls_px[0] = 0;
  a.cls_h[0] = a.OH; a.cls_w[0] = a.OW;
  a.cls_ntap[0] = taps;
  a.cls_taps[0] = 0;
  for (int t = 0; t < taps; ++t) a.cls_taps[0] |= (unsigned long long)t << (4 * t);
  a.cls_tile0[0] = 0;
  a.cls_tile0[1] = (a.N * a.OH * a.OW + 127) / 128;
}
// forward convolution: in = activation triples [N, IH, IW, Cin], out [N, OH, OW, Cout]
inline SConvArgs conv_fwd_args(const Trip& in, const Filt& f, float* out, int N, int IH, int IW, int OH, int OW, int k, int stride, int pad) {
  SConvArgs a;
  memset(&a, 0, sizeof(a));
  a.in = in.p; a.in_plane = in.plane; a.zero_row = in.rows;
  a.w = f.wf; a.w_plane = f.plane;
  a.out = out;
  a.N = N; a.IH = IH; a.IW = IW; a.OH = OH; a.OW = OW; a.Cin = f.Cin; a.Cout = f.Cout;
  a.KH = a.KW = k; a.sshift = stride == 2 ? 1 : 0; a.pad = pad; a.mode = 0;
  set_single_class(a, k * k);
  return a;
}
// data gradient: in = dy triples [N, YH, YW, Cout_f], out = dx [N, XH, XW, Cin_f]
inline SConvArgs conv_dgrad_args(const Trip& dy, const Filt& f, float* dx, int N, int YH, int YW, int XH, int XW, int k, int stride, int pad) {
  SConvArgs a;
  memset(&a, 0, sizeof(a));
  a.in = dy.p; a.in_plane = dy.plane; a.zero_row = dy.rows;
  a.w = f.wd; a.w_plane = f.plane;
  a.out = dx;
  a.N = N; a.IH = YH; a.IW = YW; a.OH = XH; a.OW = XW; a.Cin = f.Cout; a.Cout = f.Cin;
  a.KH = a.KW = k; a.sshift = stride == 2 ? 1 : 0; a.pad = pad; a.mode = 1;
  if (stride == 1) {
    set_single_class(a, k * k);
    return a;
  }
  // stride 2: one class per (row parity, column parity) of the pixel written; its taps are those with (o + pad - k) even
  a.step = 2;
  int nc = 0, tiles = 0;
  for (int py = 0; py < 2; ++py)
    for (int px = 0; px < 2; ++px) {
      int nt = 0, taps[16];
      for (int ky = 0; ky < k; ++ky)
        for (int kx = 0; kx < k; ++kx)
          if (((py + pad - ky) & 1) == 0 && ((px + pad - kx) & 1) == 0) taps[nt++] = ky * k + kx;
      const int ch = (XH - py + 1) / 2, cw = (XW - px + 1) / 2;
      if (nt == 0 || ch <= 0 || cw <= 0) continue;
      a.cls_py[nc] = py; a.cls_px[nc] = px; a.cls_h[nc] = ch; a.cls_w[nc] = cw;
      a.cls_ntap[nc] = nt;
      a.cls_taps[nc] = 0;
      for (int t = 0; t < nt; ++t) a.cls_taps[nc] |= (unsigned long long)taps[t] << (4 * t);
      a.cls_tile0[nc] = tiles;
      tiles += (N * ch * cw + 127) / 128;
      ++nc;
    }
  a.nclass = nc;
  a.cls_tile0[nc] = tiles;
  return a;
}
inline SWgradArgs wgrad_args(const Trip& dy, const Trip* dy2, const Trip& in, const Wg& w, int N, int IH, int IW, int OH, int OW, int Cin,
                      int Cout, int k, int stride, int pad) {
  SWgradArgs a;
  memset(&a, 0, sizeof(a));
  a.dy3 = dy.p; a.dy_plane = dy.plane; a.dy_zero_row = dy.rows;
  a.dy23 = dy2 ? dy2->p : nullptr;
  a.in = in.p; a.in_plane = in.plane; a.zero_row = in.rows;
  a.slab = w.slab; a.slab2 = w.slab2;
  a.N = N; a.IH = IH; a.IW = IW; a.OH = OH; a.OW = OW; a.Cin = Cin; a.Cout = Cout; a.KH = a.KW = k; a.stride = stride; a.pad = pad;
  a.nsplit = w.nsplit; a.rows_per_split = w.rps;
  return a;
}
inline SGnArgs gn_args(const float* h, const float* gamma, const float* beta, float* stats, int N, int HW, int C, float eps) {
  SGnArgs a;
  memset(&a, 0, sizeof(a));
  a.h = h; a.gamma = gamma; a.beta = beta; a.stats = stats;
  a.N = N; a.HW = HW; a.C = C; a.cpg = C / (C < 32 ? C : 32); a.eps = eps;
  a.CB = stem_gn_cb(HW, C, a.cpg);
  return a;
}

// what launch_stem_gn_fwd / launch_stem_gn_bwd make of gn_args(.., N, HW, C, ..): the record of node_stem_describe / node_trunk_describe
inline node_stem_gn_info gn_info(int N, int HW, int C) {
  const SGnArgs a = gn_args(nullptr, nullptr, nullptr, nullptr, N, HW, C, 0.f);
  node_stem_gn_info i;
  i.hw = a.HW; i.channels = a.C; i.cpg = a.cpg; i.cb = a.CB;
  i.blocks_per_sample = a.C / a.CB;
  i.grid = a.N * (a.C / a.CB);
  return i;
}

inline int launch_ok(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
  return NODE_OK;
}

}  // namespace node
