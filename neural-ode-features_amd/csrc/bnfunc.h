// The `norm='batch'` dynamics on the host side: the workspace plan of one evaluation and its NHWC-to-NHWC launch sequences,
// shared by bnfunc_api.hip (one evaluation per call, NCHW at the boundary) and bnsolve_api.hip (a whole solve, the state in
// this layout from the first stage to the last, the parameters prepared once).
#pragma once
#include "host_common.h"
#include "batchnorm.h"
#include "stem_plan.h"

namespace node {

struct BnPlan {
  int N, C, H, W, R, cr, nchunk;
  float eps;
  Filt c1, c2;
  float *T1, *T2;
  float *xh, *h1, *h2, *y;
  Trip a1, a2;
  float *part, *stats1, *stats2, *stats3;
  // backward
  float *gf, *da, *clsp1, *clsp2;
  double *gpart, *dtp1, *dtp2;
  Trip dht;
  Wg w1, w2;
  size_t bytes;
};
// boundary = false: the plan of a whole solve, whose evaluations read and write the caller's NHWC tensors -- no xh, and y (= gf)
// only with keep
BnPlan make_bn_plan(const node_bnfunc_shape* sh, bool keep, void* base, bool boundary = true);
int check_bn_shape(const node_bnfunc_shape* sh);
int check_bn_tensors(const void* s, const char* what);     // node_bnfunc_params / node_bnfunc_grads: ten non-NULL, 16-byte aligned pointers

// once per parameter version: both filters -> triples, the time tables, the zero rows of the triples tensors
int bn_prepare(const BnPlan& p, const node_bnfunc_params* prm, bool keep, hipStream_t st);
// out = out_scale * f(t, x): x, out fp32 NHWC, t a device scalar.  Leaves in the plan what bn_eval_bwd reads; x must stay as it is
// until that backward has run (norm1's backward reads it again).
int bn_eval_fwd(const BnPlan& p, const node_bnfunc_params* prm, const float* t, const float* x, float* out, float out_scale, hipStream_t st);
// the vector-Jacobian product of the evaluation before it with the cotangent da_scale * da (fp32 NHWC): grads (nullable: all ten or
// none), dx (fp32 NHWC; written when want_dx or grads), d_t (nullable device scalar).  da is only read; dx may be da.
int bn_eval_bwd(const BnPlan& p, const node_bnfunc_params* prm, const float* t, const float* x, const float* da, float da_scale,
                const node_bnfunc_grads* grads, float* dx, bool want_dx, float* d_t, hipStream_t st);

}  // namespace node
