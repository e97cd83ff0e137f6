// The workspace layout of a fused solve, and the argument checks that the solve entry points share.
#pragma once
#include "host_common.h"
#include "wino4.h"

namespace node {

struct Plan {
  // common
  Ctrl* ctrl;
  float* partial[3];        // [ERR_BLOCKS][2] each
  float* wf[2];             // packed forward weights
  float* wd[2];             // packed dgrad weights (adjoint)
  float* tmap[2];
  float *Y, *Y1, *KY[7];
  float *act1, *act2;
  float* RAW;               // split-conv / small mode: the conv's raw output, consumed by the GroupNorm pass
  float* wsmall[2];         // small mode: filters packed for k_conv3x3_small
  unsigned short* wtiny[2]; // latency path (kernels_tiny.hip): filters as column-padded bf16 triples in fragment order
  float* tpart;             //   K-slice partial sums
  unsigned* tcount;         //   arrival counters [N G]
  void* thand;              // resident form (kernels_tiny_solve.hip): hand-off buffers of tagged words (activations, partial sums, decisions)
  float *W4V, *W4M;         // F(4x4,3x3) pipeline: the current conv's row operand and component products (wino4.h)
  float* w4u[4];            // its filter operands: forward conv1 / conv2, data gradient conv1 / conv2
  unsigned short* w4ub[4];  // the same as exact bf16 triples (k_w4_gemm64b)
  float* tmapS[2];          // the border maps in the W4S blocking (kernels_w4s.hip)
  W4Scales* w4sc;           // power-of-two scales of the fp16-pair operands (wino4.h)
  float* W4Va0b;            // second copy of W4Va[0]: the pass that ends an evaluation writes the NEXT one's conv-1 operand into the set
                            // this evaluation's weight gradient does not read (Solver::va0_of).  On one stream the weight gradient is
                            // enqueued in front of that pass; whether one copy would do is open
  float *W4Va[2], *W4Z[2], *W4dU;   // F(4x4,3x3)-domain weight gradient (C % 128 == 0): the forward convs' row operands
                                    // kept until it runs, Z = A dz A^T of both conv outputs' cotangents, the gradients
  float *act1b, *xh1b, *r1b;   // second set of GroupNorm-1's saved tensors: the pass that ends evaluation s also forms
                               // stage s + 1's conv input, while evaluation s's own set is still being read
  // adjoint
  float *A, *A1, *KA[7];
  float *TH, *TH1, *KT[7];
  float *xh1, *xh2, *xh3, *r1, *r2, *r3;
  float *dz1, *dz2, *G;
  float *wpart[2], *spart[2], *gpart[3], *sred, *wtime[2];
  float* dots;              // [n_t] time vjps scratch
  // device-resident stepping
  double* targets;          // [n_t] output times of the current interval (solver orientation)
  double* forced;           // [STEP_LIST_CAP] replay-mode step sizes
  double* dtlog;            // [STEP_LIST_CAP] dt tried per step of the current interval (negative: rejected)
  size_t bytes;
};
constexpr int STEP_LIST_CAP = 4096;   // replay lists / dt logs longer than this are refused / truncated

// the layout for (geometry, adjoint, number of time points); base == nullptr: sizes only (Plan::bytes)
Plan make_plan(const Dims& d, int adjoint, int n_t, void* base);

// ----------------------------------------------------------------------------
// argument checks of the solve entry points
// ----------------------------------------------------------------------------
// shape, parameter pointers and workspace of one solve -> its geometry and its plan
int check_common(const node_shape* shape, const node_params* params, void* ws, size_t ws_bytes, int adjoint, int n_t,
                 Dims* d, Plan* plan);
int check_method(int method);
int check_times(const float* t_pts, int n_t);

// What node_solve_opts asks of a solve, decoded once for node_solve_fwd and node_solve_adjoint.
struct SolveCtl {
  bool forced;           // replay mode: dopri5 with a list of recorded step sizes
  int n_forced;
  long long max_steps;
  int log_cap;           // > 0: dt log wanted (at most STEP_LIST_CAP entries)
  int blind;             // > 0: deferred completion -- exactly this many steps, no read-back (node_solve_opts::blind_steps)
};
// check_method, check_times, check_common and the replay-list limit, in the order the ABI reports them; then the decoding
int check_solve(const node_shape* shape, const node_params* params, void* ws, size_t ws_bytes, int adjoint, const float* t_pts,
                int n_t, int method, const node_solve_opts* opts, Dims* d, Plan* plan, SolveCtl* ctl);
// the return value (and error text) of a solve that ended with device status `status`; `dt`: its last step size
int solve_rc(int status, double dt);

}  // namespace node
