// C ABI of a whole solve of the `norm='batch'` dynamics (include/node_hip.h: node_bnsolve_fwd / node_bnsolve_adjoint): the
// structure of generic.solve_forward / solve_adjoint on the host side of this library, around the NHWC-to-NHWC evaluations of
// bnfunc_api.hip (bn_eval_fwd / bn_eval_bwd) and the step controller of api_flat.hip (node_flat_*: every kernel in it is
// elementwise or a whole-tensor norm, so it does not care that the flat state is an NHWC tensor).
//
//   - the state stays NHWC from the first stage to the last: NCHW <-> NHWC once per solve, batched over the time slices;
//   - k_bn_prep runs once per solve: the parameters cannot change inside one;
//   - an evaluation writes tsign * f, tsign * vjp_y(-a), tsign * vjp_theta(-a) STRAIGHT into stage-derivative slot k[j] of the
//     segments (out_scale = tsign, da_scale = -tsign: the gradient is linear in the cotangent; the ten parameter gradients go
//     through a node_bnfunc_grads whose pointers are the parameters() offsets inside the adj_params slot) and tsign * vjp_t(-a)
//     into the controller's scalar (launch_flat_scalar).  No copy, no sign pass.
//
// The host takes no step decision: it enqueues `steps_hint` steps (then two at a time), reads the controller back, and repeats
// until the controller says done.  Steps enqueued past the end of an interval run their kernels on states the commit discards.
#include "bnfunc.h"
#include <cstring>

using namespace node;

namespace {

constexpr int MAX_T = 1024;      // time points of one call (STEP_LIST_CAP bounds the targets of an interval as well)

struct SolvePlan {
  BnPlan bn;
  int nseg;
  size_t n[3];
  float *y[3], *y1[3], *stage[3], *k[3][7];
  size_t poff[10];               // parameters() offsets inside the adj_params segment
  float *t_stage, *t_i, *dt_tmp, *dot_out;
  double* dot_part;
  float* slices;                 // forward: NHWC outputs [n_t - 1][RC]; adjoint: the trajectory's slices 1 .. n_t - 1
  float* gslices;                // adjoint: the output gradient's slices as NHWC ([n_t], or one with grad_last_only)
  void* flat_ws;
  size_t flat_bytes, bytes;
};

SolvePlan make_plan(const node_bnfunc_shape* sh, bool adjoint, int n_t, int n_grad, void* base) {
  SolvePlan s;
  memset(&s, 0, sizeof(s));
  s.bn = make_bn_plan(sh, adjoint, base, false);      // (no NCHW boundary per evaluation: no xh; y only where the adjoint evaluates f(t_i, y_i))
  const size_t off0 = (s.bn.bytes + 255) & ~(size_t)255;
  Bump b(base ? (char*)base + off0 : nullptr);
  const size_t C = (size_t)s.bn.C, RC = (size_t)s.bn.R * C;
  const size_t sizes[10] = {C, C, C * (C + 1) * 9, C, C, C, C * (C + 1) * 9, C, C, C};
  size_t P = 0;
  for (int i = 0; i < 10; ++i) { s.poff[i] = P; P += sizes[i]; }
  s.nseg = adjoint ? 3 : 1;
  s.n[0] = RC; s.n[1] = RC; s.n[2] = P;
  for (int i = 0; i < s.nseg; ++i) {
    s.y[i] = b.take<float>(s.n[i]);
    s.y1[i] = b.take<float>(s.n[i]);
    s.stage[i] = b.take<float>(s.n[i]);
    for (int j = 0; j < 7; ++j) s.k[i][j] = b.take<float>(s.n[i]);
  }
  s.t_stage = b.take<float>(1);
  s.t_i = b.take<float>(1);
  s.dt_tmp = b.take<float>(1);
  s.dot_out = b.take<float>(1);
  s.dot_part = b.take<double>(BN_DOT_BLOCKS);
  s.slices = b.take<float>((size_t)(n_t - 1) * RC);
  if (adjoint) s.gslices = b.take<float>((size_t)n_grad * RC);
  s.flat_bytes = node_flat_workspace_bytes(n_t - 1);
  s.flat_ws = b.take<char>(s.flat_bytes);
  s.bytes = off0 + b.off + 256;
  return s;
}

int check_method(int method) {
  if (method != NODE_METHOD_DOPRI5 && method != NODE_METHOD_RK4) return fail(NODE_ERR_ARG, "unknown method %d (dopri5 = 0, rk4 = 1)", method);
  return NODE_OK;
}
int check_grid(const float* t, int n_t) {
  if (n_t < 2 || n_t > MAX_T) return fail(NODE_ERR_ARG, "n_t must be 2..%d (got %d)", MAX_T, n_t);
  if (!t) return fail(NODE_ERR_NULL, "t_pts is NULL (a host array)");
  const bool inc = t[1] > t[0];
  for (int i = 1; i < n_t; ++i)
    if (!(inc ? t[i] > t[i - 1] : t[i] < t[i - 1])) return fail(NODE_ERR_ARG, "t_pts must be strictly increasing or strictly decreasing");
  return NODE_OK;
}
// every slice of a call together stays under 2^31 elements: the boundary's layout launches take n_t * n samples at once
int check_slices(const node_bnfunc_shape* sh, int n_t) {
  if (n_t < 2 || n_t > MAX_T) return fail(NODE_ERR_ARG, "n_t must be 2..%d (got %d)", MAX_T, n_t);
  const size_t elems = (size_t)sh->n * sh->h * sh->w * sh->channels;
  if (elems * (size_t)n_t >= ((size_t)1 << 31))
    return fail(NODE_ERR_UNSUPPORTED, "the %d slices of a batch-norm solve must stay under 2^31 elements together (%zu each)", n_t, elems);
  return NODE_OK;
}
int check_dev(const void* p, const char* what) {
  if (!p) return fail(NODE_ERR_NULL, "%s is NULL", what);
  if (((uintptr_t)p) & 15) return fail(NODE_ERR_ARG, "%s must be 16-byte aligned", what);
  return NODE_OK;
}
int check_ws(const void* ws) {
  if (!ws) return fail(NODE_ERR_NULL, "workspace is NULL");
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  return NODE_OK;
}

struct Driver {
  const SolvePlan* sp;
  const node_bnfunc_params* prm;
  node_flat_solve fs;
  hipStream_t st;
  bool adjoint;
  int max_steps, hint;
  long nfe;
  node_flat_status last;

  void init(const SolvePlan& s, const node_bnfunc_params* p, float rtol, float atol, bool adj, const node_bnsolve_opts* o, hipStream_t stream) {
    sp = &s; prm = p; st = stream; adjoint = adj; nfe = 0;
    memset(&last, 0, sizeof(last));
    max_steps = (o && o->max_num_steps > 0) ? o->max_num_steps : 0x7fffffff;
    hint = (o && o->steps_hint > 0) ? o->steps_hint : 1;
    memset(&fs, 0, sizeof(fs));
    fs.nseg = s.nseg; fs.has_scalar = adj ? 1 : 0;
    for (int i = 0; i < s.nseg; ++i) {
      fs.seg[i].y = s.y[i]; fs.seg[i].y1 = s.y1[i]; fs.seg[i].n = s.n[i];
      for (int j = 0; j < 7; ++j) fs.seg[i].k[j] = s.k[i][j];
    }
    fs.rtol = rtol; fs.atol = atol; fs.tsign = 1.f;
    fs.n_targets = 1;
    fs.ws = s.flat_ws; fs.ws_bytes = s.flat_bytes;
  }

  // the dynamics (and, in the adjoint, their vector-Jacobian product with -a) at *t_stage / `states` -> slot k[kslot], times tsign
  int evaluate(int kslot, float* const* states) {
    const float tsign = fs.tsign;
    TRY(bn_eval_fwd(sp->bn, prm, sp->t_stage, states[0], sp->k[0][kslot], tsign, st));
    ++nfe;
    if (!adjoint) return NODE_OK;
    float* base = sp->k[2][kslot];
    node_bnfunc_grads g;
    float** gp = reinterpret_cast<float**>(&g);
    for (int i = 0; i < 10; ++i) gp[i] = base + sp->poff[i];
    TRY(bn_eval_bwd(sp->bn, prm, sp->t_stage, states[0], states[1], -tsign, &g, sp->k[1][kslot], true, sp->dt_tmp, st));
    return node_flat_scalar(&fs, kslot, sp->dt_tmp, 1.0f, 0, st);
  }
  int stage_eval(int method, int stage, int kslot, bool into_y1) {
    if (stage == NODE_FLAT_F0) {
      TRY(node_flat_stage(&fs, method, stage, nullptr, sp->t_stage, st));
      return evaluate(kslot, sp->y);
    }
    float* const* dst = into_y1 ? sp->y1 : sp->stage;
    TRY(node_flat_stage(&fs, method, stage, dst, sp->t_stage, st));
    return evaluate(kslot, dst);
  }
  // one rk4 step (3/8 rule) over the interval that node_flat_begin set
  int rk4_step() {
    TRY(stage_eval(NODE_METHOD_RK4, NODE_FLAT_F0, 0, false));
    for (int s = 1; s <= 3; ++s) TRY(stage_eval(NODE_METHOD_RK4, s, s, false));
    return node_flat_finish_step(&fs, NODE_METHOD_RK4, nullptr, st);
  }
  // f0 (the FSAL seed), Hairer's initial step with its probe evaluation, then dopri5 steps until the controller says done.
  // Returns NODE_OK or the status that stopped the solve; `last` holds the controller as read back last.
  int dopri5_interval(float* y_out) {
    const int D = NODE_METHOD_DOPRI5;
    TRY(stage_eval(D, NODE_FLAT_F0, 0, false));
    TRY(node_flat_initial_step(&fs, 0, st));
    TRY(stage_eval(D, NODE_FLAT_PROBE, 1, false));
    TRY(node_flat_initial_step(&fs, 1, st));
    long enq = 0;
    int batch = hint;
    for (;;) {
      if ((long)batch > (long)max_steps - enq) batch = (int)((long)max_steps - enq);
      for (int b = 0; b < batch; ++b) {
        for (int s = 0; s < 6; ++s) TRY(stage_eval(D, s, s + 1, s == 5));
        TRY(node_flat_finish_step(&fs, D, y_out, st));
      }
      enq += batch;
      TRY(node_flat_status_read(&fs, &last, st));
      if (last.status != 0) {
        nfe -= 6 * (enq - last.steps);
        return status_fail(last.status, last.dt);
      }
      if (last.done) {
        nfe -= 6 * (enq - last.steps);      // the steps enqueued past the end ran on discarded states: not the solver's evaluations
        return NODE_OK;
      }
      if (enq >= max_steps) return status_fail(NODE_ERR_MAX_STEPS, last.dt);
      batch = 2;
    }
  }
  static int status_fail(int status, double dt) {
    if (status == NODE_ERR_MAX_STEPS) return fail(status, "max_num_steps exceeded");
    if (status == NODE_ERR_NONFINITE) return fail(status, "non-finite error norm / state");
    if (status == NODE_ERR_DT_UNDERFLOW) return fail(status, "underflow in dt %g", dt);
    return fail(status, "solver status %d", status);
  }
  void fill(node_stats* stats, int status) const {
    if (!stats) return;
    stats->nfe = (int32_t)nfe; stats->accepted = last.accepted; stats->rejected = last.rejected; stats->status = status;
    stats->last_dt = last.dt; stats->t_final = last.t; stats->first_dt = last.first_dt;
  }
};

double f32(double v) { return (double)(float)v; }

}  // namespace

extern "C" {

size_t node_bnsolve_workspace_bytes(const node_bnfunc_shape* shape, int method, int adjoint, int n_t) {
  if (check_bn_shape(shape) != NODE_OK || check_method(method) != NODE_OK || check_slices(shape, n_t) != NODE_OK) return 0;
  return make_plan(shape, adjoint != 0, n_t, n_t, nullptr).bytes;
}

int node_bnsolve_fwd(const node_bnfunc_shape* shape, const node_bnfunc_params* prm, const float* y0, const float* t_pts, int n_t,
                     float rtol, float atol, int method, const node_bnsolve_opts* opts, float* y_out, node_stats* stats, void* ws,
                     size_t ws_bytes, void* stream) {
  TRY(check_bn_shape(shape));
  TRY(check_method(method));
  TRY(check_bn_tensors(prm, "params"));
  TRY(check_grid(t_pts, n_t));
  TRY(check_slices(shape, n_t));
  TRY(check_dev(y0, "y0"));
  TRY(check_dev(y_out, "y_out"));
  TRY(check_ws(ws));
  const SolvePlan sp = make_plan(shape, false, n_t, 0, ws);
  if (ws_bytes < sp.bytes) return fail(NODE_ERR_WORKSPACE, "bnsolve workspace too small: %zu < %zu", ws_bytes, sp.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int N = sp.bn.N, C = sp.bn.C, HW = sp.bn.H * sp.bn.W;
  const size_t RC = sp.n[0];
  const double tsign = t_pts[1] < t_pts[0] ? -1.0 : 1.0;
  Driver d;
  d.init(sp, prm, rtol, atol, false, opts, st);
  d.fs.tsign = (float)tsign;

  // everything that launches: whatever way it ends, `stats` is filled behind it
  auto run = [&]() -> int {
    TRY(bn_prepare(sp.bn, prm, false, st));
    launch_stem_from_nchw(y0, sp.y[0], nullptr, 0, N, C, HW, st);
    TRY(launch_ok("stem_from_nchw"));
    HIP_TRY(hipMemcpyAsync(y_out, y0, RC * sizeof(float), hipMemcpyDeviceToDevice, st));      // out[0] = y0, bit for bit
    if (method == NODE_METHOD_RK4) {
      for (int j = 1; j < n_t; ++j) {
        const double t0 = f32(tsign * t_pts[j - 1]), t1 = f32(tsign * t_pts[j]);
        TRY(node_flat_begin(&d.fs, t0, &t1, f32(t1 - t0), j == 1, st));
        TRY(d.rk4_step());
        launch_stem_to_nchw(sp.y[0], y_out + (size_t)j * RC, N, C, HW, st);
        TRY(launch_ok("stem_to_nchw"));
        d.last.accepted = j; d.last.t = t1; d.last.dt = t1 - t0;
        if (j == 1) d.last.first_dt = t1 - t0;
      }
      return NODE_OK;
    }
    double targets[MAX_T];
    for (int j = 1; j < n_t; ++j) targets[j - 1] = tsign * (double)t_pts[j];
    d.fs.n_targets = n_t - 1;
    TRY(node_flat_begin(&d.fs, tsign * (double)t_pts[0], targets, 0.0, 1, st));
    TRY(d.dopri5_interval(sp.slices));
    launch_stem_to_nchw(sp.slices, y_out + RC, N * (n_t - 1), C, HW, st);      // every slice in one launch: the layouts differ per sample only
    return launch_ok("stem_to_nchw");
  };
  const int rc = run();
  d.fill(stats, rc);
  return rc;
}

int node_bnsolve_adjoint(const node_bnfunc_shape* shape, const node_bnfunc_params* prm, const float* y_traj, const float* grad_out,
                         const float* t_pts, int n_t, float rtol, float atol, int method, const node_bnsolve_opts* opts, float* grad_y0,
                         const node_bnfunc_grads* grad_params, node_stats* stats, void* ws, size_t ws_bytes, void* stream) {
  TRY(check_bn_shape(shape));
  TRY(check_method(method));
  TRY(check_bn_tensors(prm, "params"));
  if (grad_params) TRY(check_bn_tensors(grad_params, "grad_params"));
  TRY(check_grid(t_pts, n_t));
  TRY(check_slices(shape, n_t));
  TRY(check_dev(y_traj, "y_traj"));
  TRY(check_dev(grad_out, "grad_out"));
  TRY(check_dev(grad_y0, "grad_y0"));
  TRY(check_ws(ws));
  const bool last_only = opts && opts->grad_last_only;
  const SolvePlan sp = make_plan(shape, true, n_t, n_t, ws);       // (the query does not know grad_last_only: room for every slice)
  if (ws_bytes < sp.bytes) return fail(NODE_ERR_WORKSPACE, "bnsolve workspace too small: %zu < %zu", ws_bytes, sp.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int N = sp.bn.N, C = sp.bn.C, HW = sp.bn.H * sp.bn.W;
  const size_t RC = sp.n[0];
  Driver d;
  d.init(sp, prm, rtol, atol, true, opts, st);
  // gradient slice i as NHWC, or NULL where grad_last_only declares it zero
  auto gslice = [&](int i) -> const float* {
    if (last_only) return i == n_t - 1 ? sp.gslices : nullptr;
    return sp.gslices + (size_t)i * RC;
  };

  // everything that launches: whatever way it ends, `stats` is filled behind it
  auto run = [&]() -> int {
    TRY(bn_prepare(sp.bn, prm, true, st));
    // the trajectory's slices 1 .. n_t - 1 and the output gradient's slices -> NHWC, one launch each
    launch_stem_from_nchw(y_traj + RC, sp.slices, nullptr, 0, N * (n_t - 1), C, HW, st);
    TRY(launch_ok("stem_from_nchw"));
    launch_stem_from_nchw(grad_out, sp.gslices, nullptr, 0, N * (last_only ? 1 : n_t), C, HW, st);
    TRY(launch_ok("stem_from_nchw"));
    HIP_TRY(hipMemcpyAsync(sp.y[1], gslice(n_t - 1), RC * sizeof(float), hipMemcpyDeviceToDevice, st));      // adj_y = grad_out[-1]
    HIP_TRY(hipMemsetAsync(sp.y[2], 0, sp.n[2] * sizeof(float), st));                                         // adj_params = 0
    int rk4_acc = 0;
    for (int i = n_t - 1; i >= 1; --i) {
      const double tsign = t_pts[i - 1] < t_pts[i] ? -1.0 : 1.0;
      d.fs.tsign = (float)tsign;
      const double s0 = tsign * (double)t_pts[i], s1 = tsign * (double)t_pts[i - 1];
      const float* yi = sp.slices + (size_t)(i - 1) * RC;
      HIP_TRY(hipMemcpyAsync(sp.y[0], yi, RC * sizeof(float), hipMemcpyDeviceToDevice, st));
      // adj_t -= <f(t_i, y_i), grad_out_i>: the evaluation counts where the slice is declared zero too (the generic solver runs it)
      const float* gi = gslice(i);
      d.nfe += 1;
      if (gi != nullptr) {
        launch_bn_set_scalar(sp.t_i, t_pts[i], st);
        TRY(launch_ok("bn_set_scalar"));
        TRY(bn_eval_fwd(sp.bn, prm, sp.t_i, yi, sp.bn.y, 1.0f, st));
        launch_bn_dot(sp.bn.y, gi, RC, sp.dot_part, sp.dot_out, st);
        TRY(launch_ok("bn_dot"));
      }
      const bool first = i == n_t - 1;
      if (method == NODE_METHOD_RK4) {
        const double t0 = f32(s0), t1 = f32(s1);
        TRY(node_flat_begin(&d.fs, t0, &t1, f32(t1 - t0), first, st));
        if (gi != nullptr) TRY(node_flat_scalar(&d.fs, -1, sp.dot_out, -1.0f, 1, st));
        TRY(d.rk4_step());
        d.last.accepted = ++rk4_acc; d.last.t = t1; d.last.dt = t1 - t0;
        if (first) d.last.first_dt = t1 - t0;
      } else {
        TRY(node_flat_begin(&d.fs, s0, &s1, 0.0, first, st));
        if (gi != nullptr) TRY(node_flat_scalar(&d.fs, -1, sp.dot_out, -1.0f, 1, st));
        TRY(d.dopri5_interval(nullptr));
      }
      const float* gp = gslice(i - 1);
      if (gp != nullptr) {
        launch_bn_add(sp.y[1], gp, RC, st);        // adj_y += grad_out[i - 1]
        TRY(launch_ok("bn_add"));
      }
    }
    launch_stem_to_nchw(sp.y[1], grad_y0, N, C, HW, st);
    TRY(launch_ok("stem_to_nchw"));
    if (grad_params) {
      const size_t Cs = (size_t)C, wn = Cs * (Cs + 1) * 9;
      const size_t sizes[10] = {Cs, Cs, wn, Cs, Cs, Cs, wn, Cs, Cs, Cs};
      float* const* gp = reinterpret_cast<float* const*>(grad_params);
      for (int k = 0; k < 10; ++k)
        HIP_TRY(hipMemcpyAsync(gp[k], sp.y[2] + sp.poff[k], sizes[k] * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    return NODE_OK;
  };
  const int rc = run();
  d.fill(stats, rc);
  return rc;
}

}  // extern "C"
