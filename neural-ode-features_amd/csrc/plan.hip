// Workspace layout of a fused solve (Plan) and the argument checks of the solve entry points.
#include "plan.h"

#include <cstring>

namespace node {

Plan make_plan(const Dims& d, int adjoint, int n_t, void* base) {
  Plan p;
  memset(&p, 0, sizeof(p));
  Bump b(base);
  p.ctrl = b.take<Ctrl>(1);
  p.targets = b.take<double>((size_t)(n_t > 0 ? n_t : 1));
  p.forced = b.take<double>(STEP_LIST_CAP);
  p.dtlog = b.take<double>(STEP_LIST_CAP);
  for (int i = 0; i < 3; ++i) p.partial[i] = b.take<float>(ERR_BLOCKS * 2);
  const size_t wsz = conv_packed_elems(d);
  for (int i = 0; i < 2; ++i) p.wf[i] = b.take<float>(wsz);
  for (int i = 0; i < 2; ++i) p.tmap[i] = b.take<float>((size_t)d.HW * d.C);
  p.Y = b.take<float>(d.numel);
  p.Y1 = b.take<float>(d.numel);
  for (int i = 0; i < 7; ++i) p.KY[i] = b.take<float>(d.numel);
  // conv inputs carry a tail of C zeros: the 2-D Winograd kernel reads its zero halo there
  p.act1 = b.take<float>(d.numel + d.C);
  p.act2 = b.take<float>(d.numel + d.C);
  if (d.csplit || d.small) p.RAW = b.take<float>(d.numel);
  if (d.small && !adjoint)
    for (int i = 0; i < 2; ++i) p.wsmall[i] = b.take<float>((size_t)9 * d.C * d.C);
  if (d.tiny && !adjoint) {
    for (int i = 0; i < 2; ++i) p.wtiny[i] = b.take<unsigned short>(tiny_packed_elems(d));
    p.tpart = b.take<float>(tiny_part_elems(d));
    p.tcount = b.take<unsigned>((size_t)d.N * d.G);
    if (tiny_resident_ok(d)) p.thand = b.take<unsigned long long>(tiny_resident_handoff_words(d));
  }
  if (d.wino4) {
    p.W4V = b.take<float>(w4_v_elems(d.N8, d.C));
    p.W4M = b.take<float>(w4_v_elems(d.N8, d.C));
    for (int i = 0; i < (adjoint ? 4 : 2); ++i) p.w4u[i] = b.take<float>(w4_u_elems(d.C));
    for (int i = 0; i < (adjoint ? 4 : 2); ++i) p.w4ub[i] = b.take<unsigned short>(w4_ub_elems(d.C));
    for (int i = 0; i < 2; ++i) p.tmapS[i] = b.take<float>((size_t)d.HW * d.C);
    p.w4sc = b.take<W4Scales>(1);
    if (adjoint && d.C % 128 == 0) {
      for (int i = 0; i < 2; ++i) p.W4Va[i] = b.take<float>(w4_v_elems(d.N8, d.C));
      p.W4Va0b = b.take<float>(w4_v_elems(d.N8, d.C));
      for (int i = 0; i < 2; ++i) p.W4Z[i] = b.take<float>(w4_z_elems(d.N8, d.C));
      p.W4dU = b.take<float>(w4_du_elems(d.C));
    }
    if (adjoint) {
      p.act1b = b.take<float>(d.numel + d.C);
      p.xh1b = b.take<float>(d.numel);
      p.r1b = b.take<float>((size_t)d.N * d.G);
    }
  }
  const size_t prow = d.wino4 ? (size_t)d.N * d.w4q : (size_t)d.N;   // rows of the per-sample partials (F(4x4,3x3) passes: per quadrant)
  if (adjoint) {
    for (int i = 0; i < 2; ++i) p.wd[i] = b.take<float>(wsz);
    p.A = b.take<float>(d.numel);
    p.A1 = b.take<float>(d.numel);
    for (int i = 0; i < 7; ++i) p.KA[i] = b.take<float>(d.numel);
    p.TH = b.take<float>(d.P);
    p.TH1 = b.take<float>(d.P);
    for (int i = 0; i < 7; ++i) p.KT[i] = b.take<float>(d.P);
    p.xh1 = b.take<float>(d.numel);
    p.xh2 = b.take<float>(d.numel);
    p.xh3 = b.take<float>(d.numel);
    p.r1 = b.take<float>((size_t)d.N * d.G);
    p.r2 = b.take<float>((size_t)d.N * d.G);
    p.r3 = b.take<float>((size_t)d.N * d.G);
    p.dz1 = b.take<float>(d.numel + d.C);
    p.dz2 = b.take<float>(d.numel + d.C);
    p.G = b.take<float>(d.numel);
    for (int i = 0; i < 2; ++i) {
      p.wpart[i] = b.take<float>((size_t)d.nsplit * 9 * d.C * d.C);
      p.spart[i] = b.take<float>(prow * 9 * d.C);
    }
    p.sred = b.take<float>((size_t)2 * 9 * d.C + 2 * ((9 * (size_t)d.C + 63) / 64) + 4);   // + vjp_t partials + arrival counter
    for (int i = 0; i < 2; ++i) p.wtime[i] = b.take<float>((size_t)9 * d.C);
    const size_t grows = prow > (size_t)d.mtiles ? prow : (size_t)d.mtiles;
    p.gpart[0] = b.take<float>(grows * 2 * d.C);
    p.gpart[1] = b.take<float>(grows * 2 * d.C);
    p.gpart[2] = b.take<float>(prow * 2 * d.C);
    p.dots = b.take<float>((size_t)(n_t > 0 ? n_t : 1));
  }
  p.bytes = ((b.off + 255) & ~(size_t)255);
  return p;
}

int check_common(const node_shape* shape, const node_params* params, void* ws, size_t ws_bytes, int adjoint, int n_t,
                 Dims* d, Plan* plan) {
  if (!params) return fail(NODE_ERR_NULL, "params is NULL");
  if (!ws) return fail(NODE_ERR_NULL, "workspace is NULL");
  TRY(dims_for(shape, d));
  const float* ptrs[10] = {params->norm1_w, params->norm1_b, params->conv1_w, params->conv1_b, params->norm2_w,
                           params->norm2_b, params->conv2_w, params->conv2_b, params->norm3_w, params->norm3_b};
  for (int i = 0; i < 10; ++i) {
    if (!ptrs[i]) return fail(NODE_ERR_NULL, "parameter pointer %d is NULL", i);
    if (((uintptr_t)ptrs[i]) & 15) return fail(NODE_ERR_ARG, "parameter pointer %d is not 16-byte aligned", i);
  }
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  *plan = make_plan(*d, adjoint, n_t, ws);
  if (ws_bytes < plan->bytes) return fail(NODE_ERR_WORKSPACE, "workspace too small: %zu < %zu", ws_bytes, plan->bytes);
  return NODE_OK;
}

int check_method(int method) {
  if (method != NODE_METHOD_DOPRI5 && method != NODE_METHOD_RK4) return fail(NODE_ERR_ARG, "unknown method %d", method);
  return NODE_OK;
}

int check_times(const float* t_pts, int n_t) {
  if (!t_pts) return fail(NODE_ERR_NULL, "t_pts is NULL");
  if (n_t < 2) return fail(NODE_ERR_ARG, "need at least two time points (got %d)", n_t);
  bool inc = true, dec = true;
  for (int i = 1; i < n_t; ++i) {
    if (!(t_pts[i] > t_pts[i - 1])) inc = false;
    if (!(t_pts[i] < t_pts[i - 1])) dec = false;
  }
  if (!inc && !dec) return fail(NODE_ERR_ARG, "t must be strictly increasing or strictly decreasing");
  return NODE_OK;
}

int check_solve(const node_shape* shape, const node_params* params, void* ws, size_t ws_bytes, int adjoint, const float* t_pts,
                int n_t, int method, const node_solve_opts* opts, Dims* d, Plan* plan, SolveCtl* ctl) {
  TRY(check_method(method));
  TRY(check_times(t_pts, n_t));
  TRY(check_common(shape, params, ws, ws_bytes, adjoint, n_t, d, plan));
  const bool dopri5 = method == NODE_METHOD_DOPRI5;
  SolveCtl c;
  c.forced = dopri5 && opts && opts->n_forced_dt > 0 && opts->forced_dt;
  if (c.forced && opts->n_forced_dt > STEP_LIST_CAP) return fail(NODE_ERR_ARG, "replay list longer than %d", STEP_LIST_CAP);
  c.n_forced = c.forced ? opts->n_forced_dt : 0;
  c.max_steps = (opts && opts->max_num_steps > 0) ? opts->max_num_steps : 2147483647LL;
  c.log_cap = (opts && opts->record_dt > 0 && opts->dt_log) ? (opts->record_dt < STEP_LIST_CAP ? opts->record_dt : STEP_LIST_CAP) : 0;
  // deferred completion: exactly `blind_steps` steps, no read-back, no host staging (nothing of this call may be
  // touched by the host after it returns); the outcome goes to the caller's device record
  c.blind = (opts && opts->blind_steps > 0 && opts->record && n_t == 2 && !c.forced && c.log_cap == 0 && dopri5)
                ? (opts->blind_steps < c.max_steps ? opts->blind_steps : (int)c.max_steps) : 0;
  *ctl = c;
  return NODE_OK;
}

int solve_rc(int status, double dt) {
  if (status == 0) return NODE_OK;
  if (status == NODE_ERR_MAX_STEPS) return fail(NODE_ERR_MAX_STEPS, "max_num_steps exceeded");
  if (status == NODE_ERR_DT_UNDERFLOW) return fail(NODE_ERR_DT_UNDERFLOW, "underflow in dt %g", dt);
  if (status == NODE_ERR_NONFINITE) return fail(NODE_ERR_NONFINITE, "non-finite error norm / state");
  return fail(status, "solver stopped with status %d", status);
}

}  // namespace node

using namespace node;

extern "C" size_t node_workspace_bytes(const node_shape* shape, int /*method*/, int adjoint, int n_t) {
  Dims d;
  if (dims_for(shape, &d) != NODE_OK) return 0;
  Plan p = make_plan(d, adjoint, n_t, nullptr);
  return p.bytes;
}
