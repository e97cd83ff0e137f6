// C ABI of the fused solver: one evaluation of the dynamics and its VJP, the forward solve, the continuous adjoint.
// What is checked and reported lives here; what a step enqueues lives in solver.hip.
#include "solver.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace node;

extern "C" {

int node_odefunc_fwd(const node_shape* shape, const node_params* params, float t, const float* y, float* f,
                     void* ws, size_t ws_bytes, void* stream) {
  w4_refresh_tuning();     // (the NODE_TUNE_W4_* switches: once per call, not per launch)
  if (!y || !f) return fail(NODE_ERR_NULL, "y / f is NULL");
  Solver S;
  TRY(check_common(shape, params, ws, ws_bytes, 0, 2, &S.d, &S.p));
  S.prm = *params; S.st = (hipStream_t)stream; S.aug = false; S.tsign = 1.f;
  S.choose_w4(false);
  TRY(S.prepare());
  launch_set_ctrl(S.p.ctrl, (double)t, 0.0, 1, S.st);
  S.to_state(y, S.p.Y);
  TRY(S.eval_sys(0, nullptr, 0, SC_ABS, S.et_stage(0.0), false));
  S.from_state(S.p.KY[0], f);
  return S.check_launch("node_odefunc_fwd");
}

int node_odefunc_vjp(const node_shape* shape, const node_params* params, float t, const float* y, const float* cot,
                     float* f, float* vjp_y, float* vjp_t, float* vjp_params, void* ws, size_t ws_bytes, void* stream) {
  w4_refresh_tuning();     // (the NODE_TUNE_W4_* switches: once per call, not per launch)
  if (!y || !cot || !f || !vjp_y || !vjp_t || !vjp_params) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  Solver S;
  TRY(check_common(shape, params, ws, ws_bytes, 1, 2, &S.d, &S.p));
  S.prm = *params; S.st = (hipStream_t)stream; S.aug = true; S.tsign = 1.f;
  S.choose_w4(false);
  TRY(S.prepare());
  launch_set_ctrl(S.p.ctrl, (double)t, 0.0, 1, S.st);
  S.to_state(y, S.p.Y);
  S.to_state(cot, S.p.A);
  Comb cy = make_comb(S.p.Y, S.p.KY, nullptr, 0, SC_ABS);
  Comb ca = make_comb(S.p.A, S.p.KA, nullptr, 0, SC_ABS);
  TRY(S.eval_aug(cy, ca, nullptr, nullptr, S.et_stage(0.0), S.p.KY[0], S.p.KA[0], S.p.KT[0], -1, +1.f, vjp_t));
  S.from_state(S.p.KY[0], f);
  S.from_state(S.p.KA[0], vjp_y);
  launch_theta_to_torch(S.d, S.p.KT[0], vjp_params, S.st);
  return S.check_launch("node_odefunc_vjp");
}

int node_solve_fwd(const node_shape* shape, const node_params* params, const float* y0, const float* t_pts, int n_t,
                   float rtol, float atol, int method, const node_solve_opts* opts, float* y_out, node_stats* stats,
                   void* ws, size_t ws_bytes, void* stream) {
  w4_refresh_tuning();
  if (!y0 || !y_out) return fail(NODE_ERR_NULL, "y0 / y_out is NULL");
  Solver S;
  SolveCtl ctl;
  TRY(check_solve(shape, params, ws, ws_bytes, 0, t_pts, n_t, method, opts, &S.d, &S.p, &ctl));
  S.prm = *params; S.st = (hipStream_t)stream; S.aug = false; S.rtol = rtol; S.atol = atol;
  const bool forced = ctl.forced;
  HostStage* hs = nullptr;
  TRY(get_stage((size_t)n_t + 2 * STEP_LIST_CAP, &hs));
  S.hctrl = hs->ctrl;
  const bool decreasing = t_pts[1] < t_pts[0];
  S.tsign = decreasing ? -1.f : 1.f;
  std::vector<double> ts(n_t);
  for (int i = 0; i < n_t; ++i) ts[i] = (double)(decreasing ? -t_pts[i] : t_pts[i]);
  node_stats stt;
  memset(&stt, 0, sizeof(stt));
  DtLog dlog(opts);
  const size_t numel = S.d.numel;

  S.choose_w4(method == NODE_METHOD_DOPRI5);   // (a replay of recorded steps runs the numerics of the solve it replays)
  S.choose_resident(method == NODE_METHOD_DOPRI5);
  if (method == NODE_METHOD_DOPRI5) S.take_norm_hook(opts);
  if (S.nr_fn != nullptr) S.resident = false;      // (global-norm mode: the host's hook sits between the launches of a step)
  // dopri5: the record's reset and, for a deferred solve, its one target time ride in the preparation launch (SolveSetup) -- nothing
  // between here and f0 reads either
  const bool setup_rides = !S.resident && method == NODE_METHOD_DOPRI5;
  bool y0_in_slot1 = false;      // a deferred solve's y_out[1] <- y0 was done by the state's layout launch
  if (!S.resident) {      // (the resident solve packs its filters, forms its border maps and copies y0 inside its one launch)
    SolveSetup su;
    memset(&su, 0, sizeof(su));
    su.ctrl = S.p.ctrl; su.set_ctrl = 1; su.t = ts[0]; su.dt = forced ? opts->forced_dt[0] : 0.0;
    if (ctl.blind) { su.targets = S.p.targets; su.target = ts[1]; }
    TRY(S.prepare(setup_rides ? &su : nullptr));
    if (S.w4) {     // y0 -> the state, the trajectory's first slot and (deferred) the output slot a missed solve leaves alone: one launch
      W4sLayoutJobs lj;
      memset(&lj, 0, sizeof(lj));
      lj.src[0] = y0; lj.dst[0] = S.p.Y; lj.copy[0][0] = y_out; lj.njobs = 1;
      if (method == NODE_METHOD_DOPRI5 && ctl.blind) { lj.copy[0][1] = y_out + numel; y0_in_slot1 = true; }
      launch_w4s_from_nchw_jobs(lj, S.d.N, S.d.C, S.d.w4q, S.st);
    } else {
      S.to_state(y0, S.p.Y);
      HIP_TRY(hipMemcpyAsync(y_out, y0, numel * sizeof(float), hipMemcpyDeviceToDevice, S.st));
    }
  }

  if (method == NODE_METHOD_RK4) {
    launch_set_ctrl(S.p.ctrl, ts[0], 0.0, 1, S.st);
    for (int j = 1; j < n_t; ++j) {
      TRY(S.rk4_interval(ts[j - 1], ts[j]));
      S.from_state(S.p.Y, y_out + (size_t)j * numel);
      stt.accepted += 1;
      dlog.add(ts[j] - ts[j - 1], true);
    }
    HIP_TRY(hipStreamSynchronize(S.st));
    stt.nfe = S.nfe; stt.t_final = ts[n_t - 1]; stt.last_dt = ts[n_t - 1] - ts[n_t - 2];
    if (stats) *stats = stt;
    return S.check_launch("node_solve_fwd(rk4)");
  }

  // ---- dopri5: every decision of the step loop is taken on the device ----
  const long long max_steps = ctl.max_steps;
  StepIO io;
  io.n_targets = n_t - 1;
  io.n_forced = ctl.n_forced;
  io.log_cap = ctl.log_cap;
  io.y_out = y_out + numel;
  const int blind = ctl.blind;     // deferred completion (SolveCtl): the outcome goes to the caller's device record
  const bool inline_targets = S.resident && io.n_targets <= 8;      // (the target times ride in the kernel arguments)
  if (inline_targets) {
    if (blind) HIP_TRY(hipMemcpyAsync(y_out + numel, y0, numel * sizeof(float), hipMemcpyDeviceToDevice, S.st));
  } else if (blind) {
    if (!setup_rides) launch_set_target(S.p.targets, ts[1], S.st);
    // a MISSED blind solve never emits its output: leave y0 there, not uninitialised memory (the caller's loss of
    // such a step is then a finite number of a step whose update is skipped anyway)
    if (!y0_in_slot1) HIP_TRY(hipMemcpyAsync(y_out + numel, y0, numel * sizeof(float), hipMemcpyDeviceToDevice, S.st));
  } else {
    TRY(S.upload(S.p.targets, ts.data() + 1, n_t - 1, hs->lists));
  }
  if (forced) TRY(S.upload(S.p.forced, opts->forced_dt, opts->n_forced_dt, hs->lists + n_t));
  if (S.resident) {
    // the whole solve -- f0, the initial step, every step with its decision, dense output -- is one launch; it needs as many steps
    // as it needs (a deferred solve of this kind cannot miss), and the host reads the same record back
    TRY(S.launch_resident(y0, y_out, io, ts.data(), inline_targets, forced, max_steps, blind));
    if (blind) {
      launch_export_record(S.p.ctrl, opts->record, opts->miss_flag, 2147483647, S.st);
      stt.status = NODE_PENDING;
      stt.accepted = blind; stt.rejected = 0;
      stt.nfe = S.nfe + 6 * blind;
      stt.t_final = ts[1];
      if (stats) *stats = stt;
      return S.check_launch("node_solve_fwd(dopri5, resident, deferred)");
    }
    // the launch wrote the record into the pinned host copy itself: completion of the stream is all the host waits for
    HIP_TRY(hipStreamSynchronize(S.st));
    if (S.hctrl->status == NODE_ERR_HIP) {
      // a wait inside the launch ran into its deadline: the grid was not co-resident (other processes' resident grids on this
      // GPU can leave two launches each waiting for compute units the other holds).  Every workgroup has left; the solve runs
      // again on the launch-per-convolution path, which needs no co-residency.
      S.resident = false;
      g_resident_cooldown.store(64, std::memory_order_relaxed);
      S.nfe = 0;
      TRY(S.prepare());
      S.to_state(y0, S.p.Y);
      HIP_TRY(hipMemcpyAsync(y_out, y0, numel * sizeof(float), hipMemcpyDeviceToDevice, S.st));
      if (inline_targets) TRY(S.upload(S.p.targets, ts.data() + 1, n_t - 1, hs->lists));
    }
  }
  if (!S.resident) {
    if (!setup_rides) launch_set_ctrl(S.p.ctrl, ts[0], forced ? opts->forced_dt[0] : 0.0, 1, S.st);   // (a resident solve that fell back)
    TRY(S.eval_sys(0, nullptr, 0, SC_ABS, S.et_stage(0.0), false));  // f0 (FSAL seed)
    if (!forced) TRY(S.initial_step());
  }
  if (blind) {
    for (int i = 0; i < blind; ++i) {
      if (i == blind - 1) { io.rec = opts->record; io.miss_flag = opts->miss_flag; io.expect_steps = blind; }   // (the record rides in the last commit)
      TRY(S.enqueue_step(io));
    }
    stt.status = NODE_PENDING;
    stt.accepted = blind; stt.rejected = 0;            // predicted: true iff the record says no miss
    stt.nfe = S.nfe + 6 * blind;
    stt.t_final = ts[1];
    if (stats) *stats = stt;
    return S.check_launch("node_solve_fwd(dopri5, deferred)");
  }
  StepGuess key = {S.d.N, S.d.C, S.d.H, S.d.W, 0, forced ? 1 : 0, rtol, atol, ts[0], ts[n_t - 1], 0};
  int status = 0;
  if (S.resident) status = S.hctrl->status;
  else TRY(S.run_steps(io, max_steps, guess_steps(key), &status));
  const Ctrl& h = *S.hctrl;
  key.steps = h.step_idx;
  if (status == 0 && !S.resident) remember_steps(key);
  stt.status = status;
  stt.accepted = h.n_acc; stt.rejected = h.n_rej;
  stt.nfe = S.nfe + 6 * h.step_idx;     // f0 (+ the initial-step probe) + six stages per step tried (show.py:199)
  stt.first_dt = h.first_dt; stt.t_final = h.t; stt.last_dt = h.dt;
  if (io.log_cap > 0) {
    const int n = h.step_idx < io.log_cap ? h.step_idx : io.log_cap;
    double* stage = hs->lists;
    HIP_TRY(hipMemcpyAsync(stage, S.p.dtlog, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, S.st));
    HIP_TRY(hipStreamSynchronize(S.st));
    for (int i = 0; i < n; ++i) dlog.add(fabs(stage[i]), stage[i] > 0.0);
  }
  if (stats) *stats = stt;
  TRY(S.check_launch("node_solve_fwd(dopri5)"));
  return solve_rc(stt.status, h.dt);
}

int node_solve_adjoint(const node_shape* shape, const node_params* params, const float* y_traj, const float* grad_out,
                       const float* t_pts, int n_t, float rtol, float atol, int method, const node_solve_opts* opts,
                       float* grad_y0, float* grad_params, float* grad_t, node_stats* stats, void* ws, size_t ws_bytes,
                       void* stream) {
  w4_refresh_tuning();
  if (!y_traj || !grad_out || !grad_y0 || !grad_params) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  Solver S;
  SolveCtl ctl;
  TRY(check_solve(shape, params, ws, ws_bytes, 1, t_pts, n_t, method, opts, &S.d, &S.p, &ctl));
  S.prm = *params; S.st = (hipStream_t)stream; S.aug = true; S.rtol = rtol; S.atol = atol;
  const bool forced = ctl.forced;
  HostStage* hs = nullptr;
  TRY(get_stage((size_t)n_t + 2 * STEP_LIST_CAP, &hs));
  S.hctrl = hs->ctrl;
  node_stats stt;
  memset(&stt, 0, sizeof(stt));
  DtLog dlog(opts);
  const size_t numel = S.d.numel;
  const long long max_steps = ctl.max_steps;
  StepIO io;
  io.n_targets = 1;
  io.n_forced = ctl.n_forced;
  io.log_cap = ctl.log_cap;
  const int blind = ctl.blind;     // deferred completion (SolveCtl)
  S.choose_w4(method == NODE_METHOD_DOPRI5);   // (a replay of recorded steps runs the numerics of the solve it replays)
  S.w4_f16_aug = method == NODE_METHOD_DOPRI5;
  if (method == NODE_METHOD_DOPRI5) S.take_norm_hook(opts);
  {
    // carried by the preparation launch (SolveSetup): the record's reset -- which also zeroes the scalar segment (adj_time = 0) --,
    // adj_params = 0, and for dopri5 the FIRST interval's start and (deferred) target: nothing in front of that interval's first
    // evaluation reads any of them.  Later intervals of a time grid keep their setters.
    SolveSetup su;
    memset(&su, 0, sizeof(su));
    su.ctrl = S.p.ctrl; su.set_ctrl = 1; su.t = 0.0; su.dt = 0.0;
    su.zero = S.p.TH; su.zero_n = S.d.P;
    if (method != NODE_METHOD_RK4) {
      const bool dec = t_pts[n_t - 2] < t_pts[n_t - 1];
      su.set_interval = 1; su.iv_t = (double)(dec ? -t_pts[n_t - 1] : t_pts[n_t - 1]); su.iv_dt = forced ? opts->forced_dt[0] : 0.0;
      if (blind) { su.targets = S.p.targets; su.target = (double)(dec ? -t_pts[n_t - 2] : t_pts[n_t - 2]); }
    }
    TRY(S.prepare(&su));
  }
  const int w4_gskew = env_int("NODE_TUNE_W4_GSKEW", 0);           // diagnostics (include/node_hip.h, node_w4_pair_stats)
  const bool w4_stats = env_int("NODE_TUNE_W4_STATS", 0) != 0;
  g_w4_pair_stats[0] = S.w4_f16 ? 1 : 0; g_w4_pair_stats[1] = -1; g_w4_pair_stats[2] = 0; g_w4_pair_stats[3] = 0;
  // grad_last_only: `grad_out` is the last slice alone, every other slice of dL/dy_out is zero (node_solve_opts)
  const bool last_only = opts && opts->grad_last_only;
  const float* g_last = last_only ? grad_out : grad_out + (size_t)(n_t - 1) * numel;
  if (S.w4) {     // adj_y = grad_output[-1] and the first interval's y = y_traj[-1]: one launch, two jobs
    W4sLayoutJobs lj;
    memset(&lj, 0, sizeof(lj));
    lj.src[0] = g_last; lj.dst[0] = S.p.A; lj.src[1] = y_traj + (size_t)(n_t - 1) * numel; lj.dst[1] = S.p.Y; lj.njobs = 2;
    launch_w4s_from_nchw_jobs(lj, S.d.N, S.d.C, S.d.w4q, S.st);
  } else {
    S.to_state(g_last, S.p.A);  // adj_y = grad_output[-1]
  }
  if (forced) TRY(S.upload(S.p.forced, opts->forced_dt, opts->n_forced_dt, hs->lists + n_t));
  double cur_t = 0.0, cur_dt = 0.0;
  bool first = true;
  int steps_total = 0;

  for (int i = n_t - 1; i >= 1 && stt.status == 0; --i) {
    // the interval is integrated from t_i to t_{i-1}; upstream negates time when that is decreasing
    const bool decreasing = t_pts[i - 1] < t_pts[i];
    S.tsign = decreasing ? -1.f : 1.f;
    const double s0 = (double)(decreasing ? -t_pts[i] : t_pts[i]);
    const double s1 = (double)(decreasing ? -t_pts[i - 1] : t_pts[i - 1]);

    if (!(S.w4 && i == n_t - 1)) S.to_state(y_traj + (size_t)i * numel, S.p.Y);
    // grad_output_i in NHWC for the dot product below: in the first interval the adjoint state still IS it; a zero
    // slice (grad_last_only) contributes nothing
    const float* gdot = i == n_t - 1 ? S.p.A : (last_only ? nullptr : S.p.G);
    if (i != n_t - 1 && !last_only) S.to_state(grad_out + (size_t)i * numel, S.p.G);
    // func_i = f(t_i, y_i); adj_time -= <func_i, grad_output_i>.  Upstream evaluates f here and again as
    // the first stage of the augmented solve at the same (t_i, y_i); the stage-0 evaluation below
    // produces tsign * f bit-identically, so the dot product is taken from it (times tsign) and the
    // separate evaluation is only COUNTED (the reference's nfe counter, model.py:340, would have seen it).
    S.nfe += 1;
    float* dots_i = grad_t ? S.p.dots + i : nullptr;
    if (gdot == nullptr && dots_i) launch_fill(dots_i, 0.f, 1, S.st);

    if (method == NODE_METHOD_RK4) {
      TRY(S.rk4_interval(s0, s1, gdot, gdot ? dots_i : nullptr));
      stt.accepted += 1;
      dlog.add(s1 - s0, true);
      cur_t = s1; cur_dt = s1 - s0;
    } else {
      // replay list restarts per interval (one odeint call each upstream)
      const bool rode = i == n_t - 1;     // (the first interval's setters rode in the preparation launch)
      if (!rode) launch_set_interval(S.p.ctrl, s0, forced ? opts->forced_dt[0] : 0.0, S.st);
      if (blind) { if (!rode) launch_set_target(S.p.targets, s1, S.st); }
      else TRY(S.upload(S.p.targets, &s1, 1, hs->lists + (n_t - 1 - i) % n_t));
      S.g_ready = false;      // (fp16-pair operands: the interval's first evaluation runs the triples and records max|dz|, wino4.h)
      TRY(S.eval_sys(0, nullptr, 0, SC_ABS, S.et_stage(0.0), false));
      if (S.w4_f16) { launch_w4_gscale(S.p.w4sc, S.st, w4_gskew); S.g_ready = true; }
      if (gdot) launch_dot_sub_scalar(S.p.ctrl, S.p.KY[0], gdot, numel, S.tsign, S.p.partial[0], dots_i, S.st);
      if (!forced) TRY(S.initial_step());
      if (blind) {   // deferred completion (one interval): the record says later whether these were the steps needed
        for (int q = 0; q < blind; ++q) {
          if (q == blind - 1) { io.rec = opts->record; io.miss_flag = opts->miss_flag; io.expect_steps = blind; }   // (the record rides in the last commit)
          TRY(S.enqueue_step(io));
        }
        io.rec = nullptr; io.miss_flag = nullptr;
        steps_total += blind;
        stt.accepted = blind; stt.rejected = 0; stt.status = 0;
        cur_t = s1; cur_dt = 0.0;
        if (!last_only) {
          S.to_state(grad_out + (size_t)(i - 1) * numel, S.p.G);
          launch_axpy(S.p.A, S.p.G, 1.f, numel, S.st);
        }
        continue;
      }
      StepGuess key = {S.d.N, S.d.C, S.d.H, S.d.W, 1, forced ? 1 : 0, rtol, atol, s0, s1, 0};
      int status = 0;
      // the dense output of the adjoint, parameter and time segments at s1 happens on the device with the last step
      TRY(S.run_steps(io, max_steps, guess_steps(key), &status));
      const Ctrl& h = *S.hctrl;
      key.steps = h.step_idx;
      if (status == 0) remember_steps(key);
      stt.status = status;
      if (first) { stt.first_dt = h.first_dt; first = false; }
      steps_total += h.step_idx;
      stt.accepted = h.n_acc; stt.rejected = h.n_rej;     // cumulative over the intervals
      cur_t = h.t; cur_dt = h.dt;
      if (io.log_cap > 0) {
        const int n = h.step_idx < io.log_cap ? h.step_idx : io.log_cap;
        double* stage = hs->lists + n_t + STEP_LIST_CAP;
        HIP_TRY(hipMemcpyAsync(stage, S.p.dtlog, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, S.st));
        HIP_TRY(hipStreamSynchronize(S.st));
        for (int q = 0; q < n; ++q) dlog.add(fabs(stage[q]), stage[q] > 0.0);
      }
      if (stt.status != 0) break;
    }
    // adj_y += grad_output[i-1]
    if (!last_only) {
      S.to_state(grad_out + (size_t)(i - 1) * numel, S.p.G);
      launch_axpy(S.p.A, S.p.G, 1.f, numel, S.st);
    }
  }

  S.from_state(S.p.A, grad_y0);
  launch_theta_to_torch(S.d, S.p.TH, grad_params, S.st);
  if (grad_t) {
    // time_vjps = [adj_time, dLd_t1, ..., dLd_t_{T-1}]
    launch_copy_scalar_out(S.p.ctrl, S.p.dots, S.st);
    HIP_TRY(hipMemcpyAsync(grad_t, S.p.dots, (size_t)n_t * sizeof(float), hipMemcpyDeviceToDevice, S.st));
  }
  if (blind) {
    stt.status = NODE_PENDING;
    stt.nfe = S.nfe + 6 * steps_total;
    stt.t_final = cur_t;
    if (stats) *stats = stt;
    return S.check_launch("node_solve_adjoint(deferred)");
  }
  // (dopri5: every interval ended with a read-back, behind which nothing of this call is staged on the host -- the launches above are
  //  ordinary stream work the caller's next launches queue behind, and the host does not wait for them; rk4 has no read-back)
  if (method == NODE_METHOD_RK4) HIP_TRY(hipStreamSynchronize(S.st));
  if (w4_stats && S.w4_f16) {   // (diagnostics: two words of the scale block; the read-back above left the stream idle)
    W4Scales hsc;
    HIP_TRY(hipMemcpyAsync(&hsc, S.p.w4sc, offsetof(W4Scales, pad), hipMemcpyDeviceToHost, S.st));
    HIP_TRY(hipStreamSynchronize(S.st));
    g_w4_pair_stats[1] = hsc.n_retry;
    g_w4_pair_stats[2] = hsc.e[W4_E_G];
  }
  stt.nfe = S.nfe + 6 * steps_total;
  stt.t_final = cur_t; stt.last_dt = cur_dt;
  if (stats) *stats = stt;
  TRY(S.check_launch("node_solve_adjoint"));
  return solve_rc(stt.status, cur_dt);
}

}  // extern "C"
