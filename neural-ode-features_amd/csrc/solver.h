// The solver context: one fused solve (forward or augmented / adjoint) on one stream.
//
// The host code is the *driver* of the integrator: it owns no numerics.  Every number (stage values, error norms,
// accept decisions, step sizes) is produced by device kernels and stays in device memory -- including the decisions of
// the adaptive step loop (accept / reject, which output times a step passed, dense output, FSAL commit, end of the
// interval).  The host
//   * enqueues whole steps on the caller's stream, as many as the previous solve of the same problem needed,
//   * reads one small `Ctrl` record back per solve to learn whether that was enough (and tops up if not), or --
//     deferred completion, node_solve_opts.blind_steps -- reads nothing back at all and leaves the verdict in a
//     device record on which the caller predicates whatever commits results.
//
// Algorithm: restated torchdiffeq dopri5 / rk4(3/8) / continuous adjoint, see SURVEY.md 8c and
// oracle/torchdiffeq_restated.py (the CPU checker).  Member bodies: solver.hip.
#pragma once
#include "butcher.h"
#include "plan.h"

#include <atomic>

namespace node {

// How many steps the last solve of the same problem took: the number enqueued blind before the first read-back.
// (One cache per host thread, solver.hip.)
struct StepGuess { int N, C, H, W, aug, forced; float rtol, atol; double t0, t1; int steps; };
int guess_steps(const StepGuess& k);
void remember_steps(const StepGuess& k);

extern int g_w4_pair_stats[4];                 // node_w4_pair_stats (diagnostics; process-wide: a backward pass runs on autograd's thread)
extern std::atomic<int> g_resident_cooldown;   // solves left before the resident latency path is tried again (Solver::choose_resident)

// Where a run of dopri5 steps writes: the interval's target times, the replay list, the dt log (device arrays),
// and -- forward solve -- the caller's trajectory.
struct StepIO {
  int n_targets = 0;
  int n_forced = 0;        // > 0: replay mode
  int log_cap = 0;         // > 0: dt log wanted
  float* y_out = nullptr;  // forward: [n_targets][N][C][H][W], slot j <-> target j
  // deferred completion, set for the LAST step enqueued only: its commit launch leaves the caller's record (CommitArgs::rec)
  node_step_record* rec = nullptr;
  float* miss_flag = nullptr;
  int expect_steps = 0;
};

// the evaluation that follows the one being enqueued: its combine may ride in this one's last pass
struct NextComb { Comb cy; float* y_out; };

struct Solver {
  Dims d;
  Plan p;
  node_params prm;
  hipStream_t st;
  bool aug = false;
  float tsign = 1.f;
  float rtol = 0.f, atol = 0.f;
  int nfe = 0;
  bool count_nfe = true;   // off while steps are enqueued blind: those evaluations are counted from the device's step counter
  Ctrl* hctrl = nullptr;   // pinned host mirror of p.ctrl (HostStage::ctrl)

  // ---- which kernels serve this solve ----
  // F(4x4,3x3) pipeline for the convs of this solve (wino4.h).  Its rounding error (3.2e-6 of max|y| per conv, against
  // 4.9e-7 for F(2x2,3x3)) must stay far below what the step controller resolves.  dopri5's embedded estimate is
  // h * sum_i e_i k_i with sum_i |e_i| = 0.16, so conv noise moves it by <= 0.16 * 3.2e-6 * h |f| ~ 5e-7 |y| -- 5 % of
  // the tolerance at 1e-5, 50 % at 1e-6.  Adaptive solves with rtol, atol >= 1e-5 take the pipeline (measured at tol
  // 1e-5: same step sequences, gradients as close to fp64 as the fp32 oracle's -- tests/test_gpu_w4.py).
  bool w4 = false;
  void choose_w4(bool adaptive) {
    w4 = d.wino4 == 2 || (d.wino4 == 1 && adaptive && rtol >= W4_MIN_TOL && atol >= W4_MIN_TOL && !tiny_mode());
  }
  // latency path: forward solves of tiny batches run two fused direct-convolution launches per evaluation (kernels_tiny.hip)
  bool tiny_mode() const { return d.tiny != 0 && !aug && p.wtiny[0] != nullptr; }
  // inference solves on grids the throughput tiles cannot spread over the chip (Dims::small)
  bool small_mode() const { return d.small && !aug && !w4 && p.wsmall[0] != nullptr && !tiny_mode(); }
  // ... and a free-running or replayed dopri5 forward solve of a state the chip can hold resident is ONE launch
  // (kernels_tiny_solve.hip).  Not under stream capture (a captured launch would replay its nonce), and not for 64
  // solves after a launch that ran into its deadline: a grid that did not get the whole chip costs 2 s.
  bool resident = false;
  void choose_resident(bool dopri5);
  // The whole resident solve -- f0, the initial step, every step with its decision, dense output -- as one launch:
  // fills its arguments, keeps the {nonce, generation} book of the hand-off buffers and sets nfe.  `ts`: the time
  // points in solver orientation.  The launch writes the record to the pinned host copy itself (deferred: to a copy
  // that only this library reads, for the cooldown).
  int launch_resident(const float* y0, float* y_out, const StepIO& io, const double* ts, bool inline_targets, bool forced,
                      long long max_steps, int blind);

  // ---- state of the F(4x4,3x3) passes, merged across evaluations (kernels_w4s.hip): the pass that ends evaluation s
  // may already have formed evaluation s + 1's conv input (Butcher combine -> GroupNorm-1 -> ReLU -> V) ----
  bool w4_b16 = false;     // the component GEMMs read the filters as exact bf16 triples (k_w4_gemm64b), decided in prepare()
  bool w4_f16 = false;     // ... both operands as fp16 pairs (k_w4_gemm64h; wino4.h), decided in prepare()
  bool w4_f16_aug = false; // set by the caller before prepare(): an augmented solve may use them (adaptive dopri5 solves: the cotangent-side
                           // scale follows the data through the step controller)
  float* va0_of(int set) const { return (set && p.W4Va0b != nullptr) ? p.W4Va0b : p.W4Va[0]; }
  bool g_ready = false;    // the cotangent-side scale is known (behind an interval's first evaluation, launch_w4_gscale)
  // the format of the evaluation being enqueued: forward solves always pairs; augmented ones once the cotangent scale is known
  bool f16_now() const { return w4_f16 && (!aug || g_ready); }
  bool v_ready = false;    // the next evaluation's first pass has run
  int cur = 0;             // which set of GroupNorm-1's saved tensors (act1, xhat-1, 1/sigma-1) the current evaluation owns
  float* act1_of(int i) const { return i ? p.act1b : p.act1; }
  float* xh1_of(int i) const { return i ? p.xh1b : p.xh1; }
  float* r1_of(int i) const { return i ? p.r1b : p.r1; }
  // the weight gradients of an augmented evaluation in the F(4x4,3x3) domain (k_w4_wgrad): needs the forward convs'
  // row operands alive behind the data-gradient convs, so they get buffers of their own
  bool w4_wgrad_on() const { return w4 && aug && p.W4dU != nullptr; }
  // ---- the theta finalize of an augmented evaluation that is followed by another of the same step (s = 1..4 of enqueue_step's
  // loop, the stage derivatives k3..k6: s = 0 has no finalize -- NODE_TUNE_SKIP_K2_THETA -- and s = 5 has no `next`, four per step)
  // is not launched: it waits here and rides in the next evaluation's P2 launch (k_w4s_pass_rider).
  // No hazard, checked against eval_w4: the finalize of evaluation i reads W4dU (or wpart), gpart[0..2], spart[0..1], wtime and
  // sred.  Between PB1C(i) and P2(i+1) only gemm0(i+1) runs, which reads V / U and writes M.  P2(i+1) writes W4Va[1] (or W4V),
  // xh2, r2 (and act2 without the F(4x4,3x3) weight gradient).  The first launches that write what the finalize reads are
  // P3B3(i+1) (gpart[2], spart[1]), PB2(i+1) (gpart[1], spart[0]), the weight gradient (W4dU / wpart) and PB1(i+1) (gpart[0]):
  // all of them behind the kernel boundary after P2(i+1).  What it writes -- KT[k], and ctrl->ts_k[k] from its last workgroup --
  // nothing reads before the step's k_error_norm / k_step_controller; P2 reads ctrl->done, t, dt (h0), other words of the record.
  // A waiting finalize never survives the end of enqueue_step.
  // Re-checked with the paired launch (NODE_TUNE_WGRAD_PAIRED, k_w4_gemm64h_wgrad64h: the weight gradient and the conv-1 data
  // gradient's GEMM of evaluation i + 1 in one launch, W4dU written concurrently with W4M): the launch sits where the two sat, behind
  // PB2(i+1) and so behind P2(i+1), which carried the finalize.  Inside it the GEMM half reads W4V (PB2's) and the packed filters,
  // the weight-gradient half va0, W4Va[1], W4Z[0..1]: neither reads W4M or W4dU.  The first readers are PB1(i+1) (W4M) and the
  // finalize of evaluation i + 1 (W4dU: its own launch behind PB1, or the rider of P2(i+2)) -- both behind the launch's end. ----
  bool theta_rider = true;          // NODE_TUNE_THETA_RIDER (default 1; 0: every finalize is its own launch), read in prepare()
  bool tf_waiting = false;
  ThetaFinalizeArgs tf_wait;

  void to_state(const float* nchw, float* dst) {    // NCHW -> the solve's internal state layout
    if (w4) launch_w4s_from_nchw(nchw, dst, d.N, d.C, d.w4q, st);
    else launch_nchw_to_nhwc(d, nchw, dst, st);
  }
  void from_state(const float* src, float* nchw) {
    if (w4) launch_w4s_to_nchw(src, nchw, d.N, d.C, d.w4q, st);
    else launch_nhwc_to_nchw(d, src, nchw, st);
  }

  // ---- global-norm mode of a data-parallel solve (node_solve_opts::norm_reduce): the caller's hook adds the ranks'
  // sums before each decision ----
  void (*nr_fn)(void*, float*, int32_t, void*) = nullptr;
  void* nr_ctx = nullptr;
  float* nr_buf = nullptr;
  float nr_world = 1.f;
  void take_norm_hook(const node_solve_opts* o);
  // this rank's sums of the coming decision -> nr_buf, summed over the ranks by the hook (both enqueued on the solve's stream)
  void norm_exchange(int mode, int nseg);

  double conv_flops() const { return 2.0 * 9.0 * d.C * d.C * (double)d.N * d.HW; }
  int check_launch(const char* what);

  // ---- set-up launches of a solve: filter packing, border maps, the solve's zero fills ----
  // `setup`: the caller's scalar set-up of the solve and one more zero fill, carried by the preparation launch (SolveSetup)
  int prepare(const SolveSetup* setup = nullptr);

  // ---- one evaluation of the dynamics ----
  // f(t, y_i) with y_i = cy; writes k_out = tsign * f  (and y_i to y_out if asked)
  int eval_fwd(const Comb& cy, float* y_out, const EvalTime& et, float* k_out, bool train, const NextComb* next = nullptr);
  // augmented dynamics: (f, csign*a^T df/dy, csign*a^T df/dt, csign*a^T df/dtheta) * tsign
  //   upstream adjoint: csign = -1.   kT_out / scalar ts_k[kidx] optional.
  // need_theta = false: the parameter / time components of this stage derivative are never consumed (dopri5
  // stage 2: b_2 = b^_2 = c_mid,2 = 0 and no stage STATE of those segments is ever formed, since f does not depend
  // on them), so the two weight-gradient GEMMs and the finalize are skipped; kT_out / ts_k[kidx] keep their
  // (finite, zero-weighted) contents.
  int eval_aug(const Comb& cy, const Comb& ca, float* y_out, float* a_out, const EvalTime& et, float* kY_out, float* kA_out,
               float* kT_out, int kidx, float csign, float* vjp_t_out, bool need_theta = true, const NextComb* next = nullptr);
  // evaluate the system at (state + scale * sum coef_j k_j) into k[kout]
  // next_coef (F(4x4,3x3) solves): the Butcher row of the evaluation that follows -- its combine rides in this one's last pass
  int eval_sys(int kout, const double* coef, int ncoef, int scale_mode, const EvalTime& et, bool write_new, bool need_theta = true,
               const double* next_coef = nullptr, int next_ncoef = 0, bool next_write_new = false);
  EvalTime et_stage(double alpha) const { EvalTime e; e.ctrl = p.ctrl; e.alpha = (float)alpha; e.tsign = tsign; e.mode = TM_STAGE; return e; }
  EvalTime et_probe() const { EvalTime e; e.ctrl = p.ctrl; e.alpha = 0.f; e.tsign = tsign; e.mode = TM_PROBE; return e; }

  // split-conv mode: GroupNorm (+ReLU) of the conv's raw output as a pointwise pass (k_combine_gn with an empty
  // Butcher row), and the ReLU-mask + GroupNorm backward of a raw data gradient (k_gn_bwd)
  void gn_pass_fwd(const float* gamma, const float* beta, int relu, float osign, float* out, float* xhat_out, float* rstd_out);
  void gn_pass_bwd(const float* act, const float* xhat, const float* rstd, const float* gamma, float osign, float* out, float* gpart,
                   float* spart);
  // F(4x4,3x3) pipeline: one conv = component GEMMs on the row operand its producer left in W4V; the GroupNorm pass
  // behind it reads the products (output transform, + bias + t * tmap for a forward conv) and, when another conv
  // follows, leaves that conv's row operand in W4V again
  void w4_gemm(int which, const float* V = nullptr);
  W4sArgs w4_args() const;
  // tail 1 of a pass: stage combine -> GroupNorm-1 -> ReLU -> V (+ act1, xhat-1, 1/sigma-1 of set `set` when training)
  void w4_tail_combine(W4sArgs& a, const Comb& cy, float* y_out, bool train, int set, int self);
  // launch one pass; under node_profile_begin() with HIP events around it and its algorithmic bytes (every tensor it
  // must read or write, once) in the record
  // `rider` (P2 only): the waiting theta finalize that this launch carries
  void w4_pass(int head, int tail, const W4sArgs& a, const ThetaFinalizeArgs* rider = nullptr);
  // One dynamics evaluation (ca == nullptr) or one augmented evaluation on the F(4x4,3x3) pipeline.  `next`: the
  // evaluation that follows takes its conv input from this one's last pass (v_ready).
  int eval_w4(const Comb& cy, float* y_out, const EvalTime& et, float* kY_out, bool train, const Comb* ca, float* a_out, float* kA_out,
              float* kT_out, int kidx, float csign, float* vjp_t_out, bool need_theta, const NextComb* next);

  // ---- the step loop ----
  int readback();          // p.ctrl -> *hctrl, and wait for it
  // Hairer initial step; leaves dt in ctrl.  Costs one probe eval (upstream: +1 NFE).
  int initial_step();
  // one dopri5 step, entirely on the device: six stages, error norms, controller (accept / dt / targets passed),
  // dense output, commit.  The host learns nothing here; see run_steps().
  int enqueue_step(const StepIO& io);
  // Advance the current interval to its last target.  `guess` steps are enqueued before the first read-back (what the
  // previous solve of the same problem needed: one synchronisation per solve in steady state), then two at a time;
  // steps enqueued past the end return at once on the device (Ctrl::done).  On return *hctrl holds the final record.
  int run_steps(const StepIO& io, long long max_steps, int guess, int* status);
  // host -> device: the interval's target times (and, once per solve, the replay list)
  int upload(double* dst, const double* src, int n, double* stage);
  // one interval of the fixed-grid RK4 (3/8 rule): state advanced in place
  int rk4_interval(double t0, double t1, const float* dot_with = nullptr, float* dot_out = nullptr);
};

// the caller's dt log (node_solve_opts::dt_log): negative entries are rejected steps
struct DtLog {
  const node_solve_opts* o;
  int n = 0;
  explicit DtLog(const node_solve_opts* opts) : o(opts) { if (o && o->n_dt_log) *o->n_dt_log = 0; }
  void add(double dt, bool accepted) {
    if (!o || o->record_dt <= 0 || !o->dt_log) return;
    if (n < o->record_dt) o->dt_log[n] = accepted ? dt : -dt;
    ++n;
    if (o->n_dt_log) *o->n_dt_log = n < o->record_dt ? n : o->record_dt;
  }
};

}  // namespace node
