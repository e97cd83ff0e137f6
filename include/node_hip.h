/*
 * node_hip.h -- C ABI of libnode_hip.so, the MI355X (gfx950) Neural-ODE
 * forward/adjoint integrator.
 *
 * This is the drop-in boundary for ONE path of fabiocarrara/neural-ode-features:
 *
 *     out = self.odeint(self.odefunc, x, self.integration_time,
 *                       method=self.method, rtol=self.tol, atol=self.tol)
 *                                                  -- reference model.py:367
 *
 * i.e. `torchdiffeq.odeint` / `odeint_adjoint` (imported at model.py:3, an
 * un-vendored third-party package) driving the Conv-GroupNorm-ReLU dynamics
 * `ODEfunc.forward` (model.py:339-348) built from `ConcatConv2d`
 * (model.py:313-323) and `nn.GroupNorm(min(32, C), C)` (model.py:268-271).
 *
 * Plain C: pointers and sizes only, no torch / C++ types.  The reference is
 * Python, so its FFI for this path is `ctypes`; the binding a maintainer adds
 * is shown in INTEGRATION.md and shipped as neural-ode-features_amd/_lib.py.
 *
 * Contract
 *  - every device buffer (inputs, outputs, workspace) is allocated and owned by
 *    the caller; the library never allocates or frees device memory and keeps
 *    no pointer after the call's work on `stream` has completed;
 *  - tensors are fp32, contiguous, NCHW exactly as PyTorch hands them over
 *    (the library converts to its internal NHWC layout inside the workspace);
 *  - `params` points INTO the live nn.Parameter storages (no copies), in the
 *    reference's layouts: conv weights are [C, C+1, 3, 3] with input channel 0
 *    being the time channel (model.py:321-322);
 *  - all work is enqueued on the caller's HIP stream (`hipStream_t` passed as
 *    void*).  The adaptive step loop runs WITHOUT host decisions: accept /
 *    reject, the next step size, which output times a step passed, dense
 *    output and the end of the interval are all decided by kernels; the host
 *    enqueues as many steps as the previous solve of the same problem needed,
 *    then synchronises once to read the controller record (and tops up two
 *    steps at a time if the interval is not finished; steps enqueued past the
 *    end return at once on the device).  `stats` is valid on return;
 *  - return 0 on success, a negative NODE_ERR_* otherwise; the message is
 *    available from node_last_error() (thread-local).  No exceptions, no abort.
 */
#ifndef NODE_HIP_H
#define NODE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NODE_ABI_VERSION 6

/* method -- the two solver names that reach model.py:367 on the graded configs
 * (`'dopri5'` train.py:219 default; `'rk4'` BASELINE.json configs[0]). */
enum { NODE_METHOD_DOPRI5 = 0, NODE_METHOD_RK4 = 1 };

enum {
  NODE_OK = 0,
  NODE_ERR_NULL = -1,         /* a required pointer is NULL                      */
  NODE_ERR_SHAPE = -2,        /* n/c/h/w/groups inconsistent                      */
  NODE_ERR_UNSUPPORTED = -3,  /* shape outside what the gfx950 kernels tile       */
  NODE_ERR_WORKSPACE = -4,    /* ws_bytes < node_workspace_bytes(...)             */
  NODE_ERR_MAX_STEPS = -5,    /* max_num_steps exceeded                           */
  NODE_ERR_NONFINITE = -6,    /* non-finite state / error norm                    */
  NODE_ERR_DT_UNDERFLOW = -7, /* t + dt == t  (upstream: 'underflow in dt')       */
  NODE_ERR_HIP = -8,          /* a HIP runtime call failed                        */
  NODE_ERR_ARG = -9           /* bad scalar argument (method, n_t, time order...) */
};
#define NODE_PENDING 1        /* node_stats.status of a solve enqueued with node_solve_opts.blind_steps */

/* State shape [n, c, h, w]; groups = min(32, c) (model.py:271); eps = 1e-5. */
typedef struct node_shape {
  int32_t n, c, h, w;
  int32_t groups;
  float eps;
} node_shape;

/* The ten parameters of ODEfunc in `ODEfunc.parameters()` order
 * (model.py:331-336).  Device pointers. */
typedef struct node_params {
  const float* norm1_w; /* [C] */
  const float* norm1_b; /* [C] */
  const float* conv1_w; /* [C, C+1, 3, 3], input channel 0 = time */
  const float* conv1_b; /* [C] */
  const float* norm2_w;
  const float* norm2_b;
  const float* conv2_w;
  const float* conv2_b;
  const float* norm3_w;
  const float* norm3_b;
} node_params;

/* Solver telemetry.  `nfe` follows the reference's counter (model.py:340): one
 * per ODEfunc.forward, including the recompute inside every adjoint eval. */
typedef struct node_stats {
  int32_t nfe;
  int32_t accepted;
  int32_t rejected;
  int32_t status;   /* NODE_OK or the NODE_ERR_* that stopped the solve */
  double last_dt;   /* step size proposed for the step after the last one */
  double t_final;   /* solver time reached */
  double first_dt;  /* initial step chosen (dopri5) */
} node_stats;

/* What a solve that was enqueued WITHOUT a final synchronisation (node_solve_opts.blind_steps) leaves in device
 * memory, written on the stream behind its last step.  `steps` = steps actually tried (steps enqueued past the end
 * of the interval return at once).  `miss` != 0: the steps enqueued did not finish the interval, or it stopped with
 * `status` -- its outputs must not be used. */
typedef struct node_step_record {
  int32_t done, status, steps, accepted, rejected, miss;
  double t, dt, first_dt;
  double t_prev, dt_used;   /* start and size of the last step tried (solver time: -t for a solve towards smaller t): when it was
                             * accepted, t_prev + dt_used - (end of the interval) is how far the solve overshot its end -- a small
                             * fraction of dt_used means the NEXT solve of this kind may need one step more */
} node_step_record;

/* Optional knobs (pass NULL for upstream behaviour). */
typedef struct node_solve_opts {
  int32_t max_num_steps;    /* <=0: 2^31-1 like upstream                          */
  int32_t n_forced_dt;      /* >0: replay mode -- take exactly these step sizes,  */
  const double* forced_dt;  /*     every step accepted (host pointer)             */
  int32_t record_dt;        /* >0: capacity of dt_log                             */
  double* dt_log;           /* host: dt tried at each step (<0 => rejected)       */
  int32_t* n_dt_log;        /* host: number of entries written                    */
  /* Deferred completion (dopri5, n_t == 2, no replay / dt log): enqueue exactly `blind_steps` steps and RETURN
   * WITHOUT SYNCHRONISING.  The caller keeps its queue fed across the solve and learns the outcome later from
   * `record` (device memory, filled on the stream); `miss_flag` (device float, nullable) is incremented when the
   * record says miss, so that work which commits results (node_sgd_step's skip flag) can be predicated on the
   * device.  stats then hold the counts as if all `blind_steps` had been needed (nfe = 2 + 6 blind_steps ...),
   * status NODE_PENDING; the true step count is in `record` (steps past the end of the interval return at once). */
  int32_t blind_steps;
  node_step_record* record; /* device */
  float* miss_flag;         /* device, nullable */
  /* node_solve_adjoint only: the caller keeps just the last state of the trajectory (`out[-1]`, what ODEBlock returns
   * with return_last_only, model.py:368-369), so dL/dy_out is zero in every other slice: `grad_out` then points to
   * that ONE slice [n, c, h, w] and the zero slices are neither materialised by the caller nor read here. */
  int32_t grad_last_only;
  /* GLOBAL-NORM mode of a data-parallel solve (ABI 6; dopri5; SURVEY.md 8e, collective 2): every rank integrates its shard of the
   * batch, and the sums the step controller decides from -- sum (err / tol)^2 of every state segment, the sums of Hairer's
   * initial step -- are added over the ranks before each decision, so that ALL RANKS TAKE IDENTICAL STEPS (no straggler, and for
   * the sharded segments y and adj_y exactly the mixed norm of the unsharded batch).  The library packs its local sums into
   * `norm_buf` (device, >= 8 floats) on the stream and calls `norm_reduce(ctx, norm_buf, 8, stream)`, which must leave the SUM
   * over the `norm_world` ranks in the buffer, enqueued on (or ordered behind) that stream; the next launch reads it.  Called from
   * inside node_solve_fwd / node_solve_adjoint on the calling thread: twice per interval for the initial step, once per step.
   * The segments every rank holds as its own partial (adj_params, adj_t) enter with the mean of the ranks' ratios; the fp16-pair
   * "repeat this step" flag of any rank repeats the step on all.  NULL: local norms (upstream behaviour per process). */
  void (*norm_reduce)(void* ctx, float* norm_buf, int32_t n, void* stream);
  void* norm_reduce_ctx;
  float* norm_buf;
  int32_t norm_world;
} node_solve_opts;

/* Per-kernel-class timing collected with HIP events on the caller's stream
 * (bench.py's roofline block).  Classes: 0 conv3x3 fwd/dgrad as one fused kernel,
 * 1 wgrad GEMM, 2 the component GEMMs of a conv3x3 fwd/dgrad that runs as the
 * F(4x4,3x3) pipeline (`flops` counts the convolution's, as for class 0);
 * 3..8 the HBM-bound GroupNorm / transform passes of that pipeline, one class per
 * kernel instance (3 combine, 4 forward pass, 5 forward pass + next combine,
 * 6 forward pass + backward top, 7 backward pass, 8 backward pass + next combine):
 * for these `flops` holds the ALGORITHMIC BYTES of the launches (every tensor the
 * pass must read or write, once). */
#define NODE_PROFILE_CLASSES 9
typedef struct node_profile {
  int64_t launches[NODE_PROFILE_CLASSES];
  double total_ms[NODE_PROFILE_CLASSES];
  double flops[NODE_PROFILE_CLASSES]; /* algorithmic FLOPs (classes 0..2) / bytes (3..8) of those launches */
} node_profile;

int node_abi_version(void);
const char* node_last_error(void);

/* Number of fp32 elements of the flat parameter vector (18*C*C + 26*C). */
size_t node_param_count(const node_shape* shape);

/* Bytes of caller-provided device workspace needed by the calls below.
 * adjoint != 0 sizes for node_solve_adjoint / node_odefunc_vjp. */
size_t node_workspace_bytes(const node_shape* shape, int method, int adjoint, int n_t);

/* 1 when a dopri5 forward solve of this shape runs as ONE resident launch on the current device (the bs = 1 census of
 * evaluate.py:97-142: f0, the initial step, every step with its decision and dense output inside one kernel), else 0. */
int node_solve_is_resident(const node_shape* shape);

/* f = ODEfunc(t, y)                                     -- model.py:339-348 */
int node_odefunc_fwd(const node_shape* shape, const node_params* params, float t,
                     const float* y, float* f,
                     void* ws, size_t ws_bytes, void* stream);

/* What the upstream adjoint asks autograd for at every stage:
 *   f = ODEfunc(t, y);  (vjp_t, vjp_y, vjp_params) = grad(f, (t, y, *params), cot)
 * vjp_t: 1 float (device); vjp_params: node_param_count floats (device), flat in
 * parameters() order, each parameter in its PyTorch layout. */
int node_odefunc_vjp(const node_shape* shape, const node_params* params, float t,
                     const float* y, const float* cot,
                     float* f, float* vjp_y, float* vjp_t, float* vjp_params,
                     void* ws, size_t ws_bytes, void* stream);

/* Diagnostics (tests, tools): y = conv3x3(x, weight[:, 1:], padding = 1) for an [n, c, 8, 8] (n % 8 == 0) or [n, c, 16, 16]
 * (n % 2 == 0) tensor, c % 64 == 0, through the
 * Winograd F(4x4,3x3) pipeline the solver uses when its tolerance allows (csrc/wino4.h); dgrad != 0: the data
 * gradient (transposed convolution) instead.  weight is a ConcatConv2d filter [c][c+1][3][3] (model.py:320-323). */
size_t node_conv3x3_w4_workspace_bytes(const node_shape* shape);
int node_conv3x3_w4(const node_shape* shape, const float* weight, int dgrad, const float* x, float* y,
                    void* ws, size_t ws_bytes, void* stream);

/* Diagnostics (tests): the exact three-way bf16 split (x = h + m + l) the component GEMMs of that pipeline apply to
 * their fp32 operands on the device, element by element: out[3 i + p] = part p of x[i], widened to float.
 * x: n floats, out: 3 n floats (device); n a positive multiple of 8. */
int node_w4_split3(const float* x, float* out, size_t n, void* stream);

/* Diagnostics (tests): the launches that move a solve's tensors into and out of the state layout of the F(4x4,3x3) passes, and
 * the border maps its set-up launch forms, on the caller's device buffers.  [n, c, 8, 8] or [n, c, 16, 16], c % 16 == 0.
 *   node_w4s_layout       one tensor, NCHW -> state layout (to_nchw == 0) or back; src, dst: n c h w floats.
 *   node_w4s_layout_jobs  njobs (1 or 2) tensors NCHW -> state layout in ONE launch; src[i], dst[i] as above (host arrays of
 *                         device pointers); copies[2 i], copies[2 i + 1]: NCHW buffers that receive job i's source too, or NULL.
 *   node_w4s_tmaps        tmap: [2][h w][c], the border-aware time-channel maps of two ConcatConv2d filters [c][c+1][3][3];
 *                         tmap_s: [2][h w c], the same maps in the blocking the passes read, formed by the same launch. */
int node_w4s_layout(const node_shape* shape, const float* src, float* dst, int to_nchw, void* stream);
int node_w4s_layout_jobs(const node_shape* shape, int njobs, const float* const* src, float* const* dst, float* const* copies,
                         void* stream);
int node_w4s_tmaps(const node_shape* shape, const float* conv1_w, const float* conv2_w, float* tmap, float* tmap_s, void* stream);

/* Diagnostics (tests; ABI 6): what the last node_solve_adjoint of the process did with the fp16-PAIR operand format of the
 * F(4x4,3x3) pipeline (csrc/wino4.h): out[0] = 1 when the solve used it, out[1] = steps the device controller REPEATED because a
 * cotangent left the range of its power-of-two scale (such a step is not a solver step: it appears in no statistic), out[2] = the
 * cotangent exponent at the end, out[3] = 0.  Filled only by solves that ran with NODE_TUNE_W4_STATS=1 in the environment (two
 * words more in the final read-back); -1 in out[1] otherwise.  NODE_TUNE_W4_GSKEW=k (diagnostics) starts every interval with the
 * cotangent exponent k too high, so that its first step overflows and is repeated. */
int node_w4_pair_stats(int32_t* out4);

/* Diagnostics (tests, tools; ABI 6): which kernel instances and which tiling the library selects for a shape in THIS process (the
 * NODE_TUNE_* switches that move the geometry are read as the solver reads them), without touching a device.  The launchers switch on
 * the same two values (csrc/kernels_wgrad.hip wgrad_kernel_for, csrc/conv_select.hip conv_kernel_for), so what this reports is what
 * runs.  wgrad_kernel: the fp32 weight-gradient instance -- k_wgrad_w2<units of 8 | 4>, k_wgrad_w<W, RB>, k_wgrad_t<W, RB>, k_wgrad_p.
 * conv_kernel: the fp32 3x3 convolution instance -- direct / 1-D Winograd at 64-, 128- or 256-row tiles, 2-D Winograd (128 rows).
 * The other fields are the solver's Dims of the same names (csrc/node_internal.h); wino4 != 0 says that the F(4x4,3x3) pipeline
 * (and, for c % 128 == 0, its own weight gradient) may serve the shape instead.  Returns the error the solver would give the shape. */
enum { NODE_WGRAD_W2_8 = 0, NODE_WGRAD_W2_4, NODE_WGRAD_W_8_8, NODE_WGRAD_W_16_2, NODE_WGRAD_W_4_4,
       NODE_WGRAD_T_8_8, NODE_WGRAD_T_16_4, NODE_WGRAD_T_7_7, NODE_WGRAD_T_4_4, NODE_WGRAD_P, NODE_WGRAD_KERNELS };
enum { NODE_CONV_DIRECT_64 = 0, NODE_CONV_DIRECT_128, NODE_CONV_DIRECT_256, NODE_CONV_W1_64, NODE_CONV_W1_128, NODE_CONV_W1_256,
       NODE_CONV_W2_128, NODE_CONV_KERNELS };
typedef struct node_dims_info {
  int32_t wgrad_kernel, conv_kernel;
  int32_t wino, bm, s, csplit, mtiles, ntile, small, tiny, wino4, w4q, wgrad_wino, wut, rb, nbands, nsplit, wgrad_pair;
} node_dims_info;
int node_describe_dims(const node_shape* shape, node_dims_info* out);

/* torchdiffeq.odeint(ODEfunc, y0, t, rtol, atol, method)  -- model.py:367
 * t_pts: host array of n_t strictly monotonic times; y_out: [n_t, n, c, h, w]
 * with y_out[0] = y0. */
int node_solve_fwd(const node_shape* shape, const node_params* params,
                   const float* y0, const float* t_pts, int n_t,
                   float rtol, float atol, int method, const node_solve_opts* opts,
                   float* y_out, node_stats* stats,
                   void* ws, size_t ws_bytes, void* stream);

/* Backward of torchdiffeq.odeint_adjoint (triggered by train.py:51):
 * y_traj = the forward's y_out, grad_out = dL/dy_out, both [n_t, n, c, h, w].
 * Outputs: grad_y0 [n, c, h, w]; grad_params [node_param_count] flat in
 * parameters() order; grad_t [n_t] or NULL (the reference discards it).
 * grad_t is dL/dt_pts in upstream's `time_vjps` order, in the CALLER's time for an increasing and for a decreasing grid alike:
 *   grad_t[i] = <f(t_i, y_i), dL/dy_i>  for i >= 1 (exactly 0 for a slice that opts->grad_last_only declares zero),
 *   grad_t[0] = adj_time, the scalar segment of the augmented state: it starts at 0, loses <f(t_i, y_i), dL/dy_i> at the start
 *               of every interval [t_i -> t_{i-1}] and is integrated through it with d adj_time / dt = -adj_y . df/dt.
 * Sign convention: an interval that runs towards smaller t (every interval of an increasing grid) is solved in s = -t with the
 * dynamics tsign * f(tsign * s, .), tsign = -1, as upstream does; the interval's first stage then holds tsign * f, the dot
 * product is taken from it and multiplied by tsign again, and the time component of the augmented dynamics carries the same
 * factor -- so no entry of grad_t changes sign with the direction of the solve (tests/test_gpu_adjoint_time.py). */
int node_solve_adjoint(const node_shape* shape, const node_params* params,
                       const float* y_traj, const float* grad_out,
                       const float* t_pts, int n_t,
                       float rtol, float atol, int method, const node_solve_opts* opts,
                       float* grad_y0, float* grad_params, float* grad_t,
                       node_stats* stats,
                       void* ws, size_t ws_bytes, void* stream);

/* Backward of torchdiffeq.odeint with adjoint=False (the constructor default, model.py:7; selected at model.py:359):
 * upstream backpropagates through the solver's operations.  The accepted steps of the forward solve are replayed
 * from y0 (`step_dt`: their sizes as node_solve_fwd logged them through node_solve_opts.dt_log, accepted ones only,
 * `n_steps` of them; ignored for rk4, whose grid is t_pts), all stage derivatives are kept, and the cotangent
 * grad_out [n_t, n, c, h, w] is carried back through every step: grad_y0 [n, c, h, w], grad_params flat in
 * parameters() order.  Step sizes are constants of the differentiation.  `rtol`, `atol`: the forward solve's -- they
 * select the convolution kernels exactly as node_solve_fwd did (the F(4x4,3x3) pipeline for dopri5 at rtol, atol >=
 * 1e-5 on 8x8 and 16x16 states), so the replayed stage values are the ones the forward output was computed from.  Workspace:
 * node_backprop_workspace_bytes (it holds the tape: 7 state-sized tensors per step). */
size_t node_backprop_workspace_bytes(const node_shape* shape, int method, int n_t, int n_steps);
int node_solve_backprop(const node_shape* shape, const node_params* params,
                        const float* y0, const float* t_pts, int n_t,
                        const double* step_dt, int n_steps, float rtol, float atol, int method,
                        const float* grad_out, float* grad_y0, float* grad_params,
                        void* ws, size_t ws_bytes, void* stream);

/* Classifier head behind the ODE block, up to (not including) the Linear layer
 *   -- model.py:231-250 (FCClassifier): GroupNorm(min(32,C), C) [model.py:268-271] -> ReLU ->
 *      AdaptiveAvgPool2d((1,1)) -> [Dropout] -> Flatten.
 * z: [n, c, h, w] (NCHW); gamma, beta: [c]; scale: [n, c] dropout mask / (1 - p) as the
 * caller's RNG produced it, or NULL (eval mode / no dropout); pooled: [n, c];
 * stats: [n, groups, 2] (mean, 1/sigma), kept by the caller for the backward.
 * No workspace; one launch each on `stream`. */
int node_head_fwd(const node_shape* shape, const float* z, const float* gamma, const float* beta,
                  const float* scale, float* pooled, float* stats, void* stream);

/* Backward of node_head_fwd: g_pooled [n, c] = dL/dpooled.  Outputs dz [n, c, h, w], the
 * per-sample partials gpart [n, 2, c] of (dL/dgamma, dL/dbeta) and -- gsum != NULL, a second small
 * launch -- their sums over n, gsum [2, c] = (dL/dgamma, dL/dbeta). */
int node_head_bwd(const node_shape* shape, const float* z, const float* gamma, const float* beta,
                  const float* scale, const float* stats, const float* g_pooled,
                  float* dz, float* gpart, float* gsum, void* stream);

/* GroupNorm (+ReLU) of the stem's residual blocks -- model.py:284-310 (`relu(norm(x))` in front of every
 * conv; normalization('group') = nn.GroupNorm(min(32,C), C), model.py:268-271), forward and backward.
 * z, out, g_out, dz: [n, c, h, w] (NCHW); stats: [n, groups, 2] (mean, 1/sigma) from the forward;
 * gpart: [n, 2, c] per-sample partials of (dL/dgamma, dL/dbeta); gsum: NULL, or [2, c] for their sums over n (a second
 * small launch).  relu != 0: out = relu(GN(z)); relu == 0: out = GN(z).  No workspace; one launch each. */
int node_gn_relu_fwd(const node_shape* shape, const float* z, const float* gamma, const float* beta,
                     int relu, float* out, float* stats, void* stream);
int node_gn_relu_bwd(const node_shape* shape, const float* z, const float* gamma, const float* beta,
                     const float* stats, int relu, const float* g_out, float* dz, float* gpart, float* gsum, void* stream);

/* Generic ("flat") solver -- the fallback of SURVEY.md 8b: `torchdiffeq.odeint[_adjoint]` accepts ANY nn.Module as `func`
 * (model.py:367), and the reference itself offers dynamics the fused kernels do not take (train.py:202 `--norm batch`).
 * For those the CALLER evaluates the dynamics (PyTorch ops on its stream) and this library does everything else on the
 * device with the kernels of the fused solves: stage states y + dt sum_j beta_ij k_j, stage times, the Hairer initial
 * step, the mixed error norm per tensor, accept / reject, the next step size, quartic dense output at the target times,
 * FSAL commit -- no host decision; the host reads the controller back when it likes (node_flat_status_read).
 * State: 1..3 flat fp32 tensors (`seg`), each with an end-of-step buffer y1 and seven stage-derivative buffers k[0..6]
 * owned by the caller, plus -- has_scalar -- one scalar kept inside the controller (the adjoint's time cotangent).
 * Time is in SOLVER ORIENTATION: increasing; a solve towards smaller t passes tsign = -1, negated times and derivatives
 * (upstream's convention), and node_flat_stage hands out tsign * time for the caller's function.
 * dopri5 step:  for s in 0..5: node_flat_stage(s) -> caller evaluates -> stores tsign * f into k[s + 1] (stage 5's state
 * must be written to the seg's y1 buffers: it IS y1); node_flat_finish_step.  Before the first step: stage NODE_FLAT_F0
 * (k[0]), then node_flat_initial_step(0), stage NODE_FLAT_PROBE (k[1]), node_flat_initial_step(1) unless first_dt is given.
 * rk4 (3/8 rule, one step per target interval): stage F0 -> k[0], stages 1..3 -> k[1..3], finish. */
typedef struct node_flat_seg {
  float* y;        /* state at the start of the current step (updated in place by the commit)   */
  float* y1;       /* state at the end of the step                                               */
  float* k[7];     /* stage derivatives                                                          */
  size_t n;
} node_flat_seg;
typedef struct node_flat_solve {
  int32_t nseg;          /* 1..3                                                                 */
  int32_t has_scalar;    /* != 0: augmented (adjoint) solve -- scalar segment, dense output of every segment at the interval's end */
  node_flat_seg seg[3];
  float rtol, atol, tsign;
  int32_t n_targets;     /* output times of the current interval                                 */
  void* ws;              /* node_flat_workspace_bytes(n_targets) bytes, 256-byte aligned          */
  size_t ws_bytes;
} node_flat_solve;
typedef struct node_flat_status {
  int32_t done, status, steps, accepted, rejected;
  double t, dt, first_dt;
  float scalar;
} node_flat_status;
enum { NODE_FLAT_F0 = -1, NODE_FLAT_PROBE = -2 };
size_t node_flat_workspace_bytes(int n_targets);
/* new interval starting at t0 (solver orientation) with `targets` (host array, increasing); first_dt = 0: to be chosen
 * by node_flat_initial_step.  new_solve != 0 also resets the cumulative counters and the scalar segment. */
int node_flat_begin(const node_flat_solve* f, double t0, const double* targets, double first_dt, int new_solve, void* stream);
/* y_stage[i] <- stage state of segment i (nothing for NODE_FLAT_F0); *t_stage (device float, nullable) <- tsign * stage time */
int node_flat_stage(const node_flat_solve* f, int method, int stage, float* const* y_stage, float* t_stage, void* stream);
/* scalar segment: which = -1 its value, 0..6 a stage derivative; (accumulate ? old : 0) + scale * src[0], src on the device */
int node_flat_scalar(const node_flat_solve* f, int which, const float* src, float scale, int accumulate, void* stream);
int node_flat_initial_step(const node_flat_solve* f, int phase, void* stream);
/* y_out (nullable, forward solves): [n_targets][seg[0].n], row j <- dense output at target j when a step passes it */
int node_flat_finish_step(const node_flat_solve* f, int method, float* y_out, void* stream);
int node_flat_status_read(const node_flat_solve* f, node_flat_status* out, void* stream);   /* synchronises the stream */

/* The classifier's Linear layer and the loss of the training loop as ONE launch each way -- model.py:244-250
 * (`nn.Linear(in_ch, out)` behind Flatten) and train.py:43 (`F.cross_entropy(p, y)`), plus the per-batch numbers the loop
 * reads at train.py:44,46 (loss value, correct predictions), left in device memory so that a caller can read them once
 * per logging interval instead of twice per batch.
 *   forward : logits[n][o] = sum_c pooled[n][c] weight[o][c] + bias[o]      (pooled == NULL: `logits` are given, not written)
 *             loss = mean_n | sum_n ( logsumexp_o logits[n] - logits[n][target[n]] )   (target == NULL: Linear alone)
 *             stat = { loss, #{n : argmax_o logits[n] == target[n]} }                   (optional)
 *   backward: d_logits = grad_loss * (softmax(logits) - onehot(target)) (/ n for the mean)   -- or `grad_logits` as given;
 *             d_weight[o][c] = sum_n d_logits[n][o] pooled[n][c], d_bias[o] = sum_n d_logits[n][o],
 *             d_pooled[n][c] = sum_o d_logits[n][o] weight[o][c]            (pooled == NULL: only `d_logits` is written)
 * fp32 throughout; class indices are int64 (what PyTorch hands over), every index in [0, classes) (no ignore_index:
 * an out-of-range target makes the loss NaN); classes <= 1024.  All sums in a fixed order: bit-reproducible.
 * `scratch`: node_head_loss_scratch_bytes(n) bytes of device memory, ZERO before its first use (the kernel leaves its
 * arrival counter at zero again), not shared between streams. */
enum { NODE_REDUCE_MEAN = 0, NODE_REDUCE_SUM = 1 };
typedef struct node_head_loss {
  int32_t n, c, classes;
  int32_t reduction;       /* NODE_REDUCE_MEAN (train.py:43) or NODE_REDUCE_SUM (train.py:93 test loss)            */
  const float* pooled;     /* [n, c]  what the head's pooling / dropout produced (node_head_fwd), or NULL          */
  const float* weight;     /* [classes, c]  nn.Linear.weight                                                      */
  const float* bias;       /* [classes] or NULL                                                                   */
  const int64_t* target;   /* [n] class indices, or NULL                                                          */
  float* logits;           /* [n, classes]                                                                        */
  float* loss;             /* [1]   (written when target != NULL)                                                 */
  float* stat;             /* [2] or NULL                                                                         */
  float* scratch;          /* node_head_loss_scratch_bytes(n)   (needed when target != NULL)                      */
} node_head_loss;
typedef struct node_head_loss_grad {
  const float* grad_loss;    /* [1] upstream gradient of the scalar loss (device), NULL = 1                       */
  const float* grad_logits;  /* [n, classes] given instead of the loss gradient (Linear alone), or NULL          */
  float* d_logits;           /* [n, classes] or NULL                                                              */
  float* d_pooled;           /* [n, c]                                                                            */
  float* d_weight;           /* [classes, c]                                                                      */
  float* d_bias;             /* [classes] or NULL                                                                 */
} node_head_loss_grad;
size_t node_head_loss_scratch_bytes(int n);
int node_head_loss_fwd(const node_head_loss* head, void* stream);
int node_head_loss_bwd(const node_head_loss* head, const node_head_loss_grad* grads, void* stream);

/* node_head_loss_fwd for `slices` trajectories' slices in ONE launch: rows [s*n, (s+1)*n) are slice s, `target` [n] is shared.
 * logits [slices*n, classes] (computed from pooled [slices*n, c], or given with pooled == NULL); loss [slices] (NODE_REDUCE_SUM
 * only); stat [slices, 2] = {loss, hits}.  Every logit, loss[s] and stat[s] the bits of node_head_loss_fwd on slice s alone.
 * `scratch`: node_head_loss_slices_scratch_bytes(slices, n) bytes, ZERO before its first use, not shared between streams and
 * kept for ONE value of `slices` (the arrival counters, one per slice, lie in front of the partials; any n up to the one it
 * was sized for); needed when target != NULL; loss and stat are optional then, but one of them must be given; slices <= 65535. */
typedef struct node_head_loss_slices { int32_t slices, n, c, classes; const float *pooled, *weight, *bias; const int64_t* target;
                                       float *logits, *loss, *stat, *scratch; } node_head_loss_slices;
size_t node_head_loss_slices_scratch_bytes(int slices, int n);
int node_head_loss_slices_fwd(const node_head_loss_slices* head, void* stream);

/* u = relu(GroupNorm(z)) per sample for two trajectories a, b [rows, c, h, w] (rows = T*N), never written:
 * out [rows, 2] = { sqrt(sum (ub - ua)^2), cosine similarity of ua and ub as F.cosine_similarity defines it (eps 1e-8) }
 * -- diff.py:111-123's two numbers per (time slice, sample).  ONE launch, each trajectory read once, fixed summation order,
 * no atomics.  Shapes: those of node_head_fwd (shape->n = rows). */
int node_gn_relu_distance(const node_shape* shape /* n = rows */, const float* a, const float* b, const float* gamma,
                          const float* beta, float* out, void* stream);

/* The optimizer step of the training loop -- train.py:136 (`torch.optim.SGD(params, lr, momentum=0.9, weight_decay=wd)`)
 * stepped at train.py:56-58 -- for ALL parameter tensors of the model in one launch (per 64 tensors):
 *   g = grad_scale * grad + weight_decay * p;  buf = momentum * buf + g;  p -= lr * buf
 * (dampening 0, no Nesterov: the reference's settings).  `tensors` is a HOST array of `count` records of device
 * pointers; gradients are read where autograd / the data-parallel reducer left them.  grad_scale folds the
 * 1/world of a data-parallel gradient SUM into the step.  momentum_buf must start at zero (the first step then
 * equals PyTorch's buf = g); it may be NULL when momentum == 0 (torch.optim.SGD keeps no buffer then).  `skip_if_nonzero` (device float, nullable): the launch leaves everything untouched
 * when it reads a non-zero value there -- the commit point of a step whose solves ran with deferred completion. */
typedef struct node_sgd_tensor {
  float* param;
  const float* grad;
  float* momentum_buf;
  size_t n;
} node_sgd_tensor;
int node_sgd_step(const node_sgd_tensor* tensors, int count, float lr, float momentum, float weight_decay,
                  float grad_scale, const float* skip_if_nonzero, void* stream);

/* The reference's other optimizer -- train.py:138 (`Adam(params, lr, weight_decay=wd)`) -- in the same form: every parameter
 * tensor in one update launch (per 64 tensors), torch.optim.Adam's arithmetic with amsgrad off and coupled L2 weight decay:
 *   g = grad_scale * grad + weight_decay * p;  exp_avg += (1 - beta1) (g - exp_avg);  exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) g g
 *   t = step + 1;  p -= (lr / (1 - beta1^t)) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps)
 * `step` is a one-element fp32 counter per tensor in DEVICE memory (PyTorch's state['step']), read by the update launch and
 * advanced by one by a second, one-workgroup launch behind it; the bias corrections are formed in double from it.  exp_avg
 * and exp_avg_sq start at zero, step at 0.  beta1 / beta2 are read as the shortest decimal d that rounds to the float given
 * (0.999f means 0.999, the double a PyTorch caller holds): the kernel multiplies by (float)d and (float)(1 - d) and forms
 * d^t in double.  1 - beta2 formed from the float's own value, 0.99900001287, would be off by 1.3e-5 of itself, and
 * exp_avg_sq with it.  A float that is no short decimal is taken within half an ulp of its own value.  `skip_if_nonzero`
 * as for node_sgd_step: a skipped step changes nothing and advances no counter. */
typedef struct node_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  float* step;
  size_t n;
} node_adam_tensor;
int node_adam_step(const node_adam_tensor* tensors, int count, float lr, float beta1, float beta2, float eps,
                   float weight_decay, float grad_scale, const float* skip_if_nonzero, void* stream);

/* The residual stem in front of the ODE block -- model.py:167-178 (`ResDownsample`):
 *     nn.Conv2d(in_ch, 64, 3, 1)                                              bias, no padding
 *     ResBlock(64, 64,      stride=2, downsample=conv1x1(64, 64, 2))          model.py:284-310
 *     ResBlock(64, filters, stride=2, downsample=conv1x1(64, filters, 2))
 * with ResBlock.forward (model.py:297-310): out = relu(norm1(x)); shortcut = downsample(out);
 * out = conv2(relu(norm2(conv1(out)))); return out + shortcut  -- conv3x3 / conv1x1 without bias (model.py:255-265),
 * norm = nn.GroupNorm(min(32, C), C) (model.py:268-271).  Forward and backward as hand-written gfx950 kernels, NHWC
 * inside the workspace: every convolution and data gradient on the bf16 matrix pipe at fp32 accuracy (activations,
 * gradients and filters as exact three-way bf16 splits, six products), weight gradients on the fp32 matrix
 * instructions.  x: [n, in_ch, h, w] NCHW (in_ch <= 3), out / grad_out: [n, filters, h2, w2] NCHW with
 * h0 = h - 2, h1 = (h0 - 1) / 2 + 1, h2 = (h1 - 1) / 2 + 1 (32 -> 30 -> 15 -> 8); filters % 64 == 0.
 * node_stem_bwd needs the workspace exactly as node_stem_fwd left it (the caller keeps it between the two calls);
 * every gradient pointer receives the full gradient (written, not accumulated). */
typedef struct node_stem_shape {
  int32_t n, in_ch, h, w, filters;
  float eps;
} node_stem_shape;
typedef struct node_stem_params {       /* state_dict keys under `downsample.module.` */
  const float* conv0_w;  /* 0.weight            [64, in_ch, 3, 3] */
  const float* conv0_b;  /* 0.bias              [64]              */
  const float* b1_n1_w;  /* 1.norm1.weight      [64]              */
  const float* b1_n1_b;  /* 1.norm1.bias        [64]              */
  const float* b1_c1_w;  /* 1.conv1.weight      [64, 64, 3, 3]    */
  const float* b1_n2_w;  /* 1.norm2.weight      [64]              */
  const float* b1_n2_b;  /* 1.norm2.bias        [64]              */
  const float* b1_c2_w;  /* 1.conv2.weight      [64, 64, 3, 3]    */
  const float* b1_ds_w;  /* 1.downsample.weight [64, 64, 1, 1]    */
  const float* b2_n1_w;  /* 2.norm1.weight      [64]              */
  const float* b2_n1_b;  /* 2.norm1.bias        [64]              */
  const float* b2_c1_w;  /* 2.conv1.weight      [filters, 64, 3, 3] */
  const float* b2_n2_w;  /* 2.norm2.weight      [filters]         */
  const float* b2_n2_b;  /* 2.norm2.bias        [filters]         */
  const float* b2_c2_w;  /* 2.conv2.weight      [filters, filters, 3, 3] */
  const float* b2_ds_w;  /* 2.downsample.weight [filters, 64, 1, 1] */
} node_stem_params;
typedef struct node_stem_grads {        /* same order and shapes as node_stem_params; device pointers, all required */
  float* conv0_w; float* conv0_b;
  float* b1_n1_w; float* b1_n1_b; float* b1_c1_w; float* b1_n2_w; float* b1_n2_b; float* b1_c2_w; float* b1_ds_w;
  float* b2_n1_w; float* b2_n1_b; float* b2_c1_w; float* b2_n2_w; float* b2_n2_b; float* b2_c2_w; float* b2_ds_w;
} node_stem_grads;
size_t node_stem_workspace_bytes(const node_stem_shape* shape);
int node_stem_fwd(const node_stem_shape* shape, const node_stem_params* params, const float* x, float* out,
                  void* ws, size_t ws_bytes, void* stream);
int node_stem_bwd(const node_stem_shape* shape, const node_stem_params* params, const float* x, const float* grad_out,
                  const node_stem_grads* grads, void* ws, size_t ws_bytes, void* stream);
/* node_stem_bwd plus the gradient of the image, d_x [n, in_ch, h, w] NCHW fp32 (required; written, not accumulated): behind
 * the data-gradient chain that ends at the first layer's output, one more kernel -- the transposed first layer
 *     d_x[n][ci][y][x] = sum_co sum_ky,kx dh0[n][y - ky][x - kx][co] * w0[co][ci][ky][kx]
 * in fp32 without atomics (the same bits on every run).  grads may be NULL (saliency maps, adversarial attacks: frozen
 * parameters): then only the data-gradient chain runs -- the dgrad convolutions, the GroupNorm backward passes, the
 * F(4x4,3x3) dgrad where the stem takes that pipeline -- and no weight-gradient or slab-reduction launch.  With grads given,
 * the parameter gradients are node_stem_bwd's bit for bit.  Same workspace contract as node_stem_bwd. */
int node_stem_bwd_dx(const node_stem_shape* shape, const node_stem_params* params, const float* x, const float* grad_out,
                     const node_stem_grads* grads, float* d_x, void* ws, size_t ws_bytes, void* stream);
/* Diagnostics (host only, needs no GPU): the launch plan of node_stem_fwd / node_stem_bwd for a shape, in this process.
 * One node_stem_gn_info per GroupNorm + ReLU launch, in the order of the tensors they normalise (block 1 norm1, norm2, block 2
 * norm1, norm2): hw pixels per sample, channels, cpg channels per group, cb the channel block one workgroup holds in LDS,
 * blocks_per_sample = channels / cb, grid = n * blocks_per_sample workgroups; the backward launch of the same norm has the same
 * geometry and (2 hw cb + 1024) * 4 bytes of LDS, the forward (hw cb + 512) * 4.  takes_w4: the last convolution (and with it
 * the fourth norm) runs through the F(4x4,3x3) pipeline instead, so gn[3] describes launches that do not happen and
 * wgrad_nsplit[3] slabs nobody fills.  wgrad_nsplit / wgrad_rows_per_split [i]: the split-K plan of the weight gradient of
 * b1_c1_w (with b1_ds_w), b1_c2_w, b2_c1_w (with b2_ds_w), b2_c2_w.  Returns what node_stem_fwd would return for the shape
 * (NODE_ERR_SHAPE, NODE_ERR_UNSUPPORTED: the shapes node_stem_workspace_bytes answers with 0), with `out` zeroed. */
typedef struct node_stem_gn_info {
  int32_t hw, channels, cpg, cb, blocks_per_sample, grid;
} node_stem_gn_info;
typedef struct node_stem_info {
  node_stem_gn_info gn[4];
  int32_t takes_w4;
  int32_t wgrad_nsplit[4];
  int32_t wgrad_rows_per_split[4];
} node_stem_info;
int node_stem_describe(const node_stem_shape* shape, node_stem_info* out);

/* The residual stem above for images the resident GroupNorm passes refuse -- 64 x 64 inputs (tiny-imagenet-200, CIFAR-10 resized
 * for the transfer evaluation): 62 x 62 = 3844 pixels behind the first layer.  The same plan, kernels, arguments and workspace
 * contract as node_stem_fwd / node_stem_bwd / node_stem_bwd_dx (grads NULL in node_stem_banded_bwd_dx: the data-gradient chain
 * alone, d_x the same bits); each of the four GroupNorm + ReLU passes is the resident launch where its (sample, channel block)
 * fits the LDS and otherwise a BANDED pair of launches (csrc/kernels_stem_banded.hip): a workgroup takes (sample, band of band_px
 * consecutive pixels, cb channels) and holds nothing of the tensor.  Forward: per-band (mean, centred second moment) of every group,
 * then every workgroup merges its groups' partials with Chan's formula in band order and normalises its band.  Backward: per-band
 * channel sums, then every workgroup adds them in band order and writes its band of the gradient.  No atomics, no workgroup waits
 * for another, every sum in one order: the same bits on every run.  LDS per workgroup does not depend on the image.
 *   n >= 1; in_ch <= 3; h, w >= 5, no upper limit; filters a power of two in [64, 4096]; EVERY tensor of the plan under 2^31
 *   elements -- (n h0 w0 + 1) 64, (n h1 w1 + 1) 64, (n h2 w2 + 1) filters.  NODE_ERR_SHAPE / NODE_ERR_UNSUPPORTED as node_stem_fwd
 *   returns them for the same defect; the workspace-size call returns 0 then.
 * NODE_TUNE_STEM_BAND_PX (default 128): pixels per band.  NODE_TUNE_STEM_BANDED=all: every pass banded, whatever fits (tests, A/B).
 * Both are read once per call and are part of the workspace layout: a backward runs under the values its forward ran under.
 * The describe call (host only, needs no GPU): per norm the node_stem_gn_info of the launch that runs -- resident: node_stem_describe's
 * record, banded = 0 and the other fields 0; banded: cb the banded passes' channel block (max(64, cpg)), blocks_per_sample =
 * channels / cb, grid = n * bands_per_sample * blocks_per_sample, which is grid_first and grid_second, the grids of the two launches
 * of either direction -- then takes_w4 (the fourth norm then runs inside the F(4x4,3x3) pipeline and is never banded) and the
 * split-K plans as in node_stem_info.  Refusals leave `out` zeroed. */
typedef struct node_stem_banded_gn_info {
  node_stem_gn_info gn;
  int32_t banded, band_px, bands_per_sample, grid_first, grid_second;
} node_stem_banded_gn_info;
typedef struct node_stem_banded_info {
  node_stem_banded_gn_info gn[4];
  int32_t takes_w4;
  int32_t wgrad_nsplit[4];
  int32_t wgrad_rows_per_split[4];
} node_stem_banded_info;
size_t node_stem_banded_workspace_bytes(const node_stem_shape* shape);
int node_stem_banded_describe(const node_stem_shape* shape, node_stem_banded_info* out);
int node_stem_banded_fwd(const node_stem_shape* shape, const node_stem_params* params, const float* x, float* out,
                         void* ws, size_t ws_bytes, void* stream);
int node_stem_banded_bwd(const node_stem_shape* shape, const node_stem_params* params, const float* x, const float* grad_out,
                         const node_stem_grads* grads, void* ws, size_t ws_bytes, void* stream);
int node_stem_banded_bwd_dx(const node_stem_shape* shape, const node_stem_params* params, const float* x, const float* grad_out,
                            const node_stem_grads* grads, float* d_x, void* ws, size_t ws_bytes, void* stream);

/* Diagnostics (tests, tools): the transposed first layer alone on NCHW tensors.  w0: [64, in_ch, 3, 3];
 * dy: [n, 64, h - 2, w - 2]; d_x: [n, in_ch, h, w]; shape->filters and shape->eps are ignored; any h, w >= 3. */
size_t node_stem_conv0_dgrad_workspace_bytes(const node_stem_shape* shape);
int node_stem_conv0_dgrad(const node_stem_shape* shape, const float* w0, const float* dy, float* d_x,
                          void* ws, size_t ws_bytes, void* stream);

/* Diagnostics (tests): ONE convolution of the stem's kernel family on NCHW fp32 tensors, through the same layout /
 * split / MFMA kernels node_stem_fwd and node_stem_bwd use.  what: 0 forward y = conv2d(x, w, stride, pad);
 * 1 data gradient dx = conv_transpose of dy (x_h, x_w: the input's spatial size); 2 weight gradient dw.
 * x: [n, cin, x_h, x_w]; w / dw: [cout, cin, k, k]; y / dy: [n, cout, y_h, y_w]; cin, cout % 64 == 0.  Geometries:
 * k = 3 with pad 1 and k = 1 with pad 0, stride 1 or 2 (the residual stem's); k = 4 with stride 2 and pad 1 (the
 * down-sampling convolution of the `convolution` / `ode2` stems, node_downconv_* below; x_h, x_w >= 4) and no other k = 4. */
typedef struct node_conv_geom {
  int32_t n, cin, cout, x_h, x_w, k, stride, pad;
} node_conv_geom;
size_t node_stem_conv_workspace_bytes(const node_conv_geom* g);
int node_stem_conv(const node_conv_geom* g, int what, const float* x, const float* w, const float* dy, float* result,
                   void* ws, size_t ws_bytes, void* stream);

/* The residual trunk of the ResNet baseline -- model.py:79 (`features`): `blocks` x ResBlock(channels, channels), stride 1,
 * identity shortcut (model.py:284-310 with downsample = None).  Per block
 *     a = relu(norm1(x));  h = conv1(a);  y = conv2(relu(norm2(h))) + x
 * with norm = nn.GroupNorm(min(32, channels), channels) and both convolutions 3x3 / stride 1 / padding 1 without bias, on
 * the stem's kernels: gather GEMMs on the bf16 matrix pipe at fp32 accuracy (exact three-way bf16 splits, which keep
 * fp32's exponent range: no scale anywhere), the residual added in conv2's epilogue, NHWC inside the workspace.
 * x, out, grad_out, d_x: [n, channels, h, w] NCHW fp32.  taps (NULL: not wanted): [blocks][n, channels, h, w], every
 * block's output; the last one is `out` bit for bit.
 *   channels: a power of two in [64, 4096]; blocks >= 1; any n >= 1; h w <= 2400 pixels (the GroupNorm passes hold a
 *   (sample, channel block) in LDS); tensors under 2^31 elements.  Anything else: NODE_ERR_UNSUPPORTED with a message.
 * The backward needs the workspace exactly as the forward left it with keep_for_backward = 1 (one workspace per forward
 * in flight).  It writes (does not accumulate) every parameter gradient and the input gradient d_x (required: the stem
 * trains behind the trunk).  No floating-point atomics: every sum runs in a fixed order, so results are bit-reproducible
 * run to run.  The calls never synchronise, allocate device memory or read back.  The workspace-size call returns 0, with
 * a message behind node_last_error(), for a shape it refuses. */
typedef struct node_trunk_shape {
  int32_t n, channels, h, w, blocks;
  float eps;
} node_trunk_shape;
typedef struct node_trunk_block {        /* state_dict keys under `features.<i>.` */
  const float* n1_w;   /* norm1.weight [channels]                     */
  const float* n1_b;   /* norm1.bias   [channels]                     */
  const float* c1_w;   /* conv1.weight [channels, channels, 3, 3]     */
  const float* n2_w;   /* norm2.weight [channels]                     */
  const float* n2_b;   /* norm2.bias   [channels]                     */
  const float* c2_w;   /* conv2.weight [channels, channels, 3, 3]     */
} node_trunk_block;
typedef struct node_trunk_block_grads {  /* same order and shapes; device pointers, all required */
  float* n1_w; float* n1_b; float* c1_w; float* n2_w; float* n2_b; float* c2_w;
} node_trunk_block_grads;
size_t node_trunk_workspace_bytes(const node_trunk_shape* shape, int keep_for_backward);
int node_trunk_fwd(const node_trunk_shape* shape, const node_trunk_block* blocks, const float* x, float* out, float* taps,
                   int keep_for_backward, void* ws, size_t ws_bytes, void* stream);
int node_trunk_bwd(const node_trunk_shape* shape, const node_trunk_block* blocks, const float* grad_out,
                   const node_trunk_block_grads* grads, float* d_x, void* ws, size_t ws_bytes, void* stream);
/* Diagnostics (host only, needs no GPU): the geometry of the trunk's GroupNorm + ReLU launches (node_stem_gn_info above; one
 * record, every norm of the trunk has the same).  Returns what node_trunk_fwd would return for the shape, with `out` zeroed. */
int node_trunk_describe(const node_trunk_shape* shape, node_stem_gn_info* out);

/* The dynamics of an ODE block with norm = 'batch' -- model.py:326-348 with model.py:274:
 *     f(t, x) = norm3(conv2(t, relu(norm2(conv1(t, relu(norm1(x)))))))
 * norm = nn.BatchNorm2d(channels, track_running_stats=False): statistics of the BATCH (mean and biased variance per channel
 * over n h w values) in training and evaluation alike, affine, no running buffers; conv = ConcatConv2d (model.py:313-323): a
 * 3x3 / stride 1 / padding 1 convolution with bias over [t * 1, x], filter [channels, channels + 1, 3, 3], input channel 0 =
 * the time plane.  One evaluation and its vector-Jacobian product, on the stem's kernels: gather GEMMs on the bf16 matrix
 * pipe at fp32 accuracy for the x part of the filters, the time channel as the additive term t * (sum of the time taps inside
 * the image) that the BatchNorm passes add while they read the convolution's output, BatchNorm statistics in two stages
 * (centred second moments per chunk of rows, combined by Chan's formula in a fixed order).
 * t: a DEVICE scalar (the calls never read it on the host).  x, out, grad_out, d_x: [n, channels, h, w] NCHW fp32.
 *   channels: a multiple of 64 in [64, 4096] (192 is fine: BatchNorm has no groups); any n >= 1; h, w >= 3; tensors under
 *   2^31 elements.  Anything else: NODE_ERR_UNSUPPORTED with a message, and the workspace-size call returns 0.
 * The backward needs the workspace exactly as the forward left it with keep_for_backward = 1 (one workspace per forward in
 * flight).  It writes (does not accumulate) what is asked for: grads (NULL: no parameter gradient wanted; otherwise all
 * ten), d_x (NULL: not wanted), d_t (NULL: not wanted; a device scalar).  The gradient of a convolution's bias in front of a
 * BatchNorm is zero identically: conv1_b / conv2_b receive the computed sum, rounding noise around zero.  No floating-point
 * atomics: every sum runs in a fixed order, so results are bit-reproducible run to run.  The calls never synchronise,
 * allocate device memory or read back; NULL and misaligned arguments are rejected before any launch. */
typedef struct node_bnfunc_shape {
  int32_t n, channels, h, w;
  float eps;
} node_bnfunc_shape;
typedef struct node_bnfunc_params {      /* ODEfunc.named_parameters() order */
  const float* norm1_w; /* [C] */
  const float* norm1_b; /* [C] */
  const float* conv1_w; /* conv1._layer.weight [C, C + 1, 3, 3] */
  const float* conv1_b; /* conv1._layer.bias   [C] */
  const float* norm2_w;
  const float* norm2_b;
  const float* conv2_w;
  const float* conv2_b;
  const float* norm3_w;
  const float* norm3_b;
} node_bnfunc_params;
typedef struct node_bnfunc_grads {       /* same order and shapes; device pointers */
  float* norm1_w; float* norm1_b; float* conv1_w; float* conv1_b; float* norm2_w; float* norm2_b;
  float* conv2_w; float* conv2_b; float* norm3_w; float* norm3_b;
} node_bnfunc_grads;
size_t node_bnfunc_workspace_bytes(const node_bnfunc_shape* shape, int keep_for_backward);
int node_bnfunc_fwd(const node_bnfunc_shape* shape, const node_bnfunc_params* params, const float* t, const float* x, float* out,
                    int keep_for_backward, void* ws, size_t ws_bytes, void* stream);
int node_bnfunc_bwd(const node_bnfunc_shape* shape, const node_bnfunc_params* params, const float* t, const float* grad_out,
                    const node_bnfunc_grads* grads, float* d_x, float* d_t, void* ws, size_t ws_bytes, void* stream);
/* Diagnostics (tests; ABI 6): the launch plan node_bnfunc_fwd / _bwd and the node_bnsolve_* calls make for a shape, taken from the
 * plan itself.  Host only, no launch, needs no GPU.  Every BatchNorm pass runs nchunk chunks of chunk_rows rows (the last one
 * last_chunk_rows) by column_tiles blocks of 64 channels, a thread walking every 32nd row of its chunk; each of the two weight
 * gradients is split over wgrad_nsplit shares of wgrad_rows_per_split rows, which the backward's reduction launch sums.
 * Returns what the other calls return for a refused shape, NODE_ERR_NULL for a missing argument. */
typedef struct node_bnfunc_info {
  int32_t rows, chunk_rows, nchunk, last_chunk_rows, column_tiles, wgrad_nsplit, wgrad_rows_per_split;
} node_bnfunc_info;
int node_bnfunc_describe(const node_bnfunc_shape* shape, node_bnfunc_info* out);

/* The residual trunk of the ResNet baseline with norm = 'batch' -- model.py:79 with model.py:274: `blocks` x
 * ResBlock(channels, channels, norm='batch'), stride 1, identity shortcut.  Per block
 *     a = relu(norm1(x));  h = conv1(a);  y = conv2(relu(norm2(h))) + x
 * with norm = nn.BatchNorm2d(channels, track_running_stats=False) (statistics of the batch in training and evaluation alike)
 * and both convolutions 3x3 / stride 1 / padding 1 without bias.  The residual trunk above in every respect but the norm:
 * the same shape and block structures (parameter order n1_w, n1_b, c1_w, n2_w, n2_b, c2_w), NCHW at the boundary, optional
 * taps, keep_for_backward, one workspace per forward in flight; the BatchNorm passes are those of the batch-norm dynamics
 * (two-stage statistics combined by Chan's formula, fp64 backward partials), and the gradient of a block's input leaves its
 * norm1 backward pass with the shortcut's gradient already added.
 *   channels: a multiple of 64 in [64, 4096] (192 is fine); blocks >= 1; any n, h, w >= 1; tensors under 2^31 elements.
 *   Anything else: NODE_ERR_UNSUPPORTED with a message, and the workspace-size call returns 0.  Every tensor 16-byte aligned
 *   (NODE_ERR_ARG), the workspace 256-byte aligned.
 * The backward writes (does not accumulate) every parameter gradient and d_x (required).  No floating-point atomics: every
 * sum runs in a fixed order, so results are bit-reproducible run to run.  The calls never synchronise, allocate device memory
 * or read back.  The describe call is the one of the batch-norm dynamics for this plan (host only, needs no GPU). */
size_t node_bntrunk_workspace_bytes(const node_trunk_shape* shape, int keep_for_backward);
int node_bntrunk_fwd(const node_trunk_shape* shape, const node_trunk_block* blocks, const float* x, float* out, float* taps,
                     int keep_for_backward, void* ws, size_t ws_bytes, void* stream);
int node_bntrunk_bwd(const node_trunk_shape* shape, const node_trunk_block* blocks, const float* grad_out,
                     const node_trunk_block_grads* grads, float* d_x, void* ws, size_t ws_bytes, void* stream);
int node_bntrunk_describe(const node_trunk_shape* shape, node_bnfunc_info* out);

/* The residual stem with norm = 'batch' -- model.py:167-178 (`ResDownsample`) with model.py:274: the residual stem above in
 * every respect but the norm, nn.BatchNorm2d(C, track_running_stats=False) (statistics of the batch in training and evaluation
 * alike) in all four places.  The same shape structure, the same sixteen tensors in the same order (node_stem_params /
 * node_stem_grads), NCHW at the boundary; the launch plan is the GroupNorm stem's with the BatchNorm passes of the batch-norm
 * dynamics (two-stage statistics combined by Chan's formula, fp64 backward partials) in place of the GroupNorm passes.  The
 * last convolution stays on the gather GEMM (the F(4x4,3x3) route of the GroupNorm stem has GroupNorm inside its passes):
 * NODE_TUNE_STEM_W4 has no effect on this node.
 *   in_ch <= 3; h, w >= 5 and (h - 2)(w - 2) <= 2400 (the GroupNorm stem's image limit is kept: the first layer's kernels have
 *   not run above it); filters a multiple of 64 in [64, 4096] (192 and 384 are fine: BatchNorm has no groups); tensors under
 *   2^31 elements; n h2 w2 > 1 (nn.BatchNorm2d refuses one value per channel).  Anything else: NODE_ERR_UNSUPPORTED with a
 *   message, and the workspace-size call returns 0.  Every tensor 16-byte aligned (NODE_ERR_ARG), the workspace 256-byte aligned.
 * keep_for_backward = 0 is the no-grad forward: activations whose lives do not overlap share storage.  The backward needs the
 * workspace exactly as the forward left it with keep_for_backward = 1 (one workspace per forward in flight).  It writes (does
 * not accumulate) what is asked for: grads (NULL: frozen parameters -- only the data-gradient chain runs: no weight-gradient
 * and no slab-reduction launch), d_x [n, in_ch, h, w] (NULL: no image gradient -- the transposed first layer is left out); both
 * NULL: NODE_ERR_NULL.  d_x is the same bits with and without grads.  The gradient of conv0's bias in front of a BatchNorm is
 * zero identically: conv0_b receives the computed sum, rounding noise around zero.  No floating-point atomics: every sum runs
 * in a fixed order, so results are bit-reproducible run to run.  The calls never synchronise, allocate device memory or read
 * back; refused shapes, NULL and misaligned arguments and a short workspace are rejected before any launch.
 * The BatchNorm passes' chunks follow a policy of this node's own: at most NODE_TUNE_BNSTEM_MAXCHUNK chunks per 64-channel
 * tensor (read once per call; unset or 0: the built-in 128, the policy of the other batch-norm nodes).  It is part of the
 * workspace layout: a backward must run under the value its forward ran under.
 * The describe call (host only, needs no GPU) fills one node_bnfunc_info per norm, in the order of the tensors they normalise --
 * h0 (block 1 norm1), h1 (block 1 norm2), x1 (block 2 norm1), h3 (block 2 norm2): rows, chunks and column tiles of that tensor,
 * wgrad_nsplit / wgrad_rows_per_split of the convolution that reads the norm's output. */
size_t node_bnstem_workspace_bytes(const node_stem_shape* shape, int keep_for_backward);
int node_bnstem_describe(const node_stem_shape* shape, node_bnfunc_info out[4]);
int node_bnstem_fwd(const node_stem_shape* shape, const node_stem_params* params, const float* x, float* out,
                    int keep_for_backward, void* ws, size_t ws_bytes, void* stream);
int node_bnstem_bwd(const node_stem_shape* shape, const node_stem_params* params, const float* x, const float* grad_out,
                    const node_stem_grads* grads, float* d_x, void* ws, size_t ws_bytes, void* stream);

/* Classifier head of a norm = 'batch' net, up to (not including) the Linear layer -- model.py:231-250 with model.py:274:
 * BatchNorm2d(channels, track_running_stats=False) -> ReLU -> AdaptiveAvgPool2d((1,1)) -> [Dropout] -> Flatten:
 *     pooled[n, c] = scale[n, c] * mean over pixels of relu(gamma[c] * xhat + beta[c])
 * with xhat normalised by the mean and biased variance of channel c over all n h w values.  z, dz: [n, channels, h, w] NCHW;
 * gamma, beta, dgamma, dbeta: [channels]; scale: [n, channels] dropout mask / (1 - p) as the caller's RNG produced it, or NULL;
 * pooled, g_pooled: [n, channels]; stats: [2, channels] (mean, 1 / sqrt(var + eps)), kept by the caller for the backward;
 * scratch: node_bnhead_scratch_bytes bytes, 8-byte aligned, the statistics' partials of the call in flight (each call may be
 * given another).  Two launches each on `stream`.  Shapes: channels as above, tensors under 2^31 elements; NODE_ERR_UNSUPPORTED
 * otherwise (the scratch-size call returns 0).  Two-stage statistics with centred second moments, fp64 partials in the
 * backward, no atomics: the same bits on every run. */
size_t node_bnhead_scratch_bytes(const node_bnfunc_shape* shape);
int node_bnhead_fwd(const node_bnfunc_shape* shape, const float* z, const float* gamma, const float* beta, const float* scale,
                    float* pooled, float* stats, void* scratch, void* stream);
int node_bnhead_bwd(const node_bnfunc_shape* shape, const float* z, const float* gamma, const float* beta, const float* scale,
                    const float* stats, const float* g_pooled, float* dz, float* dgamma, float* dbeta, void* scratch, void* stream);

/* node_bnhead_fwd with the statistics PER SLICE (the reference normalises slice by slice): z [slices, n, c, h, w],
 * pooled [slices, n, c], stats [slices, 2, c]; two launches; every slice the bits of node_bnhead_fwd on it alone.  Forward only
 * (no dropout scale).  Shapes: those of node_bnhead_fwd for a slice, 1 <= slices <= 65535; scratch: 8-byte aligned,
 * node_bnhead_slices_scratch_bytes bytes (0 for a shape the entry refuses). */
size_t node_bnhead_slices_scratch_bytes(const node_bnfunc_shape* shape, int slices);
int node_bnhead_fwd_slices(const node_bnfunc_shape* shape, int slices, const float* z, const float* gamma, const float* beta,
                           float* pooled, float* stats, void* scratch, void* stream);

/* A whole SOLVE of these dynamics, forward and continuous adjoint: what the generic solver does around node_bnfunc_fwd / _bwd
 * (stage states, Hairer's initial step, error norms, accept / reject, dense output, FSAL: the node_flat_* kernels), driven from
 * inside the library.  The state stays in the BatchNorm kernels' NHWC layout from the first stage to the last (NCHW at the
 * boundary only: y0, y_out, y_traj, grad_out, grad_y0 are [.., n, channels, h, w]), the parameters are prepared once per solve,
 * and every evaluation writes tsign * f and tsign * vjp(-a) straight into the stage-derivative slots.
 *   method: NODE_METHOD_DOPRI5, or NODE_METHOD_RK4 (3/8 rule, one step per interval of t_pts, times rounded to fp32).
 *   t_pts: HOST array of n_t >= 2 times, strictly increasing or strictly decreasing (NODE_ERR_ARG otherwise).
 *   Shapes: those of node_bnfunc_fwd, and the n_t slices of a call together under 2^31 elements (n_t <= 1024); the workspace
 *   query returns 0 with a message for anything else.
 *   y_out: [n_t] slices, y_out[0] = y0 bit for bit.  y_traj: what node_bnsolve_fwd returned.  grad_out: [n_t] slices, or ONE
 *   slice (the last one's) with opts->grad_last_only.  grad_params: NULL (not wanted) or all ten; written, not accumulated.
 * The calls read the step controller back (they synchronise the stream) once per `steps_hint` / two steps until it reports the
 * interval done; the host takes no step decision.  Steps enqueued past the end of an interval run on discarded states, so no
 * result depends on the hint.  A controller status -- NODE_ERR_MAX_STEPS, NODE_ERR_NONFINITE, NODE_ERR_DT_UNDERFLOW -- is the
 * return code, with stats->status set.  stats->nfe counts what the generic solver leaves in func.nfe for the same step history:
 * forward 2 + 6 steps tried (rk4: 4 per interval); adjoint, per interval, one f(t_i, y_i) plus 2 + 6 steps tried (rk4: 4).
 * The caller owns every byte: the workspace holds the evaluation's plan, the flat segments (y, y1, a stage state and seven stage
 * derivatives each; y alone forward, y / adj_y / adj_params in the adjoint, adj_t in the controller), the NHWC slices and the
 * controller.  No floating-point atomics: the same bits on every run. */
typedef struct node_bnsolve_opts {
  int32_t max_num_steps;    /* <= 0: 2^31 - 1; steps tried per interval */
  int32_t steps_hint;       /* dopri5 steps enqueued before the first read-back (<= 0: 1); later rounds enqueue 2 */
  int32_t grad_last_only;   /* node_bnsolve_adjoint: as in node_solve_opts */
} node_bnsolve_opts;
size_t node_bnsolve_workspace_bytes(const node_bnfunc_shape* shape, int method, int adjoint, int n_t);   /* 0: refused, with a message */
int node_bnsolve_fwd(const node_bnfunc_shape* shape, const node_bnfunc_params* params, const float* y0, const float* t_pts, int n_t,
                     float rtol, float atol, int method, const node_bnsolve_opts* opts, float* y_out, node_stats* stats,
                     void* ws, size_t ws_bytes, void* stream);
int node_bnsolve_adjoint(const node_bnfunc_shape* shape, const node_bnfunc_params* params, const float* y_traj, const float* grad_out,
                         const float* t_pts, int n_t, float rtol, float atol, int method, const node_bnsolve_opts* opts,
                         float* grad_y0, const node_bnfunc_grads* grad_params, node_stats* stats, void* ws, size_t ws_bytes,
                         void* stream);

/* The hand-off between the two solves of the `ode2` stem -- model.py:199-223 (`ODEDownsample2`: `conv2(norm(x))`):
 *     y = conv(relu(norm(x))),   norm = nn.GroupNorm(min(32, cin), cin),   conv = nn.Conv2d(cin, cout, 4, 2, 1) with bias
 * on the stem's kernels: the GroupNorm + ReLU pass writes the exact bf16 triples the gather GEMM reads, the 16 taps of the
 * 4x4 filter are one K loop on the bf16 matrix pipe at fp32 accuracy, the bias is added in its epilogue; the data gradient
 * runs as four parity classes of four taps, the weight gradient one kernel row per workgroup.  NHWC inside the workspace.
 * x, d_x: [n, cin, h, w]; y, grad_y: [n, cout, oh, ow] with oh = (h + 2 - 4) / 2 + 1 (likewise ow), NCHW fp32.
 *   cin, cout: powers of two in [64, 4096]; any n >= 1; h, w >= 4 with h w pixels that fit the GroupNorm passes' LDS block
 *   (2400 at cin <= 256); tensors under 2^31 elements.  Anything else: NODE_ERR_UNSUPPORTED with a message; the
 *   workspace-size call returns 0 with the same message.
 * keep_for_backward = 0: the forward alone (a smaller workspace).  With 1 the backward needs the workspace exactly as the
 * forward left it.  node_downconv_bwd writes (does not accumulate) d_x (required) and, with grads given (NULL: the input
 * gradient only -- no weight-gradient and no reduction launch), all four parameter gradients.  No floating-point atomics:
 * every sum, the bias gradient's included, runs in a fixed order, so results are bit-reproducible run to run.  The calls
 * never synchronise, allocate device memory or read back. */
typedef struct node_downconv_shape {
  int32_t n, cin, cout, h, w;
  float eps;
} node_downconv_shape;
typedef struct node_downconv_params {    /* state_dict keys under `downsample.` of an `ode2` net */
  const float* gn_w;     /* norm.0.weight [cin]               */
  const float* gn_b;     /* norm.0.bias   [cin]               */
  const float* conv_w;   /* conv2.weight  [cout, cin, 4, 4]   */
  const float* conv_b;   /* conv2.bias    [cout]              */
} node_downconv_params;
typedef struct node_downconv_grads {     /* same order and shapes; device pointers, all required when given */
  float* gn_w; float* gn_b; float* conv_w; float* conv_b;
} node_downconv_grads;
size_t node_downconv_workspace_bytes(const node_downconv_shape* shape, int keep_for_backward);
int node_downconv_fwd(const node_downconv_shape* shape, const node_downconv_params* params, const float* x, float* y,
                      int keep_for_backward, void* ws, size_t ws_bytes, void* stream);
int node_downconv_bwd(const node_downconv_shape* shape, const node_downconv_params* params, const float* grad_y,
                      const node_downconv_grads* grads, float* d_x, void* ws, size_t ws_bytes, void* stream);

/* The `convolution` stem in front of the ODE block -- model.py:148-164 (`ConvDownsample`):
 *     Conv2d(in_ch, 64, 3, 1) | GroupNorm(32, 64) + ReLU | Conv2d(64, 64, 4, 2, 1) | GroupNorm(32, 64) + ReLU |
 *     Conv2d(64, filters, 4, 2, 1),  every convolution with bias
 * on the same kernels as the residual stem and the hand-off above; NHWC inside the workspace, no layout transposes between
 * the layers.  x: [n, in_ch, h, w]; out, grad_out: [n, filters, h2, w2] with h0 = h - 2, h1 = (h0 - 2) / 2 + 1,
 * h2 = (h1 - 2) / 2 + 1 (likewise w), NCHW fp32.
 *   in_ch <= 3; filters a power of two in [64, 4096]; h, w >= 10 and (h - 2)(w - 2) <= 2400 pixels (the GroupNorm passes hold
 *   a (sample, 8 channels) block in LDS); tensors under 2^31 elements.  Anything else: NODE_ERR_UNSUPPORTED with a message;
 *   the workspace-size call returns 0 with the same message.
 * node_convstem_bwd needs the workspace exactly as node_convstem_fwd left it with keep_for_backward = 1.  It writes (does not
 * accumulate) all ten parameter gradients; the image's gradient is not produced.  No floating-point atomics: every sum runs in
 * a fixed order.  The calls never synchronise, allocate device memory or read back. */
typedef struct node_convstem_shape {
  int32_t n, in_ch, h, w, filters;
  float eps;
} node_convstem_shape;
typedef struct node_convstem_params {    /* state_dict keys under `downsample.module.`, in state_dict order */
  const float* c0_w;     /* 0.weight [64, in_ch, 3, 3]     */
  const float* c0_b;     /* 0.bias   [64]                  */
  const float* n1_w;     /* 1.weight [64]                  */
  const float* n1_b;     /* 1.bias   [64]                  */
  const float* c1_w;     /* 3.weight [64, 64, 4, 4]        */
  const float* c1_b;     /* 3.bias   [64]                  */
  const float* n2_w;     /* 4.weight [64]                  */
  const float* n2_b;     /* 4.bias   [64]                  */
  const float* c2_w;     /* 6.weight [filters, 64, 4, 4]   */
  const float* c2_b;     /* 6.bias   [filters]             */
} node_convstem_params;
typedef struct node_convstem_grads {     /* same order and shapes; device pointers, all required */
  float* c0_w; float* c0_b; float* n1_w; float* n1_b; float* c1_w; float* c1_b; float* n2_w; float* n2_b; float* c2_w; float* c2_b;
} node_convstem_grads;
size_t node_convstem_workspace_bytes(const node_convstem_shape* shape, int keep_for_backward);
int node_convstem_fwd(const node_convstem_shape* shape, const node_convstem_params* params, const float* x, float* out,
                      int keep_for_backward, void* ws, size_t ws_bytes, void* stream);
int node_convstem_bwd(const node_convstem_shape* shape, const node_convstem_params* params, const float* x, const float* grad_out,
                      const node_convstem_grads* grads, void* ws, size_t ws_bytes, void* stream);
/* node_convstem_bwd plus the gradient of the image, d_x [n, in_ch, h, w] NCHW fp32 (required; written, not accumulated), with
 * the contract of node_stem_bwd_dx: the first layer is the residual stem's Conv2d(in_ch, 64, 3, 1), so the same transposed
 * first layer runs behind the data-gradient chain, in fp32 without atomics.  grads may be NULL (frozen parameters): then only
 * the data-gradient chain runs -- no weight-gradient, partial-sum or reduction launch.  With grads given, the parameter
 * gradients are node_convstem_bwd's bit for bit; d_x is the same bits with and without grads. */
int node_convstem_bwd_dx(const node_convstem_shape* shape, const node_convstem_params* params, const float* x, const float* grad_out,
                         const node_convstem_grads* grads, float* d_x, void* ws, size_t ws_bytes, void* stream);

/* The `convolution` stem with norm = 'batch' -- model.py:148-164 with model.py:274: the stem above in every respect but the
 * norm, nn.BatchNorm2d(64, track_running_stats=False) (statistics of the batch in training and evaluation alike) in both
 * places.  The same shape structure and the same ten tensors in the same order (node_convstem_params / node_convstem_grads,
 * n1_* / n2_* holding the BatchNorms' weight and bias), NCHW at the boundary; the launch plan is the GroupNorm stem's with the
 * BatchNorm passes of the batch-norm dynamics (two-stage statistics combined by Chan's formula, fp64 backward partials) in place
 * of the GroupNorm passes.
 *   in_ch <= 3; h, w >= 10 and (h - 2)(w - 2) <= 2400 (the GroupNorm stem's image limit is kept: the first layer's kernels have
 *   not run above it); filters a multiple of 64 in [64, 4096] (192 and 384 are fine: BatchNorm has no groups); tensors under
 *   2^31 elements.  Anything else: NODE_ERR_SHAPE / NODE_ERR_UNSUPPORTED with a message, and the workspace-size call returns 0.
 *   Every tensor 16-byte aligned (NODE_ERR_ARG), the workspace 256-byte aligned.
 * keep_for_backward = 0 is the no-grad forward: tensors whose lives do not overlap share storage.  The backward calls need the
 * workspace exactly as the forward left it with keep_for_backward = 1 (one workspace per forward in flight).  node_bnconvstem_bwd
 * writes (does not accumulate) all ten parameter gradients (grads required); node_bnconvstem_bwd_dx also the image's gradient
 * d_x [n, in_ch, h, w] (required), and with grads == NULL (frozen parameters) runs the data-gradient chain alone: no
 * weight-gradient, partial-sum or reduction launch.  d_x is the same bits with and without grads, the parameter gradients the
 * same bits from either call.  The biases of the first two convolutions stand in front of a BatchNorm, so their gradients are
 * zero identically: c0_b and c1_b receive the computed sums, rounding noise around zero.  No floating-point atomics: every
 * sum runs in a fixed order, so results are bit-reproducible run to run.  The calls never synchronise, allocate device memory
 * or read back; refused shapes, NULL and misaligned arguments and a short workspace are rejected before any launch.
 * The BatchNorm passes' chunks follow the batch-norm residual stem's policy (NODE_TUNE_BNSTEM_MAXCHUNK, part of the workspace
 * layout).  The describe call (host only, needs no GPU) fills one node_bnfunc_info per norm -- h0 (behind the first
 * convolution), h1 (behind the middle one): rows, chunks and column tiles of that tensor, wgrad_nsplit /
 * wgrad_rows_per_split of the convolution that reads the norm's output. */
size_t node_bnconvstem_workspace_bytes(const node_convstem_shape* shape, int keep_for_backward);
int node_bnconvstem_describe(const node_convstem_shape* shape, node_bnfunc_info out[2]);
int node_bnconvstem_fwd(const node_convstem_shape* shape, const node_convstem_params* params, const float* x, float* out,
                        int keep_for_backward, void* ws, size_t ws_bytes, void* stream);
int node_bnconvstem_bwd(const node_convstem_shape* shape, const node_convstem_params* params, const float* x, const float* grad_out,
                        const node_convstem_grads* grads, void* ws, size_t ws_bytes, void* stream);
int node_bnconvstem_bwd_dx(const node_convstem_shape* shape, const node_convstem_params* params, const float* x,
                           const float* grad_out, const node_convstem_grads* grads, float* d_x, void* ws, size_t ws_bytes,
                           void* stream);

/* The `ode2` stem's hand-off with norm = 'batch' -- model.py:199-223 with model.py:274:
 *     y = conv(relu(norm(x))),   norm = nn.BatchNorm2d(cin, track_running_stats=False),   conv = nn.Conv2d(cin, cout, 4, 2, 1) with bias
 * node_downconv_*'s plan with the BatchNorm passes; node_downconv_params / node_downconv_grads with gn_w / gn_b holding the
 * BatchNorm's weight and bias.  x, d_x: [n, cin, h, w]; y, grad_y: [n, cout, oh, ow], NCHW fp32.
 *   slices: 1, or T > 1: n = T * (n / T) samples are T slices of a trajectory [T, n / T, cin, h, w], each normalised with its own
 *   statistics (model.py:214-216 sends a trajectory through the norm slice by slice) -- one call instead of T, and every slice
 *   the bits of its own slices = 1 call.  Forward with keep_for_backward = 0 only: node_bndownconv_workspace_bytes(shape, 1)
 *   returns 0 with a message and node_bndownconv_fwd(.., keep_for_backward = 1, ..) / node_bndownconv_bwd return
 *   NODE_ERR_UNSUPPORTED for slices > 1 (feature extraction runs without gradients).
 *   cin, cout multiples of 64 in [64, 4096] (192 is fine); h, w >= 4 (no upper limit: the BatchNorm passes hold no image);
 *   slices >= 1 and n % slices == 0 (NODE_ERR_SHAPE); tensors under 2^31 elements.  Anything else: NODE_ERR_UNSUPPORTED with a
 *   message; the workspace-size call returns 0 with the same message.  Every tensor 16-byte aligned (NODE_ERR_ARG), the
 *   workspace 256-byte aligned.
 * node_bndownconv_bwd writes (does not accumulate) d_x (required) and, with grads given (NULL: the input gradient only -- no
 * weight-gradient and no reduction launch), all four parameter gradients.  No floating-point atomics; the same bits on every
 * run.  The calls never synchronise, allocate device memory or read back; everything refused is refused before any launch.
 * The describe call (host only, needs no GPU): rows = n h w, chunk_rows (what ONE slice's plan takes), nchunk = slices x chunks
 * per slice, last_chunk_rows = the last chunk's of every slice, column_tiles = cin / 64, the weight gradient's split. */
typedef struct node_bndownconv_shape {
  int32_t n, cin, cout, h, w, slices;
  float eps;
} node_bndownconv_shape;
size_t node_bndownconv_workspace_bytes(const node_bndownconv_shape* shape, int keep_for_backward);
int node_bndownconv_describe(const node_bndownconv_shape* shape, node_bnfunc_info* out);
int node_bndownconv_fwd(const node_bndownconv_shape* shape, const node_downconv_params* params, const float* x, float* y,
                        int keep_for_backward, void* ws, size_t ws_bytes, void* stream);
int node_bndownconv_bwd(const node_bndownconv_shape* shape, const node_downconv_params* params, const float* grad_y,
                        const node_downconv_grads* grads, float* d_x, void* ws, size_t ws_bytes, void* stream);

/* The `minimal` stem in front of the ODE block -- model.py:129-145 (`MinimalConvDownsample`):
 *     Conv2d(in_ch, 24, 3, 1) | GroupNorm(24, 24) + ReLU | Conv2d(24, 24, 4, 2, 1) | GroupNorm(24, 24) + ReLU |
 *     Conv2d(24, filters, 4, 2, 1),  every convolution with bias
 * on kernels of its own (csrc/kernels_ministem.hip): register-tiled fp32 convolutions on NHWC tensors of channel pitch 24,
 * GroupNorm with groups of ONE channel (statistics per (sample, channel) plane, one workgroup per sample).  Same geometry as
 * the `convolution` stem: x: [n, in_ch, h, w]; out, grad_out: [n, filters, h2, w2], NCHW fp32.
 *   in_ch <= 3; filters a power of two in [64, 4096]; h, w >= 10 (no upper limit on the image: no pass holds a plane in LDS);
 *   tensors under 2^31 elements.  Anything else: NODE_ERR_UNSUPPORTED with a message; the workspace-size call returns 0 with
 *   the same message.
 * node_ministem_bwd needs the workspace exactly as node_ministem_fwd left it with keep_for_backward = 1.  It writes (does not
 * accumulate) all ten parameter gradients (grads, nullable) and the image's gradient d_x [n, in_ch, h, w] (nullable).
 * grads == NULL (frozen parameters): the data-gradient chain alone, no weight-gradient and no reduction launch; d_x == NULL:
 * the transposed first layer is left out; both NULL: NODE_ERR_NULL.  The parameter gradients are the same bits with and
 * without d_x, and d_x is the same bits with and without grads.  With one channel per group the gradients of 0.bias and
 * 3.bias vanish in exact arithmetic; what is written is the rounding residue of the GroupNorm backward's own sums.  No
 * floating-point atomics: every sum runs in a fixed order.  The calls never synchronise, allocate device memory or read back. */
typedef struct node_ministem_shape {
  int32_t n, in_ch, h, w, filters;
  float eps;
} node_ministem_shape;
typedef struct node_ministem_params {    /* state_dict keys under `downsample.module.`, in state_dict order */
  const float* c0_w;     /* 0.weight [24, in_ch, 3, 3]     */
  const float* c0_b;     /* 0.bias   [24]                  */
  const float* n1_w;     /* 1.weight [24]                  */
  const float* n1_b;     /* 1.bias   [24]                  */
  const float* c1_w;     /* 3.weight [24, 24, 4, 4]        */
  const float* c1_b;     /* 3.bias   [24]                  */
  const float* n2_w;     /* 4.weight [24]                  */
  const float* n2_b;     /* 4.bias   [24]                  */
  const float* c2_w;     /* 6.weight [filters, 24, 4, 4]   */
  const float* c2_b;     /* 6.bias   [filters]             */
} node_ministem_params;
typedef struct node_ministem_grads {     /* same order and shapes; device pointers, all required when given */
  float* c0_w; float* c0_b; float* n1_w; float* n1_b; float* c1_w; float* c1_b; float* n2_w; float* n2_b; float* c2_w; float* c2_b;
} node_ministem_grads;
size_t node_ministem_workspace_bytes(const node_ministem_shape* shape, int keep_for_backward);
int node_ministem_fwd(const node_ministem_shape* shape, const node_ministem_params* params, const float* x, float* out,
                      int keep_for_backward, void* ws, size_t ws_bytes, void* stream);
int node_ministem_bwd(const node_ministem_shape* shape, const node_ministem_params* params, const float* x, const float* grad_out,
                      const node_ministem_grads* grads, float* d_x, void* ws, size_t ws_bytes, void* stream);

/* The `minimal` stem with norm = 'batch' -- model.py:129-145 with model.py:274: the stem above in every respect but the norm,
 * nn.BatchNorm2d(24, track_running_stats=False) (statistics of the batch in training and evaluation alike) in both places.  The
 * same shape structure, the same ten tensors in the same order (node_ministem_params / node_ministem_grads, n1_* / n2_* holding
 * the BatchNorms' weight and bias) and the same shapes taken and refused, with the same messages: in_ch <= 3; filters a power of
 * two in [64, 4096]; h, w >= 10 (no upper limit on the image); tensors under 2^31 elements.  The convolutions are the stem's
 * above, used as they are; the norms are BatchNorm + ReLU passes on the [rows = n h w][24] tensors (csrc/kernels_bnministem.hip)
 * with the conventions of the batch-norm dynamics: statistics in two stages (per chunk of rows the mean and the centred second
 * moment, combined by Chan's formula in one fixed order), the backward's sums in two stages with fp64 partials, the dx pass in
 * place on the activation's gradient.
 *   forward: 7 launches.  node_bnministem_bwd: 12 launches with grads and d_x; grads == NULL (frozen parameters): the
 *   data-gradient chain alone, 7 launches with d_x; d_x == NULL leaves the transposed first layer out; both NULL: NODE_ERR_NULL.
 * The backward needs the workspace exactly as the forward left it with keep_for_backward = 1 (one workspace per forward in
 * flight) and writes (does not accumulate) its results.  The parameter gradients are the same bits with and without d_x, d_x the
 * same bits with and without grads.  The biases of the first two convolutions stand in front of a BatchNorm, so their gradients
 * are zero identically: c0_b and c1_b receive the computed column sums of the dx passes, rounding noise around zero.  No
 * floating-point atomics: every sum runs in a fixed order, so results are bit-reproducible run to run.  The calls never
 * synchronise, allocate device memory or read back; refused shapes, NULL arguments, parameter or gradient tensors that are not
 * 16-byte aligned (NODE_ERR_ARG), a workspace that is not 256-byte aligned and a short workspace are rejected before any launch.
 * The describe call (host only, needs no GPU) fills one node_bnministem_info per norm -- h0 (behind the first convolution), h1
 * (behind the middle one): every BatchNorm pass runs nchunk workgroups (<= 128; NODE_TUNE_BNMINI_MAXCHUNK sets another cap, for measurements only, and with it
 * another workspace layout), one per chunk of chunk_rows rows (the last one
 * last_chunk_rows), each walking its chunk trip_rows rows at a time; wgrad_nsplit / wgrad_rows_per_split of the convolution that
 * reads the norm's output. */
typedef struct node_bnministem_info {
  int32_t rows, chunk_rows, nchunk, last_chunk_rows, trip_rows, wgrad_nsplit, wgrad_rows_per_split;
} node_bnministem_info;
size_t node_bnministem_workspace_bytes(const node_ministem_shape* shape, int keep_for_backward);
int node_bnministem_describe(const node_ministem_shape* shape, node_bnministem_info out[2]);
int node_bnministem_fwd(const node_ministem_shape* shape, const node_ministem_params* params, const float* x, float* out,
                        int keep_for_backward, void* ws, size_t ws_bytes, void* stream);
int node_bnministem_bwd(const node_ministem_shape* shape, const node_ministem_params* params, const float* x, const float* grad_out,
                        const node_ministem_grads* grads, float* d_x, void* ws, size_t ws_bytes, void* stream);

/* Retrieval evaluation -- `evaluate.py retrieval` of the reference (evaluate.py:308-361).  For every query i, with scores
 * s_i[j] = q[i] . x[j] and relevance gt_i[j] = (q_labels[i] == x_labels[j]):
 *   ap[i]   = sklearn average_precision_score(gt_i, s_i): descending scores, equal scores form ONE threshold; a row with no
 *             relevant item gives 0.0
 *   ap_k[i] = average_precision_score of the top min(k, nd) items (the reference's AP@k, evaluate.py:343-346): normalised by
 *             the relevant items inside the window, 0.0 when there are none.  Among equal scores the HIGHER database index
 *             ranks first (a stable ascending argsort reversed): that decides which items of a tie at the boundary enter.
 * -0.0 and +0.0 are one score.  q: [nq, d], x: [nd, d], scores: [nq, nd]  (fp32 row-major, device); labels int32 [nq] /
 * [nd]; ap, ap_k: fp64 [nq] (device).  nd <= 16384 (one row's sort keys in LDS), d >= 1, k >= 1.  Scores on the fp32
 * matrix pipe, one workgroup per query row for the ranking, sums in fp64 in a fixed order: bit-reproducible.
 * node_retrieval_workspace_bytes returns 0 (with a message) for a shape it refuses; node_rank_ap needs no workspace
 * (ws may be NULL). */
size_t node_retrieval_workspace_bytes(int nq, int nd, int d);
int node_retrieval_ap(int nq, int nd, int d, const float* q, const float* x, const int32_t* q_labels, const int32_t* x_labels,
                      int k, double* ap, double* ap_k, void* ws, size_t ws_bytes, void* stream);
int node_rank_ap(int nq, int nd, const float* scores, const int32_t* q_labels, const int32_t* x_labels, int k, double* ap,
                 double* ap_k, void* ws, size_t ws_bytes, void* stream);

/* Finetune evaluation -- `evaluate.py finetune` of the reference (evaluate.py:364-413): the linear SVMs behind
 * GridSearchCV(LinearSVC(), cv=5), as ONE batch of p problems over a shared x [n, d] (fp32 row-major, device).  Problem j is
 * the row (fold, cls, c) of `problems` (device): it trains on the rows i with row_fold[i] != fold (fold -1: all rows), with
 * targets +1 where labels[i] == cls and -1 elsewhere, and minimises, with x~ = [x, 1] (the bias is regularised),
 *     f(w) = 1/2 |w|^2 + c * sum_i max(0, 1 - y_i w . x~_i)^2                        (LinearSVC's defaults, one-vs-rest)
 * by a truncated Newton method (conjugate gradients on Hessian-vector products, backtracking line search) whose products
 * run on the fp32 matrix pipe for all problems at once; per-problem scalars are fp64, the state lives on the device.  A
 * problem stops when |grad f(w)| <= eps * max(min(#pos, #neg), 1) / #rows * |grad f(0)| (liblinear's rule) and is then
 * `converged`; after max_iter Newton iterations, or when no step length decreases f any more, it ends with converged = 0.
 * max_iter = 0 returns zero weights, converged = 0.  weights: [p, d + 1] (device; column d is the intercept); results: [p]
 * (device).  d <= 280.  Problems are solved in chunks when the workspace would pass 256 MiB.  node_svm_fit reads one word
 * per Newton iteration from the device and returns after the stream has drained.  Bit-reproducible: no atomics, fixed
 * summation orders, and a problem's result does not depend on its position in the table (within one chunk).
 * node_svm_workspace_bytes returns 0 (with a message) for a shape it refuses.
 *
 * node_svm_cv_score: group g is the k problems group_problems[g * k ...] (indices into `problems`, one per class in class
 * order; all of one fold).  For every row held out by that fold it predicts the class of the first maximum of w . x~ over the
 * group (k = 1: the problem's class iff w . x~ > 0, else neg_class) and counts: correct[g], held[g] (int32, device).  pred,
 * when not NULL, is int32 [n_groups, n]: the predicted class, -1 for rows that are not held out. */
typedef struct { int32_t fold; int32_t cls; float c; } node_svm_problem;
typedef struct { int32_t iterations; int32_t converged; double grad_ratio; } node_svm_result;
size_t node_svm_workspace_bytes(int n, int d, int p);
int node_svm_fit(int n, int d, int p, const float* x, const int32_t* labels, const int32_t* row_fold,
                 const node_svm_problem* problems, double eps, int max_iter, float* weights, node_svm_result* results, void* ws,
                 size_t ws_bytes, void* stream);
int node_svm_cv_score(int n, int d, int p, int n_groups, int k, const float* x, const int32_t* labels, const int32_t* row_fold,
                      const node_svm_problem* problems, const float* weights, const int32_t* group_problems, int neg_class,
                      int32_t* correct, int32_t* held, int32_t* pred, void* stream);

/* The input pipeline of the training loop -- the transform chains of utils.py:81-196 -- as ONE launch per batch on a split
 * that lives in device memory as uint8:
 *   out[b]        = Normalize(ToTensor(Flip(Jitter(Crop(Pad(data[index[b]]))))))      fp32  [batch, c, h, w]
 *   out_labels[b] = labels[index[b]]                                                  int64 [batch]
 * Every stage is switched by a bit of `flags`; with none set the launch is gather + / 255 (the test transform), with
 * NODE_AUG_NORM alone the normalising test transform.
 *   NODE_AUG_CROP    RandomCrop(size, padding), zero fill: output pixel (i, j) reads source pixel (i + dy - padding,
 *                    j + dx - padding), dy and dx uniform on {0 .. 2 padding}, or 0 outside the image
 *   NODE_AUG_JITTER  ColorJitter(saturation, hue), c == 3 only: fs uniform on [1 - saturation, 1 + saturation], fh uniform on
 *                    [-hue, hue], in the order a random bit picks; torchvision's tensor formulas in fp32 on [0, 1]
 *                    (adjust_saturation, adjust_hue), without requantisation to 8 bits between the two
 *   NODE_AUG_FLIP    RandomHorizontalFlip (p = 0.5)
 *   NODE_AUG_NORM    (x - mean[ch]) / std[ch]
 * Random numbers are Philox4x32-10 with key = `seed` (low word, high word) and counter = (dataset index, epoch, call, 0):
 * what an image looks like depends on (seed, epoch, index[b]) alone, not on the batch, the position in it or the rank.  Call 0
 * gives w0..w3: dy = (w0 (2 padding + 1)) >> 32, dx likewise from w1, flip = w2 >> 31, hue before saturation = w3 >> 31; call 1:
 * fs = (1 - saturation) + 2 saturation u(w0), fh = -hue + 2 hue u(w1) with u(w) = (w >> 8) 2^-24, in fp32.
 * data: uint8 [n, c, h, w]; labels: int64 [n]; index: int64 [batch], all device memory.  An index outside [0, n) reads
 * nothing: it gives a black image and the label -1.  No workspace, no synchronisation. */
enum { NODE_AUG_CROP = 1, NODE_AUG_JITTER = 2, NODE_AUG_FLIP = 4, NODE_AUG_NORM = 8 };
typedef struct node_augment {
  int32_t n, c, h, w;        /* the split; c is 1 or 3                                                              */
  int32_t padding;           /* NODE_AUG_CROP: 0 <= 2 padding + 1 <= 65536                                          */
  uint32_t flags;            /* NODE_AUG_* bits                                                                      */
  float saturation, hue;     /* NODE_AUG_JITTER: 0 <= saturation <= 1, 0 <= hue <= 0.5                              */
  float mean[3], std[3];     /* NODE_AUG_NORM: the first c entries, std > 0                                          */
} node_augment;
int node_augment_batch(const node_augment* aug, const uint8_t* data, const int64_t* labels, const int64_t* index, int batch,
                       uint64_t seed, uint32_t epoch, float* out, int64_t* out_labels, void* stream);

/* The transfer evaluations' test transform -- evaluate.py:38-50, `Resize(side)`, `ToTensor`, `Normalize` on a PIL image -- as
 * ONE launch per batch on a split that lives in device memory as uint8:
 *   out_u8[b]     = Resize(data[index[b]])                                            uint8 [batch, c, out_h, out_w]
 *   out_f32[b]    = Normalize(ToTensor(out_u8[b]))                                    fp32  [batch, c, out_h, out_w]
 *   out_labels[b] = labels[index[b]]                                                  int64 [batch]
 * Resize is PIL's `Image.resize((out_w, out_h), Image.BILINEAR)` on an 8-bit image, bit for bit.  Per axis, with `in` and
 * `out` the sizes along it: scale = in / out (double), filterscale = support = max(scale, 1); output position xx has
 * center = (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in) and the
 * weights w(x) = max(0, 1 - |(x - center + 0.5) / filterscale|) for x in [xmin, xmax), divided by their sum in double; the
 * fixed-point coefficient of a weight is int(w 2^22 + 0.5), and an output byte is clip(((1 << 21) + sum coeff pixel) >> 22, 0,
 * 255) in 32-bit integers.  The horizontal pass runs first, over every input row, and its result is rounded to bytes (they
 * stay on chip); the vertical pass runs on those bytes.  A pass whose size does not change is skipped: in == out on both
 * axes is the identity.  out_f32 is (byte / 255.f - mean[ch]) / std[ch] with `normalize`, byte / 255.f without: the
 * expressions of node_augment_batch's test transform, so the two agree bit for bit on the same bytes.  Integer arithmetic
 * and fixed orders throughout: every result is bit-reproducible.
 * data: uint8 [n, c, h, w]; labels: int64 [n]; index: int64 [batch], all device memory.  out_f32 or out_u8 may be NULL, not
 * both.  An index outside [0, n) reads nothing: a black image (normalised like any other) and the label -1.
 * Supported: c in (1, 3), every size >= 1, h out_w <= 65536 (the bytes between the passes), every tensor below 2^31 elements
 * and at most 2^24 coefficients per axis (NODE_ERR_UNSUPPORTED otherwise).  The coefficient tables are built on the host in
 * double and kept per (device, in, out): the FIRST call of a size pair on a device allocates and copies them (and so cannot
 * be captured into a graph); every later call only launches.  No workspace, no synchronisation.
 *
 * node_resize_table: host only, touches no device.  The table of one axis: xmin[out], count[out] (= xmax - xmin) and
 * coeff[out * ksize], row xx holding its count coefficients then zeros.  Returns out * ksize, the capacity (int32 entries of
 * coeff) it needs; xmin, count and coeff are written only when capacity is at least that (they may be NULL otherwise).  A
 * negative return is a NODE_ERR_* code.  ksize = 2 ceil(support) + 1. */
typedef struct node_resize {
  int32_t n, c, h, w;        /* the split; c is 1 or 3                                                              */
  int32_t out_h, out_w;
  int32_t normalize;         /* != 0: out_f32 = (x - mean[ch]) / std[ch]                                            */
  float mean[3], std[3];     /* normalize: the first c entries, std > 0                                             */
} node_resize;
int node_resize_batch(const node_resize* rs, const uint8_t* data, const int64_t* labels, const int64_t* index, int batch,
                      float* out_f32, uint8_t* out_u8, int64_t* out_labels, void* stream);
int node_resize_table(int in, int out, int32_t* xmin, int32_t* count, int32_t* coeff, int capacity);

/* The 4x4 stride-2 padding-1 convolution that turns the image into the ODE block's state -- the whole of the one-shot stem,
 * model.py:119-126 (`nn.Conv2d(in_ch, filters, 4, 2, 1)`), and the conv1 of the `ode` / `ode2` stems (model.py:185, 203):
 *     y = conv2d(x, weight, bias, stride 2, padding 1)
 * x: [n, in_ch, h, w] NCHW fp32 with 1 <= in_ch <= 4 and even h, w >= 4; weight: [filters, in_ch, 4, 4] with filters % 64 == 0;
 * bias: [filters] or NULL; y / grad_y: [n, filters, h / 2, w / 2] NCHW fp32, the layout the solver consumes.  Anything else is
 * refused with NODE_ERR_UNSUPPORTED.  All arithmetic is fp32 FMA (vector ALU), sums in a fixed order: no floating-point
 * atomics, every result is bit-reproducible run to run.
 *   node_imgconv_fwd  one launch.
 *   node_imgconv_bwd  d_weight[o][c][kh][kw] = sum_{n,oh,ow} grad_y[n][o][oh][ow] x[n][c][2 oh - 1 + kh][2 ow - 1 + kw] and
 *                     d_bias[o] = sum grad_y (NULL: not wanted) from ONE read of grad_y: per-slab partials in `ws`, summed in
 *                     slab order by a second small launch.  d_x (NULL: not wanted, nothing is launched for it) is one more
 *                     launch: each input pixel receives 2 x 2 taps x filters terms.  d_x must be 8-byte aligned.
 * Gradients are written, not accumulated.  The workspace carries nothing between calls (the forward needs none), but two calls
 * that may run at the same time (two streams) need a workspace each.  The calls never synchronise, allocate or read back.
 * node_imgconv_fwd is captured into graphs by graphs.capture_inference; a capture of node_imgconv_bwd has not been run and
 * is not claimed: imgconv.py keeps it out of captures.  filters <= 65536.  node_imgconv_workspace_bytes returns 0, with a
 * message behind node_last_error(), for a shape it refuses. */
typedef struct node_imgconv_shape {
  int32_t n, in_ch, h, w, filters;
} node_imgconv_shape;
size_t node_imgconv_workspace_bytes(const node_imgconv_shape* shape);
int node_imgconv_fwd(const node_imgconv_shape* shape, const float* x, const float* weight, const float* bias, float* y,
                     void* stream);
int node_imgconv_bwd(const node_imgconv_shape* shape, const float* x, const float* weight, const float* grad_y, float* d_weight,
                     float* d_bias, float* d_x, void* ws, size_t ws_bytes, void* stream);

/* The hand-off between the two solves of the `ode` stem -- model.py:181-196, `ODEDownsample.maxpool` = nn.MaxPool2d(4, 2, 1) --
 * and the plane means of the stem's trajectory in feature extraction (model.py:36, `fi.mean(-1).mean(-1)`).  fp32 NCHW.
 *
 * node_pool_fwd, ONE launch: x is a trajectory [t, n, c, h, w] (t = 1: a plain batch).
 *   pooled [n, c, oh, ow]  the max-pool of the LAST slice, oh = (h - 2) / 2 + 1, ow = (w - 2) / 2 + 1 (integer division).
 *                          ATen's semantics: padding counts as -inf; the window is scanned row-major with
 *                          `val > max || isnan(val)`, so ties go to the first tap and a NaN wins and propagates.
 *   argmax [n, c, oh, ow]  uint8 or NULL: the winning tap kh * 4 + kw (0..15) of input pixel (2 oh - 1 + kh, 2 ow - 1 + kw).
 *   means  [t, n, c]       or NULL: sum over the plane / (h w) of every slice; one fixed summation order.
 * node_pool_bwd, ONE launch: d_x [n, c, h, w] = the sum of grad_y [n, c, oh, ow] over the (at most 2 x 2) windows whose argmax
 *   names the pixel, in ascending (oh, ow) order.  Every element of d_x is written exactly once (no zero-fill, nothing
 *   accumulated, `t` is ignored); no atomics: bit-reproducible, and the bits of ATen's CPU backward.
 * Any t, n, c >= 1 and 2 <= h, w <= 32768 with at most 2^40 elements; anything else is refused with NODE_ERR_UNSUPPORTED and a
 * message.  Rows with w % 4 == 0 in 16-byte aligned tensors move as 16-byte accesses, everything else as scalars, with the
 * same results.  The calls need no workspace and never synchronise, allocate or read back. */
typedef struct node_pool_shape {
  int32_t t, n, c, h, w;
} node_pool_shape;
int node_pool_fwd(const node_pool_shape* shape, const float* x, float* pooled, uint8_t* argmax, float* means, void* stream);
int node_pool_bwd(const node_pool_shape* shape, const float* grad_y, const uint8_t* argmax, float* d_x, void* stream);

/* Event-based per-kernel-class timing (off by default; adds two event records
 * per profiled launch).  begin() resets the counters; end() synchronises the
 * recorded events and fills `out`. */
int node_profile_begin(void);
int node_profile_end(node_profile* out);

/* The basic-iterative (BIM / PGD) attack's per-iteration arithmetic -- adversarial/attack.py:72 (foolbox 2.x
 * LinfinityBasicIterativeAttack / L2BasicIterativeAttack with binary_search=False, no random start, untargeted,
 * Misclassification).  Images are [n, c, h, w] fp32 in pixel space [lo, hi]; s = hi - lo.  Two launches per iteration for the
 * whole batch, one workgroup per sample; neither synchronises, allocates or reads back.
 *
 * node_attack_step: for every sample with active[i] != 0, with g the gradient of the loss with respect to the NORMALISED
 * model input (x - mean) / std (the kernel divides it by std):
 *     L-infinity: x += stepsize * sign(g) * s;                      p = clip(x - x0, -epsilon s, epsilon s)
 *     L2:         x += stepsize * g / max(1e-12, rms(g)) * s;       p = (x - x0) * min(1, epsilon s / max(1e-12, rms(x - x0)))
 *     x = clip(x0 + p, lo, hi);   x_norm = (x - mean) / std         (rms: root MEAN square over the sample)
 * x is updated in place.  An inactive sample keeps x and x_norm bit for bit.  Any c h w.
 *
 * node_attack_judge: predicted class = arg-max of logits [n, classes] (first index on ties).  initial != 0: writes
 * original_class; a sample whose prediction differs from its label (a natural error) gets distance 0, adversarial_class =
 * the prediction, found_iteration 0 and active = 0.  Otherwise, for an active sample whose prediction differs from its
 * label: distance = mean((x - x0)^2) / s^2 (L2) or max |x - x0| / s (L-infinity); with return_early the record
 * (adversarial_class, found_iteration = iteration, distance, and best_x if given) is written and active cleared; without, the sample
 * stays active and the record and best_x (required) are replaced only by a strictly smaller distance.  The caller
 * initialises active = 1, adversarial_class = -1, found_iteration = -1, distance = +inf. */
#define NODE_ATTACK_LINF 0
#define NODE_ATTACK_L2 2
typedef struct node_attack {
  int32_t n, c, h, w;
  int32_t norm;              /* NODE_ATTACK_LINF or NODE_ATTACK_L2 */
  int32_t return_early;
  double stepsize, epsilon, lo, hi;
  const float* mean;         /* device [c], or NULL with std: no preprocessing */
  const float* std;
} node_attack;
typedef struct node_attack_record {    /* device pointers, one entry per sample */
  int32_t* active;
  int32_t* original_class;
  int32_t* adversarial_class;
  int32_t* found_iteration;
  float* distance;
  float* best_x;             /* [n, c, h, w]; nullable with return_early */
} node_attack_record;
int node_attack_step(const node_attack* attack, float* x, const float* x0, const float* g, const int32_t* active,
                     float* x_norm, void* stream);
int node_attack_judge(const node_attack* attack, int classes, const float* logits, const int64_t* labels, const float* x,
                      const float* x0, int initial, int iteration, const node_attack_record* record, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NODE_HIP_H */
