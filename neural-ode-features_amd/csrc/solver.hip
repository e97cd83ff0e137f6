// Member bodies of the solver context (solver.h): what a solve enqueues, in the order it enqueues it.
#include "solver.h"

#include <cmath>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

namespace node {

// the step-count guesses of this thread (solver.h, StepGuess)
static thread_local std::vector<StepGuess> g_guess;
int guess_steps(const StepGuess& k) {
  for (const auto& g : g_guess)
    if (g.N == k.N && g.C == k.C && g.H == k.H && g.W == k.W && g.aug == k.aug && g.forced == k.forced && g.rtol == k.rtol &&
        g.atol == k.atol && g.t0 == k.t0 && g.t1 == k.t1)
      return g.steps;
  return 1;
}
void remember_steps(const StepGuess& k) {
  for (auto& g : g_guess)
    if (g.N == k.N && g.C == k.C && g.H == k.H && g.W == k.W && g.aug == k.aug && g.forced == k.forced && g.rtol == k.rtol &&
        g.atol == k.atol && g.t0 == k.t0 && g.t1 == k.t1) { g.steps = k.steps; return; }
  if (g_guess.size() >= 64) g_guess.erase(g_guess.begin());
  g_guess.push_back(k);
}

const double DP_ALPHA[6] = {1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
const double DP_CMID[7] = {6025192743.0 / 30085553152.0 / 2.0, 0.0, 51252292925.0 / 65400821598.0 / 2.0,
                           -2691868925.0 / 45128329728.0 / 2.0, 187940372067.0 / 1594534317056.0 / 2.0,
                           -1776094331.0 / 19743644256.0 / 2.0, 11237099.0 / 235043384.0 / 2.0};
const double DP_BETA[6][6] = {
    {1.0 / 5, 0, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656, 0},
    {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84},
};

int g_w4_pair_stats[4] = {0, -1, 0, 0};
static thread_local Ctrl* g_blind_resident_ctrl = nullptr;   // pinned: where a DEFERRED resident solve leaves its record for this library itself --
                                                       // the caller reads the device record; a later call of this thread arms the cooldown from this one
std::atomic<int> g_resident_cooldown{0};

// ----------------------------------------------------------------------------
// Solver
// ----------------------------------------------------------------------------
void Solver::choose_resident(bool dopri5) {
  resident = dopri5 && tiny_mode() && !w4 && p.thand != nullptr && tiny_resident_ok(d);
  if (g_blind_resident_ctrl != nullptr && g_blind_resident_ctrl->status == NODE_ERR_HIP) {
    // an earlier DEFERRED resident solve of this thread ran into its deadline (nobody read its record on this side): same cooldown
    g_blind_resident_ctrl->status = 0;
    g_resident_cooldown.store(64, std::memory_order_relaxed);
  }
  if (resident) {      // a captured launch would replay its nonce: words of the previous replay would pass for this one's
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    if (cs != hipStreamCaptureStatusNone) resident = false;
  }
  // a grid that did not get the whole chip costs its 2 s deadline: after one, the next 64 solves of this process do not try
  if (resident && g_resident_cooldown.load(std::memory_order_relaxed) > 0) {
    g_resident_cooldown.fetch_sub(1, std::memory_order_relaxed);
    resident = false;
  }
}

int Solver::launch_resident(const float* y0, float* y_out, const StepIO& io, const double* ts, bool inline_targets, bool forced,
                            long long max_steps, int blind) {
  TinyResidentArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.y0 = y0; ra.y_first = y_out; ra.y_out = io.y_out;
  ra.w[0] = prm.conv1_w; ra.w[1] = prm.conv2_w;
  ra.bias[0] = prm.conv1_b; ra.bias[1] = prm.conv2_b;
  ra.gamma[0] = prm.norm1_w; ra.gamma[1] = prm.norm2_w; ra.gamma[2] = prm.norm3_w;
  ra.beta[0] = prm.norm1_b; ra.beta[1] = prm.norm2_b; ra.beta[2] = prm.norm3_b;
  if (blind && g_blind_resident_ctrl == nullptr) {
    if (hipHostMalloc((void**)&g_blind_resident_ctrl, sizeof(Ctrl), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); g_blind_resident_ctrl = nullptr; }
    else memset(g_blind_resident_ctrl, 0, sizeof(Ctrl));
  }
  ra.handoff = p.thand; ra.ctrl = p.ctrl; ra.ctrl_host = blind ? g_blind_resident_ctrl : hctrl;
  {
    // every word that crosses workgroups carries {nonce, version}: stale words of any earlier solve of this process never match, so
    // nothing is zeroed per solve.  The 28-bit nonce starts over every 2^28 solves: a hand-off buffer is zeroed the first time it
    // is used under a new generation of the counter (and the first time ever: whatever a fresh allocation holds is gone).
    // Three values are skipped: 0 (zeroed memory) and the two that, with the "solve is over" version, are the 0xFF / 0x7F byte patterns
    static std::mutex g_mu;
    static unsigned long long g_count = 0;
    static std::vector<std::pair<void*, unsigned long long>> g_seen;
    std::lock_guard<std::mutex> lock(g_mu);
    unsigned nn;
    do { nn = (unsigned)(++g_count & 0x0FFFFFFFull); } while (nn == 0u || nn == 0x0FFFFFFFu || nn == 0x07F7F7F7u);
    const unsigned long long gen = (g_count >> 28) + 1;
    bool seen = false, known = false;
    for (auto& e : g_seen) {
      if (e.first != p.thand) continue;
      known = e.second == gen;
      e.second = gen;
      seen = true;
      break;
    }
    if (!seen) {
      if (g_seen.size() >= 256) g_seen.erase(g_seen.begin());
      g_seen.emplace_back(p.thand, gen);
    }
    if (!known) HIP_TRY(hipMemsetAsync(p.thand, 0, tiny_resident_handoff_words(d) * 8, st));
    ra.nonce = nn;
  }
  ra.targets = inline_targets ? nullptr : p.targets; ra.n_targets = io.n_targets;
  if (inline_targets) for (int j = 0; j < io.n_targets; ++j) ra.targets_inline[j] = ts[j + 1];
  ra.forced = forced ? p.forced : nullptr; ra.n_forced = io.n_forced;
  ra.dt_log = io.log_cap > 0 ? p.dtlog : nullptr; ra.dt_log_cap = io.log_cap;
  ra.t0 = ts[0]; ra.max_steps = max_steps;
  ra.rtol = rtol; ra.atol = atol; ra.tsign = tsign;
  if (!blind) { hctrl->done = 0; hctrl->status = NODE_ERR_HIP; }      // (overwritten by the launch: if it never ran, the record says so)
  launch_tiny_solve(d, ra, st);
  nfe = forced ? 1 : 2;
  return NODE_OK;
}

void Solver::take_norm_hook(const node_solve_opts* o) {
  if (o != nullptr && o->norm_reduce != nullptr && o->norm_buf != nullptr && o->norm_world >= 1) {
    nr_fn = o->norm_reduce; nr_ctx = o->norm_reduce_ctx; nr_buf = o->norm_buf; nr_world = (float)o->norm_world;
  }
}

void Solver::norm_exchange(int mode, int nseg) {
  NormPackArgs np;
  memset(&np, 0, sizeof(np));
  np.ctrl = p.ctrl; np.partial[0] = p.partial[0]; np.partial[1] = p.partial[1]; np.partial[2] = p.partial[2];
  np.nseg = nseg; np.has_scalar = aug ? 1 : 0; np.mode = mode; np.rtol = rtol; np.atol = atol;
  np.w4sc = (aug && w4_f16) ? p.w4sc : nullptr; np.gbuf = nr_buf;
  launch_norm_pack(np, st);
  nr_fn(nr_ctx, nr_buf, 8, (void*)st);
}

int Solver::check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
  return NODE_OK;
}

int Solver::prepare(const SolveSetup* setup) {
  auto pack = d.wino == 2 ? launch_pack_weights_w2 : d.wino ? launch_pack_weights_w : launch_pack_weights;
  // zero fills of the solve, folded into the preparation launch below: the stage-2 parameter derivative (read with
  // weight zero by the error norm / dense output, never written by dopri5 steps -- the initial-step probe does
  // write it -- so it must hold finite values), the arrival counter of k_theta_finalize, and the zero rows behind
  // the conv inputs (see make_plan)
  float* zr[12];
  size_t zn[12];
  int nz = 0;
  if (aug) {
    zr[nz] = p.KT[1]; zn[nz++] = d.P;
    zr[nz] = p.sred + (size_t)2 * 9 * d.C + 2 * ((9 * (size_t)d.C + 63) / 64); zn[nz++] = 1;
  }
  if (d.wino == 2 || d.wgrad_wino == 2 || small_mode()) {
    zr[nz] = p.act1 + d.numel; zn[nz++] = d.C;
    zr[nz] = p.act2 + d.numel; zn[nz++] = d.C;
    if (aug) {
      zr[nz] = p.dz1 + d.numel; zn[nz++] = d.C;
      zr[nz] = p.dz2 + d.numel; zn[nz++] = d.C;
      if (p.act1b) { zr[nz] = p.act1b + d.numel; zn[nz++] = d.C; }
    }
  }
  if (small_mode()) {
    launch_pack_weights_small(d, prm.conv1_w, p.wsmall[0], st);
    launch_pack_weights_small(d, prm.conv2_w, p.wsmall[1], st);
  }
  if (tiny_mode() && !w4) {
    launch_tiny_pack(d, prm.conv1_w, p.wtiny[0], st);
    launch_tiny_pack(d, prm.conv2_w, p.wtiny[1], st);
    launch_fill(reinterpret_cast<float*>(p.tcount), 0.f, (size_t)d.N * d.G, st);     // (0.f is the all-zero word)
  }
  if (w4) {
    w4_b16 = w4_uses_bf16(d.N8, d.C);
    w4_f16 = w4_b16 && w4_f16_fits(d.N8, d.C) && (!aug || (w4_f16_aug && w4_wgrad_on() && w4_wgrad_f16_fits(d.N8, d.C)));
    g_ready = false;
    if (w4_f16) { zr[nz] = reinterpret_cast<float*>(p.w4sc); zn[nz++] = sizeof(W4Scales) / sizeof(float); }
  }
  if (setup != nullptr && setup->zero != nullptr) {
    if (nz >= 12) return fail(NODE_ERR_ARG, "prepare(): more zero fills than the preparation launch carries");
    zr[nz] = setup->zero; zn[nz++] = setup->zero_n;
  }
  // (first: it carries the solve's zero fills, among them the scratch words of k_w4_scales)
  launch_time_prep(d, prm.conv1_w, prm.conv2_w, p.tmap[0], p.tmap[1], aug ? p.wtime[0] : nullptr, aug ? p.wtime[1] : nullptr, zr, zn,
                   nz, st, w4 ? p.tmapS[0] : nullptr, w4 ? p.tmapS[1] : nullptr, d.w4q, setup);
  if (w4) {
    W4PackJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    const float* ws_[4] = {prm.conv1_w, prm.conv2_w, prm.conv1_w, prm.conv2_w};
    if (w4_f16) {       // the scales of the fp16-pair operands: filters from max|w|, forward row operands from the GroupNorm in front
      W4ScaleJobs sj;
      memset(&sj, 0, sizeof(sj));
      sj.w[0] = prm.conv1_w; sj.w[1] = prm.conv2_w; sj.wn = (size_t)d.C * (d.C + 1) * 9;
      sj.gb[0] = prm.norm1_w; sj.gb[1] = prm.norm1_b; sj.gb[2] = prm.norm2_w; sj.gb[3] = prm.norm2_b;
      sj.C = d.C; sj.gn_m = d.cpg * d.HW; sj.sc = p.w4sc;
      launch_w4_scales(sj, st);
    }
    for (int i = 0; i < (aug ? 4 : 2); ++i) {
      jobs.w[i] = ws_[i]; jobs.u[i] = p.w4u[i]; jobs.dgrad[i] = i >= 2;
      if (w4_f16) { jobs.uh[i] = reinterpret_cast<unsigned*>(p.w4u[i]); jobs.uh_exp[i] = &p.w4sc->e[(i & 1) ? W4_E_U2 : W4_E_U1]; }
      if (!w4_f16 || aug) jobs.ub[i] = w4_b16 ? p.w4ub[i] : nullptr;
    }
    launch_w4_pack(jobs, aug ? 4 : 2, d.C, st);
  } else if (d.wino == 2) {   // every packing of the solve in one launch
    const float* ws_[4] = {prm.conv1_w, prm.conv2_w, prm.conv1_w, prm.conv2_w};
    float* dst_[4] = {p.wf[0], p.wf[1], p.wd[0], p.wd[1]};
    const int dg_[4] = {0, 0, 1, 1};
    launch_pack_weights_w2_multi(d, ws_, dst_, dg_, aug ? 4 : 2, st);
  } else {
    pack(d, prm.conv1_w, p.wf[0], 0, st);
    pack(d, prm.conv2_w, p.wf[1], 0, st);
    if (aug) {
      pack(d, prm.conv1_w, p.wd[0], 1, st);
      pack(d, prm.conv2_w, p.wd[1], 1, st);
    }
  }
  if (w4 && aug && d.N * d.w4q != d.N8 && p.W4dU != nullptr) {
    // the weight gradient SUMS over the GEMM rows: the rows of the padding samples (never written by a pass) must be zero
    for (int i = 0; i < 2; ++i) {
      launch_fill(p.W4Va[i], 0.f, w4_v_elems(d.N8, d.C), st);
      launch_fill(p.W4Z[i], 0.f, w4_z_elems(d.N8, d.C), st);
    }
    launch_fill(p.W4Va0b, 0.f, w4_v_elems(d.N8, d.C), st);
  }
  v_ready = false;
  cur = 0;
  theta_rider = env_int("NODE_TUNE_THETA_RIDER", 1) != 0;     // (read per solve: tests switch it inside one process)
  tf_waiting = false;
  return check_launch("prepare");
}

void Solver::gn_pass_fwd(const float* gamma, const float* beta, int relu, float osign, float* out, float* xhat_out, float* rstd_out) {
  CombineGnArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.comb.y = p.RAW; ca.comb.nk = 0; ca.comb.scale_mode = SC_ABS; ca.ctrl = p.ctrl;
  ca.act_out = out; ca.xhat_out = xhat_out; ca.rstd_out = rstd_out;
  ca.gamma = gamma; ca.beta = beta; ca.relu = relu; ca.osign = osign;
  launch_combine_gn(d, ca, st);
}
void Solver::gn_pass_bwd(const float* act, const float* xhat, const float* rstd, const float* gamma, float osign, float* out,
                 float* gpart, float* spart) {
  GnBwdArgs g;
  memset(&g, 0, sizeof(g));
  g.comb.y = p.RAW; g.comb.nk = 0; g.comb.scale_mode = SC_ABS; g.ctrl = p.ctrl; g.csign = 1.f;
  g.xhat = xhat; g.rstd = rstd; g.gamma = gamma; g.dz_out = out; g.gpart = gpart; g.spart = spart;
  g.mask_act = act; g.osign = osign;
  launch_gn_bwd(d, g, st);
}

void Solver::w4_gemm(int which, const float* V) {
  ProfScope ps(2, conv_flops(), st);
  if (f16_now()) {     // which: 0 / 1 forward conv1 / conv2, 2 / 3 their data gradients (row operand = a cotangent)
    launch_w4_gemm_f16(reinterpret_cast<const unsigned*>(V ? V : p.W4V), reinterpret_cast<const unsigned*>(p.w4u[which]), p.W4M, p.ctrl, d.N8, d.C,
                       &p.w4sc->e[which >= 2 ? W4_E_G : which ? W4_E_V2 : W4_E_V1], &p.w4sc->e[(which & 1) ? W4_E_U2 : W4_E_U1], st);
    return;
  }
  launch_w4_gemm(V ? V : p.W4V, p.w4u[which], p.W4M, p.ctrl, d.N8, d.C, st, w4_b16 ? p.w4ub[which] : nullptr);
}

W4sArgs Solver::w4_args() const {
  W4sArgs a;
  memset(&a, 0, sizeof(a));
  a.ctrl = p.ctrl; a.N = d.N; a.Q = d.w4q; a.Nv = d.N8; a.C = d.C; a.cpg = d.cpg; a.eps = d.eps;
  return a;
}

void Solver::w4_tail_combine(W4sArgs& a, const Comb& cy, float* y_out, bool train, int set, int self) {
  a.t.comb = cy; a.t.self = self; a.t.y_out = y_out; a.t.gamma = prm.norm1_w; a.t.beta = prm.norm1_b;
  if (train) { a.t.act_nhwc = w4_wgrad_on() ? nullptr : act1_of(set); a.t.xhat_s = xh1_of(set); a.t.rstd = r1_of(set); }
  a.V = (train && w4_wgrad_on()) ? va0_of(set) : p.W4V;
  if (f16_now()) a.v_exp = &p.w4sc->e[W4_E_V1];
}

void Solver::w4_pass(int head, int tail, const W4sArgs& a, const ThetaFinalizeArgs* rider) {
  double bytes = 0.0;
  if (g_prof.on) {
    const double state = (double)d.numel * sizeof(float), comp = 36.0 * 4.0 * d.N * d.w4q * d.C * sizeof(float);
    int tensors = 0;
    if (head) {
      tensors += (a.h.out_s != nullptr) + (a.h.out_nhwc != nullptr);
      tensors += a.h.xhat_s != nullptr;      // written (forward) or read (backward)
      bytes += comp;
    }
    if (tail) {
      tensors += 1 + a.t.comb.nk - (a.t.self ? 1 : 0);
      tensors += (a.t.y_out != nullptr) + (a.t.act_nhwc != nullptr) + (a.t.xhat_s != nullptr);
    }
    if (a.V) bytes += comp;
    bytes += tensors * state;
    if (rider != nullptr) {     // what the finalize reads (weight-gradient partials, GroupNorm / masked-sum partials) and writes (theta)
      const double cc = (double)d.C * d.C * sizeof(float), rows = (double)d.N * d.w4q;
      bytes += (rider->dU != nullptr ? 2.0 * W4_COMPS : 2.0 * 9.0 * d.nsplit) * cc;
      bytes += rows * (3.0 * 2.0 + 2.0 * 9.0) * d.C * sizeof(float) + (double)d.P * sizeof(float);
    }
  }
  const int cls = head == 0 ? 3 : head == 1 ? 4 + tail : 7 + tail;
  ProfScope ps(cls, bytes, st);
  if (rider != nullptr) launch_w4s_p2_rider(a, *rider, d, st);
  else launch_w4s_pass(head, tail, a, st);
}

int Solver::eval_w4(const Comb& cy, float* y_out, const EvalTime& et, float* kY_out, bool train, const Comb* ca, float* a_out,
            float* kA_out, float* kT_out, int kidx, float csign, float* vjp_t_out, bool need_theta, const NextComb* next) {
  const bool do_aug = ca != nullptr;
  if (next != nullptr)   // a combine that reads this evaluation's own derivative anywhere but as its last term cannot merge
    for (int j = 0; j + 1 < next->cy.nk; ++j)
      if (next->cy.k[j] == kY_out || (do_aug && next->cy.k[j] == kA_out)) next = nullptr;
  if (!v_ready) {
    W4sArgs a = w4_args();
    w4_tail_combine(a, cy, y_out, train, cur, 0);
    w4_pass(0, 1, a);
  }
  v_ready = false;
  const bool wg4 = do_aug && w4_wgrad_on();
  w4_gemm(0, wg4 ? va0_of(cur) : nullptr);
  {   // P2
    W4sArgs a = w4_args();
    a.h.M = p.W4M; a.h.bias = prm.conv1_b; a.h.tmapS = p.tmapS[0]; a.h.et = et; a.h.gamma = prm.norm2_w; a.h.beta = prm.norm2_b;
    a.h.osign = 1.f; a.h.relu = 1;
    if (train) { a.h.out_nhwc = wg4 ? nullptr : p.act2; a.h.xhat_s = p.xh2; a.h.rstd = p.r2; }
    a.V = wg4 ? p.W4Va[1] : p.W4V;
    if (f16_now()) a.v_exp = &p.w4sc->e[W4_E_V2];
    w4_pass(1, 0, a, tf_waiting ? &tf_wait : nullptr);     // (with the finalize of the evaluation in front, if it waits: solver.h)
    tf_waiting = false;
  }
  w4_gemm(1, wg4 ? p.W4Va[1] : nullptr);
  W4sArgs a3 = w4_args();
  a3.h.M = p.W4M; a3.h.bias = prm.conv2_b; a3.h.tmapS = p.tmapS[1]; a3.h.et = et; a3.h.gamma = prm.norm3_w; a3.h.beta = prm.norm3_b;
  a3.h.osign = et.tsign; a3.h.relu = 0; a3.h.out_s = kY_out;
  if (!do_aug) {
    if (next != nullptr) {   // P3C
      const int self = next->cy.nk > 0 && next->cy.k[next->cy.nk - 1] == kY_out;
      w4_tail_combine(a3, next->cy, next->y_out, false, cur, self);
      w4_pass(1, 1, a3);
      v_ready = true;
    } else {
      w4_pass(1, 0, a3);
    }
    if (count_nfe) nfe += 1;
    return check_launch("odefunc forward (F(4x4,3x3))");
  }
  // P3B3: GroupNorm-3, then the adjoint combine through its backward
  a3.t.comb = *ca; a3.t.csign = csign; a3.t.y_out = a_out; a3.t.gpart = p.gpart[2]; a3.t.spart = p.spart[1];
  if (wg4) a3.t.z_out = need_theta ? p.W4Z[1] : nullptr;
  else a3.t.act_nhwc = p.dz2;
  a3.V = p.W4V;
  if (w4_f16) a3.gstat = p.w4sc;
  if (f16_now()) { a3.v_exp = &p.w4sc->e[W4_E_G]; a3.z_exp = &p.w4sc->e[W4_E_G]; }
  w4_pass(1, 2, a3);
  if (count_nfe) nfe += 1;
  w4_gemm(3);   // data gradient of conv2
  {   // PB2
    W4sArgs a = w4_args();
    a.h.M = p.W4M; a.h.gamma = prm.norm2_w; a.h.beta = prm.norm2_b; a.h.xhat_s = p.xh2; a.h.rstd = p.r2; a.h.osign = 1.f;
    a.h.gpart = p.gpart[1]; a.h.spart = p.spart[0];
    if (wg4) a.h.z_out = need_theta ? p.W4Z[0] : nullptr;
    else a.h.out_nhwc = p.dz1;
    a.V = p.W4V;
    if (w4_f16) a.gstat = p.w4sc;
    if (f16_now()) { a.v_exp = &p.w4sc->e[W4_E_G]; a.z_exp = &p.w4sc->e[W4_E_G]; }
    w4_pass(2, 0, a);
  }
  // the weight gradient and the conv-1 data gradient's GEMM are independent (solver.h): one launch where the batch has the kernel
  const bool paired = need_theta && wg4 && f16_now() && w4_pair_fits(d.N8, d.C);
  if (paired) {
    // profile class 1 with the FLOPs of both halves: the GEMM's share is not in class 2 ("paired launch")
    ProfScope ps(1, 3.0 * conv_flops(), st);
    launch_w4_gemm_wgrad_f16(reinterpret_cast<const unsigned*>(p.W4V), reinterpret_cast<const unsigned*>(p.w4u[2]), p.W4M, &p.w4sc->e[W4_E_G],
                             &p.w4sc->e[W4_E_U1], reinterpret_cast<const unsigned*>(va0_of(cur)), reinterpret_cast<const unsigned*>(p.W4Z[0]),
                             reinterpret_cast<const unsigned*>(p.W4Va[1]), reinterpret_cast<const unsigned*>(p.W4Z[1]), p.W4dU, p.ctrl, d.N8, d.C,
                             &p.w4sc->e[W4_E_V1], &p.w4sc->e[W4_E_V2], &p.w4sc->e[W4_E_G], st);
  } else if (need_theta && wg4 && f16_now()) {
    ProfScope ps(1, 2.0 * conv_flops(), st);
    launch_w4_wgrad_f16(reinterpret_cast<const unsigned*>(va0_of(cur)), reinterpret_cast<const unsigned*>(p.W4Z[0]), reinterpret_cast<const unsigned*>(p.W4Va[1]),
                        reinterpret_cast<const unsigned*>(p.W4Z[1]), p.W4dU, p.ctrl, d.N8, d.C, &p.w4sc->e[W4_E_V1], &p.w4sc->e[W4_E_V2], &p.w4sc->e[W4_E_G], st);
  } else if (need_theta && wg4) {
    W4WgradArgs wa;
    memset(&wa, 0, sizeof(wa));
    wa.V1 = va0_of(cur); wa.Z1 = p.W4Z[0]; wa.V2 = p.W4Va[1]; wa.Z2 = p.W4Z[1]; wa.dU = p.W4dU; wa.ctrl = p.ctrl; wa.N = d.N8; wa.C = d.C;
    ProfScope ps(1, 2.0 * conv_flops(), st);
    launch_w4_wgrad(wa, st);
  } else if (need_theta) {
    WgradArgs w1;
    memset(&w1, 0, sizeof(w1));
    w1.act = act1_of(cur); w1.dz = p.dz1; w1.wpart = p.wpart[0]; w1.ctrl = p.ctrl;
    if (d.wgrad_pair) { w1.act2 = p.act2; w1.dz2 = p.dz2; w1.wpart2 = p.wpart[1]; }
    { ProfScope ps(1, (d.wgrad_pair ? 2.0 : 1.0) * conv_flops(), st); launch_wgrad(d, w1, st); }
    if (!d.wgrad_pair) {
      WgradArgs w2 = w1;
      w2.act = p.act2; w2.dz = p.dz2; w2.wpart = p.wpart[1];
      { ProfScope ps(1, conv_flops(), st); launch_wgrad(d, w2, st); }
    }
  }
  if (!paired) w4_gemm(2);   // data gradient of conv1
  {   // PB1 (+ the next evaluation's combine)
    W4sArgs a = w4_args();
    a.h.M = p.W4M; a.h.gamma = prm.norm1_w; a.h.beta = prm.norm1_b; a.h.xhat_s = xh1_of(cur); a.h.rstd = r1_of(cur);
    a.h.osign = et.tsign; a.h.out_s = kA_out; a.h.gpart = p.gpart[0];
    if (next != nullptr) {
      w4_tail_combine(a, next->cy, next->y_out, true, cur ^ 1, 0);
      w4_pass(2, 1, a);
      cur ^= 1;
      v_ready = true;
    } else {
      w4_pass(2, 0, a);
    }
  }
  if (!need_theta) return check_launch("augmented dynamics (F(4x4,3x3))");
  ThetaFinalizeArgs tf;
  memset(&tf, 0, sizeof(tf));
  tf.dU = wg4 ? p.W4dU : nullptr;
  tf.wpart[0] = p.wpart[0]; tf.wpart[1] = p.wpart[1];
  tf.spart[0] = p.spart[0]; tf.spart[1] = p.spart[1];
  tf.gpart[0] = p.gpart[0]; tf.gpart[1] = p.gpart[1]; tf.gpart[2] = p.gpart[2];
  tf.gpart_rows[0] = tf.gpart_rows[1] = tf.gpart_rows[2] = tf.spart_rows = d.N * d.w4q;   // per-sample (per-quadrant) partials from the GroupNorm passes
  tf.wtime[0] = p.wtime[0]; tf.wtime[1] = p.wtime[1]; tf.sred = p.sred;
  tf.et = et; tf.osign = et.tsign; tf.theta_out = kT_out;
  tf.ctrl = p.ctrl; tf.kidx = kidx; tf.write_scalar = kidx >= 0 ? 1 : 0; tf.vjp_t_out = vjp_t_out;
  if (theta_rider && next != nullptr && w4s_rider_fits(d.cpg, d.w4q)) {   // another evaluation of this step follows: its P2 launch carries it
    tf_wait = tf;
    tf_waiting = true;
  } else {
    launch_theta_finalize(d, tf, st);
  }
  return check_launch("augmented dynamics (F(4x4,3x3))");
}

int Solver::eval_fwd(const Comb& cy, float* y_out, const EvalTime& et, float* k_out, bool train, const NextComb* next) {
  if (w4) return eval_w4(cy, y_out, et, k_out, train, nullptr, nullptr, nullptr, nullptr, -1, 0.f, nullptr, false, next);
  const bool tiny = tiny_mode() && !train;
  if (!(tiny && v_ready)) {      // (latency path: the previous evaluation's last launch may have formed this conv input already)
    CombineGnArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.comb = cy; ca.ctrl = p.ctrl; ca.y_out = y_out; ca.act_out = p.act1;
    ca.xhat_out = train ? p.xh1 : nullptr; ca.rstd_out = train ? p.r1 : nullptr;
    ca.gamma = prm.norm1_w; ca.beta = prm.norm1_b; ca.relu = 1; ca.osign = 1.f;
    launch_combine_gn(d, ca, st);
  }
  v_ready = false;

  if (tiny) {     // latency path: conv + bias + t * tmap + GroupNorm (+ ReLU) per launch
    TinyConvArgs t1;
    memset(&t1, 0, sizeof(t1));
    t1.act = p.act1; t1.wq = p.wtiny[0]; t1.bias = prm.conv1_b; t1.tmap = p.tmap[0]; t1.et = et;
    t1.gamma = prm.norm2_w; t1.beta = prm.norm2_b; t1.out = p.act2; t1.part = p.tpart; t1.counter = p.tcount; t1.ctrl = p.ctrl;
    t1.relu = 1; t1.osign = 1.f;
    { ProfScope ps(0, conv_flops(), st); launch_tiny_conv_gn(d, t1, st); }
    TinyConvArgs t2 = t1;
    t2.act = p.act2; t2.wq = p.wtiny[1]; t2.bias = prm.conv2_b; t2.tmap = p.tmap[1];
    t2.gamma = prm.norm3_w; t2.beta = prm.norm3_b; t2.out = k_out; t2.relu = 0; t2.osign = et.tsign;
    if (next != nullptr) {     // the next evaluation's combine -> GroupNorm-1 -> ReLU rides in this launch
      t2.nx_on = 1; t2.nx = next->cy; t2.nx_self = -1;
      for (int j = 0; j < next->cy.nk; ++j)
        if (next->cy.k[j] == k_out) t2.nx_self = j;
      t2.nx_y_out = next->y_out; t2.nx_gamma = prm.norm1_w; t2.nx_beta = prm.norm1_b; t2.nx_act = p.act1;
      v_ready = true;
    }
    { ProfScope ps(0, conv_flops(), st); launch_tiny_conv_gn(d, t2, st); }
    if (count_nfe) nfe += 1;
    return check_launch("odefunc forward (latency path)");
  }

  ConvArgs c1;
  memset(&c1, 0, sizeof(c1));
  c1.in = p.act1; c1.wpacked = p.wf[0]; c1.mode = CM_FWD_GN_RELU;
  c1.bias = prm.conv1_b; c1.tmap = p.tmap[0]; c1.et = et;
  c1.gamma = prm.norm2_w; c1.beta = prm.norm2_b; c1.osign = 1.f;
  c1.out = p.act2; c1.xhat_out = train ? p.xh2 : nullptr; c1.rstd_out = train ? p.r2 : nullptr;
  const bool small = small_mode() && !train;
  c1.raw_out = (d.csplit || small) ? p.RAW : nullptr;
  if (small) c1.wpacked = p.wsmall[0];
  { ProfScope ps(0, conv_flops(), st); if (small) launch_conv_small(d, c1, st); else launch_conv(d, c1, st); }
  if (d.csplit || small) gn_pass_fwd(prm.norm2_w, prm.norm2_b, 1, 1.f, p.act2, train ? p.xh2 : nullptr, train ? p.r2 : nullptr);

  ConvArgs c2 = c1;
  c2.in = p.act2; c2.wpacked = small ? p.wsmall[1] : p.wf[1]; c2.mode = CM_FWD_GN;
  c2.bias = prm.conv2_b; c2.tmap = p.tmap[1];
  c2.gamma = prm.norm3_w; c2.beta = prm.norm3_b; c2.osign = et.tsign;
  c2.out = k_out; c2.xhat_out = train ? p.xh3 : nullptr; c2.rstd_out = train ? p.r3 : nullptr;
  { ProfScope ps(0, conv_flops(), st); if (small) launch_conv_small(d, c2, st); else launch_conv(d, c2, st); }
  if (d.csplit || small) gn_pass_fwd(prm.norm3_w, prm.norm3_b, 0, et.tsign, k_out, train ? p.xh3 : nullptr, train ? p.r3 : nullptr);
  if (count_nfe) nfe += 1;
  return check_launch("odefunc forward");
}

int Solver::eval_aug(const Comb& cy, const Comb& ca, float* y_out, float* a_out, const EvalTime& et,
             float* kY_out, float* kA_out, float* kT_out, int kidx, float csign, float* vjp_t_out,
             bool need_theta, const NextComb* next) {
  if (w4) return eval_w4(cy, y_out, et, kY_out, true, &ca, a_out, kA_out, kT_out, kidx, csign, vjp_t_out, need_theta, next);
  TRY(eval_fwd(cy, y_out, et, kY_out, true));

  GnBwdArgs g;
  memset(&g, 0, sizeof(g));
  g.comb = ca; g.ctrl = p.ctrl; g.csign = csign; g.a_out = a_out;
  g.xhat = p.xh3; g.rstd = p.r3; g.gamma = prm.norm3_w; g.dz_out = p.dz2; g.gpart = p.gpart[2]; g.osign = 1.f;
  g.spart = p.spart[1];   // masked column sums of dz2, fused into the pass
  launch_gn_bwd(d, g, st);

  if (need_theta && !d.wgrad_pair) {
    WgradArgs w2;
    memset(&w2, 0, sizeof(w2));
    w2.act = p.act2; w2.dz = p.dz2; w2.wpart = p.wpart[1]; w2.ctrl = p.ctrl;
    { ProfScope ps(1, conv_flops(), st); launch_wgrad(d, w2, st); }
  }

  ConvArgs b2;
  memset(&b2, 0, sizeof(b2));
  b2.in = p.dz2; b2.wpacked = p.wd[1]; b2.mode = CM_BWD_RELU_GN; b2.et = et;
  b2.gamma = prm.norm2_w; b2.osign = 1.f; b2.out = p.dz1;
  b2.act = p.act2; b2.xhat = p.xh2; b2.rstd = p.r2; b2.gpart = p.gpart[1];
  b2.spart = p.spart[0];   // masked column sums of dz1, fused into the epilogue
  b2.raw_out = d.csplit ? p.RAW : nullptr;
  { ProfScope ps(0, conv_flops(), st); launch_conv(d, b2, st); }
  if (d.csplit) gn_pass_bwd(p.act2, p.xh2, p.r2, prm.norm2_w, 1.f, p.dz1, p.gpart[1], p.spart[0]);

  if (need_theta) {   // dz1 exists now: with pairing, conv2's weight gradient rides in the same launch (grid.z = 1)
    WgradArgs w1;
    memset(&w1, 0, sizeof(w1));
    w1.act = p.act1; w1.dz = p.dz1; w1.wpart = p.wpart[0]; w1.ctrl = p.ctrl;
    if (d.wgrad_pair) { w1.act2 = p.act2; w1.dz2 = p.dz2; w1.wpart2 = p.wpart[1]; }
    { ProfScope ps(1, (d.wgrad_pair ? 2.0 : 1.0) * conv_flops(), st); launch_wgrad(d, w1, st); }
  }

  ConvArgs b1 = b2;
  b1.spart = nullptr;
  b1.in = p.dz1; b1.wpacked = p.wd[0];
  b1.gamma = prm.norm1_w; b1.osign = et.tsign; b1.out = kA_out;
  b1.act = p.act1; b1.xhat = p.xh1; b1.rstd = p.r1; b1.gpart = p.gpart[0];
  { ProfScope ps(0, conv_flops(), st); launch_conv(d, b1, st); }
  if (d.csplit) gn_pass_bwd(p.act1, p.xh1, p.r1, prm.norm1_w, et.tsign, kA_out, p.gpart[0], nullptr);

  if (!need_theta) return check_launch("augmented dynamics");
  ThetaFinalizeArgs tf;
  memset(&tf, 0, sizeof(tf));
  tf.wpart[0] = p.wpart[0]; tf.wpart[1] = p.wpart[1];
  tf.spart[0] = p.spart[0]; tf.spart[1] = p.spart[1];
  tf.gpart[0] = p.gpart[0]; tf.gpart[1] = p.gpart[1]; tf.gpart[2] = p.gpart[2];
  tf.gpart_rows[0] = tf.gpart_rows[1] = d.csplit ? d.N : d.mtiles;   // (split-conv mode: per-sample partials from the GroupNorm pass)
  tf.gpart_rows[2] = d.N;
  tf.wtime[0] = p.wtime[0]; tf.wtime[1] = p.wtime[1]; tf.sred = p.sred;
  tf.et = et; tf.osign = et.tsign; tf.theta_out = kT_out;
  tf.ctrl = p.ctrl; tf.kidx = kidx; tf.write_scalar = kidx >= 0 ? 1 : 0; tf.vjp_t_out = vjp_t_out;
  launch_theta_finalize(d, tf, st);
  return check_launch("augmented dynamics");
}

int Solver::eval_sys(int kout, const double* coef, int ncoef, int scale_mode, const EvalTime& et, bool write_new,
                     bool need_theta, const double* next_coef, int next_ncoef, bool next_write_new) {
  Comb cy = make_comb(p.Y, p.KY, coef, ncoef, scale_mode);
  NextComb nc;
  const NextComb* next = nullptr;
  if ((w4 || (tiny_mode() && !aug)) && next_coef != nullptr) {
    nc.cy = make_comb(p.Y, p.KY, next_coef, next_ncoef, scale_mode);
    nc.y_out = next_write_new ? p.Y1 : nullptr;
    next = &nc;
  }
  if (!aug) return eval_fwd(cy, write_new ? p.Y1 : nullptr, et, p.KY[kout], false, next);
  Comb ca = make_comb(p.A, p.KA, coef, ncoef, scale_mode);
  return eval_aug(cy, ca, write_new ? p.Y1 : nullptr, write_new ? p.A1 : nullptr, et,
                  p.KY[kout], p.KA[kout], p.KT[kout], kout, -1.f, nullptr, need_theta, next);
}

// (measured and not kept, profiles/r05_poll_readback_ab.txt: the record stored into coherent pinned memory by a one-thread launch and
//  a host spin on its sequence number instead of copy + synchronise -- 0.884 vs 0.883 of the deferred rate: hipStreamSynchronize spins too)
int Solver::readback() {
  HIP_TRY(hipMemcpyAsync(hctrl, p.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return NODE_OK;
}

int Solver::initial_step() {
  const int nseg = aug ? 3 : 1;
  InitSeg segs[3] = {{p.Y, p.KY[0], p.KY[1], d.numel}, {p.A, p.KA[0], p.KA[1], d.numel}, {p.TH, p.KT[0], p.KT[1], d.P}};
  InitCtlArgs ic;
  memset(&ic, 0, sizeof(ic));
  ic.ctrl = p.ctrl;
  for (int i = 0; i < nseg; ++i) { ic.partial[i] = p.partial[i]; ic.numel[i] = (double)segs[i].n; }
  ic.nseg = nseg; ic.has_scalar = aug ? 1 : 0; ic.phase = 0; ic.rtol = rtol; ic.atol = atol;
  launch_init_norms(segs, p.partial, nseg, rtol, atol, 0, st);
  if (nr_fn != nullptr) { norm_exchange(1, nseg); ic.gbuf = nr_buf; ic.gworld = nr_world; }
  launch_init_controller(ic, st);
  const double one[1] = {1.0};
  TRY(eval_sys(1, one, 1, SC_H0, et_probe(), false));
  ic.phase = 1;
  launch_init_norms(segs, p.partial, nseg, rtol, atol, 1, st);
  if (nr_fn != nullptr) norm_exchange(2, nseg);
  launch_init_controller(ic, st);
  return check_launch("initial step");
}

int Solver::enqueue_step(const StepIO& io) {
  // stage 2 (s == 0): its parameter / time derivative has zero weight everywhere (see eval_aug)
  static const int skip_k2 = env_int("NODE_TUNE_SKIP_K2_THETA", 1);
  const bool was_counting = count_nfe;
  count_nfe = false;
  for (int s = 0; s < 6; ++s) {
    const int rc = eval_sys(s + 1, DP_BETA[s], s + 1, SC_DT, et_stage(DP_ALPHA[s]), s == 5, !(skip_k2 && s == 0),
                            s < 5 ? DP_BETA[s + 1] : nullptr, s + 2, s + 1 == 5);
    if (rc != NODE_OK) { count_nfe = was_counting; tf_waiting = false; return rc; }
  }
  count_nfe = was_counting;
  if (tf_waiting) {     // (the last stage has no `next`: nothing can wait here)
    tf_waiting = false;
    return fail(NODE_ERR_HIP, "a theta finalize was left waiting at the end of a dopri5 step");
  }
  const int nseg = aug ? 3 : 1;
  ErrSeg es[3];
  es[0].y0 = p.Y; es[0].y1 = p.Y1; es[0].n = d.numel; es[0].compute_y1 = 0;
  for (int j = 0; j < 7; ++j) es[0].k[j] = p.KY[j];
  if (aug) {
    es[1] = es[0];
    es[1].y0 = p.A; es[1].y1 = p.A1;
    for (int j = 0; j < 7; ++j) es[1].k[j] = p.KA[j];
    es[2].y0 = p.TH; es[2].y1 = p.TH1; es[2].n = d.P; es[2].compute_y1 = 1;
    for (int j = 0; j < 7; ++j) es[2].k[j] = p.KT[j];
  }
  StepCtlArgs sc;
  memset(&sc, 0, sizeof(sc));
  sc.ctrl = p.ctrl;
  sc.partial[0] = p.partial[0]; sc.partial[1] = p.partial[1]; sc.partial[2] = p.partial[2];
  sc.numel[0] = (double)d.numel; sc.numel[1] = (double)d.numel; sc.numel[2] = (double)d.P;
  sc.nseg = nseg; sc.has_scalar = aug ? 1 : 0; sc.rtol = rtol; sc.atol = atol;
  sc.targets = p.targets; sc.n_targets = io.n_targets;
  sc.forced = io.n_forced > 0 ? p.forced : nullptr; sc.n_forced = io.n_forced;
  sc.dt_log = io.log_cap > 0 ? p.dtlog : nullptr; sc.dt_log_cap = io.log_cap;
  sc.interp_scalar = aug ? 1 : 0;
  sc.w4sc = (aug && w4_f16) ? p.w4sc : nullptr;
  launch_error_norm(es, p.partial, nseg, p.ctrl, rtol, atol, st);
  if (nr_fn != nullptr) { norm_exchange(0, nseg); sc.gbuf = nr_buf; sc.gworld = nr_world; }
  launch_step_controller(sc, st);
  if (!aug) {
    EmitArgs ea;
    ea.ctrl = p.ctrl; ea.targets = p.targets; ea.y0 = p.Y; ea.y1 = p.Y1;
    for (int j = 0; j < 7; ++j) ea.k[j] = p.KY[j];
    ea.y_out = io.y_out;
    if (w4) launch_w4s_emit_outputs(d, ea, st);
    else launch_emit_outputs(d, ea, st);
  }
  CommitArgs cm;
  memset(&cm, 0, sizeof(cm));
  cm.ctrl = p.ctrl; cm.targets = p.targets; cm.nseg = nseg; cm.interp_final = aug ? 1 : 0;
  cm.y[0] = p.Y; cm.y1[0] = p.Y1; cm.k0[0] = p.KY[0]; cm.k6[0] = p.KY[6]; cm.n[0] = d.numel;
  for (int j = 0; j < 7; ++j) cm.k[0][j] = p.KY[j];
  if (aug) {
    // (the y segment is reloaded from the forward trajectory at every interval: its dense output is not needed,
    //  but it is cheap and keeps the three segments uniform)
    cm.y[1] = p.A; cm.y1[1] = p.A1; cm.k0[1] = p.KA[0]; cm.k6[1] = p.KA[6]; cm.n[1] = d.numel;
    cm.y[2] = p.TH; cm.y1[2] = p.TH1; cm.k0[2] = p.KT[0]; cm.k6[2] = p.KT[6]; cm.n[2] = d.P;
    for (int j = 0; j < 7; ++j) { cm.k[1][j] = p.KA[j]; cm.k[2][j] = p.KT[j]; }
  }
  cm.rec = io.rec; cm.miss_flag = io.miss_flag; cm.expect_steps = io.expect_steps;
  launch_commit(cm, st);
  return check_launch("dopri5 step");
}

int Solver::run_steps(const StepIO& io, long long max_steps, int guess, int* status) {
  long long enq = 0;
  long long batch = guess > 0 ? guess : 1;
  for (;;) {
    if (batch > max_steps - enq) batch = max_steps - enq;
    for (long long i = 0; i < batch; ++i) TRY(enqueue_step(io));
    enq += batch;
    TRY(readback());
    if (hctrl->status != 0) { *status = hctrl->status; return NODE_OK; }
    if (hctrl->done) return NODE_OK;
    if (enq >= max_steps) { *status = NODE_ERR_MAX_STEPS; return NODE_OK; }
    batch = 2;
  }
}

int Solver::upload(double* dst, const double* src, int n, double* stage) {
  for (int i = 0; i < n; ++i) stage[i] = src[i];
  HIP_TRY(hipMemcpyAsync(dst, stage, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
  return NODE_OK;
}

int Solver::rk4_interval(double t0, double t1, const float* dot_with, float* dot_out) {
  // upstream keeps the fixed grid in the state dtype (fp32)
  const float t0f = (float)t0, t1f = (float)t1;
  launch_set_ctrl(p.ctrl, (double)t0f, (double)(t1f - t0f), 0, st);
  const double c2[1] = {1.0 / 3}, c3[2] = {-1.0 / 3, 1.0}, c4[3] = {1.0, -1.0, 1.0};
  const double cf[4] = {1.0 / 8, 3.0 / 8, 3.0 / 8, 1.0 / 8};
  TRY(eval_sys(0, nullptr, 0, SC_ABS, et_stage(0.0), false));
  if (dot_with) launch_dot_sub_scalar(p.ctrl, p.KY[0], dot_with, d.numel, tsign, p.partial[0], dot_out, st);   // adjoint: adj_t -= <f_i, g_i>
  TRY(eval_sys(1, c2, 1, SC_DT, et_stage(1.0 / 3), false));
  TRY(eval_sys(2, c3, 2, SC_DT, et_stage(2.0 / 3), false));
  TRY(eval_sys(3, c4, 3, SC_DT, et_stage(1.0), false));
  launch_lincomb(make_comb(p.Y, p.KY, cf, 4, SC_DT), p.ctrl, p.Y1, d.numel, st);
  std::swap(p.Y, p.Y1);
  if (aug) {
    launch_lincomb(make_comb(p.A, p.KA, cf, 4, SC_DT), p.ctrl, p.A1, d.numel, st);
    std::swap(p.A, p.A1);
    launch_lincomb(make_comb(p.TH, p.KT, cf, 4, SC_DT), p.ctrl, p.TH1, d.P, st);
    std::swap(p.TH, p.TH1);
    launch_set_scalar_state(p.ctrl, 0.f, 1, st);
  }
  return check_launch("rk4 interval");
}

}  // namespace node
