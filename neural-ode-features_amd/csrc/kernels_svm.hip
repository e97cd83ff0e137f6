// Finetune evaluation (`evaluate.py finetune` of the reference, evaluate.py:364-413): the linear SVMs of
// GridSearchCV(LinearSVC()) -- L2-regularised squared hinge, one-vs-rest, the bias regularised as column D of x~ = [x, 1] --
// as ONE batch of P problems over a shared X [N, D]:
//
//     f_p(w) = 1/2 |w|^2 + C_p sum_{i in train(p)} max(0, 1 - y_ip w . x~_i)^2
//
// A problem is a row of the table (fold, class, C): row i trains problem p when row_fold[i] != fold_p (fold -1: every
// row, the refit), and y_ip = +1 when labels[i] == class_p, else -1.  Mask, target and C are rebuilt from the table and
// the two per-row arrays inside the kernels; they never exist as [N, P] arrays.
//
// Solver: truncated Newton (Newton-CG) with a backtracking line search, every problem at its own pace, state on the device.
//   k_svm_product<GRAD>  z = X~ w -> Z;  part = X~^T (A o (z - y))         A_ip = train and y z < 1
//   k_svm_product<HV>    u = X~ d;       part = X~^T (A o u)               A from the Z of this Newton iteration
//   k_svm_product<XS>    XS = X~ s                                         (first multiplication only)
// One launch runs both multiplications on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32): a workgroup owns 64 problems
// (their vectors stay in LDS) and a run of 64-row slabs of X; each slab is staged ONCE in LDS, with the bias column and
// the zero padding of D + 1 to an even k written there, multiplied by the vectors [64 x (D+1)] x [(D+1) x 64], turned
// into coefficients in LDS, and multiplied back [64 problems x 64 rows] x [64 rows x (D+1)] into accumulators that live in
// registers across the slabs.  Each workgroup writes one partial [64, D+1]; the per-problem kernels add the partials of
// the row groups in index order in fp64.  No atomics anywhere: results are bit-identical from run to run, and a problem's
// result does not depend on its column.
//   k_svm_newton_begin   g = w + 2C sum(part); |g|; stop test |g| <= eps max(min(#pos, #neg), 1) / n |g(0)|; CG start
//   k_svm_cg_step        Hd = d + 2C sum(part); alpha, s, r, beta, d; CG stops at |r| <= min(0.1, sqrt(|g| / |g0|)) |g|
//   k_svm_ls_partial     sum_i h_i(t)^2 - h_i(0)^2 for t = 1, 1/2, ..., 2^-(LS_NC-1) from Z + t XS, in fp64
//   k_svm_newton_end     first t with f(w + t s) - f(w) <= 0.01 t g.s; w += t s  (none: the problem ends NOT converged)
//   k_svm_status         number of unfinished problems (the one word the host reads per Newton iteration), results
// A finished problem is a predicated exit; a tile of 64 finished problems leaves at once.
//   k_svm_cv_score       per (fold, C) group of K problems: argmax_k w_k . x~_i over the held-out rows (first maximum;
//                        K = 1: the problem's class iff z > 0), integer counts of correct and held-out rows
#include "node_internal.h"

namespace node {

namespace {

constexpr int PT = 64;            // problems per tile
constexpr int RS = 64;            // rows per slab
constexpr int MAXQ = 5;           // second-multiplication tiles per wave: 2 * ceil((D + 1) / 32) <= 4 * MAXQ
constexpr int LS_NC = 12;         // step lengths 1 ... 2^-11
constexpr int LS_RG_ROWS = 256;   // rows per line-search block

typedef float f32x16 __attribute__((ext_vector_type(16)));

enum { MODE_GRAD = 0, MODE_HV = 1, MODE_XS = 2 };

// fp64 sum over a 256-thread workgroup in a fixed order
__device__ __forceinline__ double block_sum(double v, double* wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();                // (wsum may still be read from the previous call)
  if (lane == 0) wsum[wave] = v;
  __syncthreads();
  return (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

template <int MODE>
__global__ __launch_bounds__(256) void k_svm_product(const float* __restrict__ x, const int* __restrict__ labels,
                                                     const int* __restrict__ row_fold, const node_svm_problem* __restrict__ prob,
                                                     const SvmState* __restrict__ st, const float* __restrict__ v,
                                                     float* __restrict__ zbuf, float* __restrict__ xsbuf, float* __restrict__ part,
                                                     int n, int d, int p, int slabs, int slabs_per_group) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int d1 = d + 1, d1p = (d1 + 1) & ~1, ld = d1p + 1;
  float* xs = smem;                       // [RS][ld]
  float* vs = xs + RS * ld;               // [PT][ld]
  float* us = vs + PT * ld;               // [RS][PT + 1]
  int* pfold = (int*)(us + RS * (PT + 1));
  int* pcls = pfold + PT;
  int* pact = pcls + PT;
  int* rlab = pact + PT;
  int* rfold = rlab + RS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p0 = blockIdx.x * PT;
  const int s0 = blockIdx.y * slabs_per_group;
  const int s1 = s0 + slabs_per_group < slabs ? s0 + slabs_per_group : slabs;

  int act = 0;
  if (tid < PT) {
    const int gp = p0 + tid;
    if (gp < p) {
      act = !st[gp].done && (MODE != MODE_HV || !st[gp].cg_done);
      pfold[tid] = prob[gp].fold;
      pcls[tid] = prob[gp].cls;
    } else {
      pfold[tid] = 0;
      pcls[tid] = 0;
    }
    pact[tid] = act;
  }
  if (!__syncthreads_or(act)) return;

  for (int row = wave; row < PT; row += 4) {
    const int gp = p0 + row;
    for (int col = lane; col < ld; col += 64)
      vs[row * ld + col] = (gp < p && col < d1) ? v[(size_t)gp * d1 + col] : 0.f;
  }

  const int r = lane & 31, h = lane >> 5;
  const int rw = (wave >> 1) * 32, cw = (wave & 1) * 32;
  const int ntiles = 2 * ((d1 + 31) / 32);
  f32x16 acc2[MAXQ];
  for (int q = 0; q < MAXQ; ++q)
    for (int i = 0; i < 16; ++i) acc2[q][i] = 0.f;

  for (int sl = s0; sl < s1; ++sl) {
    const int i0 = sl * RS;
    for (int row = wave; row < RS; row += 4) {
      const int gi = i0 + row;
      const float* __restrict__ xr = x + (size_t)(gi < n ? gi : 0) * d;
      for (int col = lane; col < ld; col += 64)
        xs[row * ld + col] = gi < n ? (col < d ? xr[col] : (col == d ? 1.f : 0.f)) : 0.f;
    }
    if (tid < RS) {
      const int gi = i0 + tid;
      rlab[tid] = gi < n ? labels[gi] : 0;
      rfold[tid] = gi < n ? row_fold[gi] : 0;
    }
    __syncthreads();

    // [RS x d1p] x [d1p x PT]: lane (r, h) holds A[i = r][k = h] and B[k = h][j = r] of each 32 x 32 x 2 step
    f32x16 acc;
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    {
      const float* __restrict__ xa = xs + (rw + r) * ld + h;
      const float* __restrict__ vb = vs + (cw + r) * ld + h;
      for (int kk = 0; kk < d1p; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[kk], vb[kk], acc, 0, 0, 0);
    }
    // C/D: column lane & 31 (the problem), row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    {
      const int pc = cw + r, gp = p0 + pc;
      const int fold_p = pfold[pc], cls_p = pcls[pc];
      const bool pok = gp < p && pact[pc];
      for (int i = 0; i < 16; ++i) {
        const int rl = rw + (i & 3) + 8 * (i >> 2) + 4 * h;
        const int gi = i0 + rl;
        const bool ok = pok && gi < n;
        if (MODE == MODE_XS) {
          if (ok) xsbuf[(size_t)gi * p + gp] = acc[i];
        } else {
          const float y = rlab[rl] == cls_p ? 1.f : -1.f;
          const bool train = ok && rfold[rl] != fold_p;
          float coef;
          if (MODE == MODE_GRAD) {
            const float z = acc[i];
            if (ok) zbuf[(size_t)gi * p + gp] = z;
            coef = (train && y * z < 1.f) ? z - y : 0.f;
          } else {
            const float z = ok ? zbuf[(size_t)gi * p + gp] : 0.f;
            coef = (train && y * z < 1.f) ? acc[i] : 0.f;
          }
          us[rl * (PT + 1) + pc] = coef;
        }
      }
    }
    __syncthreads();
    if (MODE != MODE_XS) {
      // [PT x RS] x [RS x d1p]: A[i = problem][k = row] = us[row][problem], B[k = row][j = feature] = xs[row][feature]
#pragma unroll
      for (int q = 0; q < MAXQ; ++q) {
        const int t = wave + 4 * q;
        if (t < ntiles) {
          const int m0 = (t & 1) * 32, j = (t >> 1) * 32 + r;
          const bool jok = j < d1p;
          const float* __restrict__ ua = us + h * (PT + 1) + m0 + r;
          const float* __restrict__ xb = xs + h * ld + (jok ? j : 0);
          f32x16 a2 = acc2[q];
          for (int kk = 0; kk < RS; kk += 2) {
            const float b = xb[kk * ld];
            a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[kk * (PT + 1)], jok ? b : 0.f, a2, 0, 0, 0);
          }
          acc2[q] = a2;
        }
      }
      __syncthreads();
    }
  }

  if (MODE != MODE_XS) {
    float* __restrict__ out = part + (size_t)blockIdx.y * p * d1;
#pragma unroll
    for (int q = 0; q < MAXQ; ++q) {
      const int t = wave + 4 * q;
      if (t < ntiles) {
        const int m0 = (t & 1) * 32, j = (t >> 1) * 32 + r;
        if (j < d1) {
          for (int i = 0; i < 16; ++i) {
            const int gp = p0 + m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (gp < p) out[(size_t)gp * d1 + j] = acc2[q][i];
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_svm_init(const int* __restrict__ labels, const int* __restrict__ row_fold,
                                                  const node_svm_problem* __restrict__ prob, SvmState* __restrict__ st,
                                                  float* __restrict__ w, int n, int d1) {
  __shared__ double wsum[4];
  const int pi = blockIdx.x, tid = threadIdx.x;
  const int fold = prob[pi].fold, cls = prob[pi].cls;
  int nt = 0, np = 0;
  for (int i = tid; i < n; i += 256) {
    if (row_fold[i] != fold) {
      ++nt;
      np += labels[i] == cls;
    }
  }
  const double tn = block_sum((double)nt, wsum);      // (counts below 2^31 are exact in fp64)
  const double tp = block_sum((double)np, wsum);
  for (int m = tid; m < d1; m += 256) w[(size_t)pi * d1 + m] = 0.f;
  if (tid == 0) {
    SvmState s;
    s.rr = 0.0;
    s.gnorm = 0.0;
    s.gnorm0 = -1.0;
    s.thresh = 0.0;
    s.cg_tol2 = 0.0;
    s.ratio = 1.0;
    s.n_train = (int)tn;
    s.n_pos = (int)tp;
    s.iters = 0;
    s.done = 0;
    s.converged = 0;
    s.cg_done = 0;
    s.cg_iters = 0;
    s.pad = 0;
    st[pi] = s;
  }
}

__global__ __launch_bounds__(256) void k_svm_newton_begin(const float* __restrict__ part, const float* __restrict__ w,
                                                          float* __restrict__ g, float* __restrict__ s, float* __restrict__ rv,
                                                          float* __restrict__ dv, SvmState* __restrict__ st,
                                                          const node_svm_problem* __restrict__ prob, int groups, int p, int d1,
                                                          int last, double eps) {
  __shared__ double wsum[4];
  const int pi = blockIdx.x, tid = threadIdx.x;
  if (st[pi].done) return;
  const double c2 = 2.0 * (double)prob[pi].c;
  double gg = 0.0;
  for (int m = tid; m < d1; m += 256) {
    double sum = 0.0;
    for (int gi = 0; gi < groups; ++gi) sum += (double)part[((size_t)gi * p + pi) * d1 + m];
    const size_t e = (size_t)pi * d1 + m;
    const float gm = (float)((double)w[e] + c2 * sum);
    g[e] = gm;
    s[e] = 0.f;
    rv[e] = -gm;
    dv[e] = -gm;
    gg += (double)gm * (double)gm;
  }
  gg = block_sum(gg, wsum);
  if (tid == 0) {
    SvmState t = st[pi];
    const double gn = sqrt(gg);
    if (t.gnorm0 < 0.0) {
      t.gnorm0 = gn;
      const int neg = t.n_train - t.n_pos;
      const int mn = t.n_pos < neg ? t.n_pos : neg;
      t.thresh = eps * (double)(mn > 1 ? mn : 1) / (double)(t.n_train > 1 ? t.n_train : 1) * gn;
    }
    t.gnorm = gn;
    t.ratio = t.gnorm0 > 0.0 ? gn / t.gnorm0 : 0.0;
    if (gn <= t.thresh) {
      t.done = 1;
      t.converged = 1;
    } else if (last) {
      t.done = 1;
      t.converged = 0;
    }
    const double rel = sqrt(t.ratio) < 0.1 ? sqrt(t.ratio) : 0.1;
    t.rr = gg;
    t.cg_tol2 = rel * rel * gg;
    t.cg_done = 0;
    t.cg_iters = 0;
    st[pi] = t;
  }
}

__global__ __launch_bounds__(256) void k_svm_cg_step(const float* __restrict__ part, float* __restrict__ s, float* __restrict__ rv,
                                                     float* __restrict__ dv, SvmState* __restrict__ st,
                                                     const node_svm_problem* __restrict__ prob, int groups, int p, int d1,
                                                     int cg_max) {
  __shared__ double wsum[4];
  const int pi = blockIdx.x, tid = threadIdx.x;
  const SvmState t0 = st[pi];
  if (t0.done || t0.cg_done) return;
  const double c2 = 2.0 * (double)prob[pi].c;
  // D + 1 <= 2 * 256 (SVM_MAX_D): at most two entries per thread, kept in registers between the two reductions
  double hd[2], dd[2];
  double dhd = 0.0;
  for (int q = 0; q < 2; ++q) {
    const int m = tid + 256 * q;
    hd[q] = dd[q] = 0.0;
    if (m < d1) {
      double sum = 0.0;
      for (int gi = 0; gi < groups; ++gi) sum += (double)part[((size_t)gi * p + pi) * d1 + m];
      dd[q] = (double)dv[(size_t)pi * d1 + m];
      hd[q] = dd[q] + c2 * sum;
      dhd += dd[q] * hd[q];
    }
  }
  dhd = block_sum(dhd, wsum);
  if (!(dhd > 0.0)) {                       // H >= I: only a zero direction gets here
    if (tid == 0) st[pi].cg_done = 1;
    return;
  }
  const double alpha = t0.rr / dhd;
  double rn[2];
  double rr = 0.0;
  for (int q = 0; q < 2; ++q) {
    const int m = tid + 256 * q;
    rn[q] = 0.0;
    if (m < d1) {
      const size_t e = (size_t)pi * d1 + m;
      s[e] = (float)((double)s[e] + alpha * dd[q]);
      const float rf = (float)((double)rv[e] - alpha * hd[q]);
      rv[e] = rf;
      rn[q] = (double)rf;
      rr += rn[q] * rn[q];
    }
  }
  rr = block_sum(rr, wsum);
  const double beta = rr / t0.rr;
  for (int q = 0; q < 2; ++q) {
    const int m = tid + 256 * q;
    if (m < d1) dv[(size_t)pi * d1 + m] = (float)(rn[q] + beta * dd[q]);
  }
  if (tid == 0) {
    st[pi].rr = rr;
    st[pi].cg_iters = t0.cg_iters + 1;
    if (rr <= t0.cg_tol2 || t0.cg_iters + 1 >= cg_max) st[pi].cg_done = 1;
  }
}

__global__ __launch_bounds__(256) void k_svm_ls_partial(const float* __restrict__ zbuf, const float* __restrict__ xsbuf,
                                                        const int* __restrict__ labels, const int* __restrict__ row_fold,
                                                        const node_svm_problem* __restrict__ prob, const SvmState* __restrict__ st,
                                                        double* __restrict__ lspart, int n, int p, int rows_per_group) {
  __shared__ double red[3][PT][LS_NC];
  const int tid = threadIdx.x, px = tid & 63, ry = tid >> 6;
  const int gp = blockIdx.x * PT + px;
  const bool act = gp < p && !st[gp].done;
  if (!__syncthreads_or(act)) return;
  const int i0 = blockIdx.y * rows_per_group;
  const int i1 = i0 + rows_per_group < n ? i0 + rows_per_group : n;
  double acc[LS_NC];
  for (int k = 0; k < LS_NC; ++k) acc[k] = 0.0;
  if (act) {
    const int fold = prob[gp].fold, cls = prob[gp].cls;
    for (int i = i0 + ry; i < i1; i += 4) {
      if (row_fold[i] == fold) continue;
      const double y = labels[i] == cls ? 1.0 : -1.0;
      const double z = (double)zbuf[(size_t)i * p + gp], u = (double)xsbuf[(size_t)i * p + gp];
      const double m0 = 1.0 - y * z, yu = y * u;
      const double h0 = m0 > 0.0 ? m0 * m0 : 0.0;
      double t = 1.0;
      for (int k = 0; k < LS_NC; ++k) {
        const double mk = m0 - t * yu;
        acc[k] += (mk > 0.0 ? mk * mk : 0.0) - h0;
        t *= 0.5;
      }
    }
  }
  if (ry > 0)
    for (int k = 0; k < LS_NC; ++k) red[ry - 1][px][k] = acc[k];
  __syncthreads();
  if (ry == 0 && act) {
    for (int k = 0; k < LS_NC; ++k)
      lspart[((size_t)blockIdx.y * p + gp) * LS_NC + k] = ((acc[k] + red[0][px][k]) + red[1][px][k]) + red[2][px][k];
  }
}

__global__ __launch_bounds__(256) void k_svm_newton_end(const double* __restrict__ lspart, float* __restrict__ w,
                                                        const float* __restrict__ s, const float* __restrict__ g,
                                                        SvmState* __restrict__ st, const node_svm_problem* __restrict__ prob,
                                                        int ls_groups, int p, int d1) {
  __shared__ double wsum[4];
  __shared__ double dl[LS_NC];
  __shared__ double step;
  const int pi = blockIdx.x, tid = threadIdx.x;
  if (st[pi].done) return;
  double ws = 0.0, ss = 0.0, gs = 0.0;
  for (int m = tid; m < d1; m += 256) {
    const size_t e = (size_t)pi * d1 + m;
    const double sm = (double)s[e];
    ws += (double)w[e] * sm;
    ss += sm * sm;
    gs += (double)g[e] * sm;
  }
  ws = block_sum(ws, wsum);
  ss = block_sum(ss, wsum);
  gs = block_sum(gs, wsum);
  if (tid < LS_NC) {
    double sum = 0.0;
    for (int gi = 0; gi < ls_groups; ++gi) sum += lspart[((size_t)gi * p + pi) * LS_NC + tid];
    dl[tid] = sum;
  }
  __syncthreads();
  if (tid == 0) {
    const double c = (double)prob[pi].c;
    double t = 1.0, found = 0.0;
    for (int k = 0; k < LS_NC; ++k) {
      const double df = t * ws + 0.5 * t * t * ss + c * dl[k];
      if (gs < 0.0 && df <= 0.01 * t * gs) {
        found = t;
        break;
      }
      t *= 0.5;
    }
    step = found;
    if (found == 0.0) {            // no decrease along s at any step length: the rounding floor of fp32; ends NOT converged
      st[pi].done = 1;
      st[pi].converged = 0;
    } else {
      st[pi].iters += 1;
    }
  }
  __syncthreads();
  const double t = step;
  if (t == 0.0) return;
  for (int m = tid; m < d1; m += 256) {
    const size_t e = (size_t)pi * d1 + m;
    w[e] = (float)((double)w[e] + t * (double)s[e]);
  }
}

__global__ __launch_bounds__(256) void k_svm_status(const SvmState* __restrict__ st, node_svm_result* __restrict__ res,
                                                    int* __restrict__ flag, int p) {
  __shared__ double wsum[4];
  int open = 0;
  for (int pi = threadIdx.x; pi < p; pi += 256) {
    const SvmState t = st[pi];
    open += !t.done;
    node_svm_result r;
    r.iterations = t.iters;
    r.converged = t.converged;
    r.grad_ratio = t.ratio;
    res[pi] = r;
  }
  const double all = block_sum((double)open, wsum);
  if (threadIdx.x == 0) flag[0] = (int)all;
}

__global__ __launch_bounds__(256) void k_svm_cv_score(const float* __restrict__ x, const int* __restrict__ labels,
                                                      const int* __restrict__ row_fold, const node_svm_problem* __restrict__ prob,
                                                      const float* __restrict__ w, const int* __restrict__ group_problems, int k,
                                                      int neg_class, int* __restrict__ correct, int* __restrict__ held,
                                                      int* __restrict__ pred, int n, int d) {
  __shared__ double wsum[4];
  const int g = blockIdx.x, tid = threadIdx.x, d1 = d + 1;
  const int* __restrict__ gp = group_problems + (size_t)g * k;
  const int fold = prob[gp[0]].fold;
  int nc = 0, nh = 0;
  for (int i = tid; i < n; i += 256) {
    int guess = -1;
    if (row_fold[i] == fold) {
      const float* __restrict__ xr = x + (size_t)i * d;
      float best = 0.f;
      for (int c = 0; c < k; ++c) {
        const float* __restrict__ wr = w + (size_t)gp[c] * d1;
        float z = wr[d];
        for (int m = 0; m < d; ++m) z = fmaf(wr[m], xr[m], z);
        if (k == 1) {
          guess = z > 0.f ? prob[gp[0]].cls : neg_class;
        } else if (c == 0 || z > best) {          // strict: the first maximum wins
          best = z;
          guess = prob[gp[c]].cls;
        }
      }
      ++nh;
      nc += guess == labels[i];
    }
    if (pred) pred[(size_t)g * n + i] = guess;
  }
  const double tc = block_sum((double)nc, wsum);
  const double th = block_sum((double)nh, wsum);
  if (tid == 0) {
    correct[g] = (int)tc;
    held[g] = (int)th;
  }
}

size_t product_lds_bytes(int d) {
  const int d1p = (d + 2) & ~1, ld = d1p + 1;
  return (size_t)(RS + PT) * ld * sizeof(float) + (size_t)RS * (PT + 1) * sizeof(float) + (3 * PT + 2 * RS) * sizeof(int);
}

template <int MODE>
void launch_product(const SvmPlan& pl, const float* x, const int* labels, const int* row_fold, const node_svm_problem* prob,
                    const SvmState* st, const float* v, float* zbuf, float* xsbuf, float* part, hipStream_t s) {
  static bool lds_ok[MAX_DEVICES] = {};
  allow_full_lds((const void*)k_svm_product<MODE>, lds_ok);
  dim3 grid((pl.p + PT - 1) / PT, pl.groups);
  hipLaunchKernelGGL(k_svm_product<MODE>, grid, dim3(256), product_lds_bytes(pl.d), s, x, labels, row_fold, prob, st, v, zbuf, xsbuf,
                     part, pl.n, pl.d, pl.p, pl.slabs, pl.slabs_per_group);
}

}  // namespace

SvmPlan svm_plan(int n, int d, int p) {
  SvmPlan pl;
  pl.n = n;
  pl.d = d;
  pl.p = p;
  pl.slabs = (n + RS - 1) / RS;
  const int ptiles = (p + PT - 1) / PT;
  int groups = (256 + ptiles - 1) / ptiles;            // about one workgroup per compute unit
  if (groups > pl.slabs) groups = pl.slabs;
  pl.slabs_per_group = (pl.slabs + groups - 1) / groups;
  pl.groups = (pl.slabs + pl.slabs_per_group - 1) / pl.slabs_per_group;
  pl.ls_rows = LS_RG_ROWS;
  pl.ls_groups = (n + LS_RG_ROWS - 1) / LS_RG_ROWS;
  pl.ls_nc = LS_NC;
  return pl;
}

void launch_svm_init(const SvmPlan& pl, const int* labels, const int* row_fold, const node_svm_problem* prob, SvmState* st, float* w,
                     hipStream_t s) {
  hipLaunchKernelGGL(k_svm_init, dim3(pl.p), dim3(256), 0, s, labels, row_fold, prob, st, w, pl.n, pl.d + 1);
}

void launch_svm_product(const SvmPlan& pl, int mode, const float* x, const int* labels, const int* row_fold,
                        const node_svm_problem* prob, const SvmState* st, const float* v, float* zbuf, float* xsbuf, float* part,
                        hipStream_t s) {
  if (mode == MODE_GRAD) launch_product<MODE_GRAD>(pl, x, labels, row_fold, prob, st, v, zbuf, xsbuf, part, s);
  else if (mode == MODE_HV) launch_product<MODE_HV>(pl, x, labels, row_fold, prob, st, v, zbuf, xsbuf, part, s);
  else launch_product<MODE_XS>(pl, x, labels, row_fold, prob, st, v, zbuf, xsbuf, part, s);
}

void launch_svm_newton_begin(const SvmPlan& pl, const float* part, const float* w, float* g, float* sv, float* rv, float* dv,
                             SvmState* st, const node_svm_problem* prob, int last, double eps, hipStream_t s) {
  hipLaunchKernelGGL(k_svm_newton_begin, dim3(pl.p), dim3(256), 0, s, part, w, g, sv, rv, dv, st, prob, pl.groups, pl.p, pl.d + 1,
                     last, eps);
}

void launch_svm_cg_step(const SvmPlan& pl, const float* part, float* sv, float* rv, float* dv, SvmState* st,
                        const node_svm_problem* prob, int cg_max, hipStream_t s) {
  hipLaunchKernelGGL(k_svm_cg_step, dim3(pl.p), dim3(256), 0, s, part, sv, rv, dv, st, prob, pl.groups, pl.p, pl.d + 1, cg_max);
}

void launch_svm_line_search(const SvmPlan& pl, const float* zbuf, const float* xsbuf, const int* labels, const int* row_fold,
                            const node_svm_problem* prob, SvmState* st, double* lspart, float* w, const float* sv, const float* g,
                            hipStream_t s) {
  dim3 grid((pl.p + PT - 1) / PT, pl.ls_groups);
  hipLaunchKernelGGL(k_svm_ls_partial, grid, dim3(256), 0, s, zbuf, xsbuf, labels, row_fold, prob, st, lspart, pl.n, pl.p, pl.ls_rows);
  hipLaunchKernelGGL(k_svm_newton_end, dim3(pl.p), dim3(256), 0, s, lspart, w, sv, g, st, prob, pl.ls_groups, pl.p, pl.d + 1);
}

void launch_svm_status(const SvmPlan& pl, const SvmState* st, node_svm_result* res, int* flag, hipStream_t s) {
  hipLaunchKernelGGL(k_svm_status, dim3(1), dim3(256), 0, s, st, res, flag, pl.p);
}

void launch_svm_cv_score(int n, int d, int n_groups, int k, const float* x, const int* labels, const int* row_fold,
                         const node_svm_problem* prob, const float* w, const int* group_problems, int neg_class, int* correct,
                         int* held, int* pred, hipStream_t s) {
  hipLaunchKernelGGL(k_svm_cv_score, dim3(n_groups), dim3(256), 0, s, x, labels, row_fold, prob, w, group_problems, k, neg_class,
                     correct, held, pred, n, d);
}

}  // namespace node
