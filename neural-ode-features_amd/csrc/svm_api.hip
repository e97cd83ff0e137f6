// C ABI of the finetune evaluation (include/node_hip.h: node_svm_workspace_bytes / node_svm_fit / node_svm_cv_score): argument
// checks, the workspace plan and the Newton-CG launch sequence of kernels_svm.hip.  Reference: evaluate.py:364-413.
//
// One Newton iteration of a chunk of problems is a fixed sequence of launches; what a problem still does is decided on the
// device (a finished problem exits at once), and the host reads ONE word per Newton iteration, the number of unfinished
// problems, to stop early.  Nothing is read inside the conjugate-gradient loop: it is enqueued at its full length.
//
//   gradient product -> newton_begin (stop test, CG start) -> status word
//   cg_max x (Hessian-vector product -> cg_step) -> X~ s product -> line search (partials, then step and w += t s)
//
// The workspace holds Z and X~ s ([n, chunk] each), one [groups, chunk, d + 1] set of product partials, the vectors g, s, r, d,
// the line-search partials and the per-problem state.  Above SVM_WS_CAP the problems run in chunks of a multiple of 64.
#include "host_common.h"

using namespace node;

namespace {

constexpr size_t SVM_WS_CAP = (size_t)256 << 20;
constexpr int SVM_CG_MAX = 48;

struct SvmWs {
  float *z, *xs, *part, *g, *s, *r, *d;
  double* lspart;
  SvmState* st;
  int* flag;
};

size_t carve(const SvmPlan& pl, void* base, SvmWs* out) {
  Bump b(base);
  const size_t d1 = (size_t)pl.d + 1, p = (size_t)pl.p;
  SvmWs w;
  w.z = b.take<float>((size_t)pl.n * p);
  w.xs = b.take<float>((size_t)pl.n * p);
  w.part = b.take<float>((size_t)pl.groups * p * d1);
  w.g = b.take<float>(p * d1);
  w.s = b.take<float>(p * d1);
  w.r = b.take<float>(p * d1);
  w.d = b.take<float>(p * d1);
  w.lspart = b.take<double>((size_t)pl.ls_groups * p * pl.ls_nc);
  w.st = b.take<SvmState>(p);
  w.flag = b.take<int>(64);
  if (out) *out = w;
  return (b.off + 255) & ~(size_t)255;
}

// problems per chunk: all of them when that fits SVM_WS_CAP, else the largest multiple of 64 that does (at least 64)
int chunk_size(int n, int d, int p) {
  int pc = p;
  while (pc > 64 && carve(svm_plan(n, d, pc), nullptr, nullptr) > SVM_WS_CAP) pc = ((pc - 1) / 64) * 64;
  return pc;
}

int check_sizes(int n, int d, int p) {
  if (n < 1 || d < 1 || p < 1) return fail(NODE_ERR_SHAPE, "svm shape n=%d d=%d p=%d: every size must be >= 1", n, d, p);
  if (d > SVM_MAX_D)
    return fail(NODE_ERR_UNSUPPORTED, "svm features of width %d: at most %d are supported (a slab of rows and a tile of problems in LDS)",
                d, SVM_MAX_D);
  return NODE_OK;
}

int launch_ok(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
  return NODE_OK;
}

int fit_chunk(int n, int d, int pc, const float* x, const int32_t* labels, const int32_t* row_fold, const node_svm_problem* prob,
              double eps, int max_iter, float* w, node_svm_result* res, void* ws, hipStream_t st) {
  const SvmPlan pl = svm_plan(n, d, pc);
  SvmWs b;
  carve(pl, ws, &b);
  const int cg_max = d + 1 < SVM_CG_MAX ? d + 1 : SVM_CG_MAX;
  launch_svm_init(pl, labels, row_fold, prob, b.st, w, st);
  TRY(launch_ok("k_svm_init"));
  for (int it = 0;; ++it) {
    launch_svm_product(pl, 0, x, labels, row_fold, prob, b.st, w, b.z, b.xs, b.part, st);
    TRY(launch_ok("k_svm_product<GRAD>"));
    launch_svm_newton_begin(pl, b.part, w, b.g, b.s, b.r, b.d, b.st, prob, it >= max_iter, eps, st);
    launch_svm_status(pl, b.st, res, b.flag, st);
    TRY(launch_ok("k_svm_newton_begin"));
    int open = 0;
    HIP_TRY(hipMemcpyAsync(&open, b.flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (open == 0 || it >= max_iter) break;
    for (int c = 0; c < cg_max; ++c) {
      launch_svm_product(pl, 1, x, labels, row_fold, prob, b.st, b.d, b.z, b.xs, b.part, st);
      launch_svm_cg_step(pl, b.part, b.s, b.r, b.d, b.st, prob, cg_max, st);
    }
    TRY(launch_ok("k_svm_cg_step"));
    launch_svm_product(pl, 2, x, labels, row_fold, prob, b.st, b.s, b.z, b.xs, b.part, st);
    launch_svm_line_search(pl, b.z, b.xs, labels, row_fold, prob, b.st, b.lspart, w, b.s, b.g, st);
    TRY(launch_ok("k_svm_newton_end"));
  }
  // (a problem that the line search ended after the last status launch: its result is written here)
  launch_svm_status(pl, b.st, res, b.flag, st);
  TRY(launch_ok("k_svm_status"));
  HIP_TRY(hipStreamSynchronize(st));
  return NODE_OK;
}

}  // namespace

extern "C" {

size_t node_svm_workspace_bytes(int n, int d, int p) {
  if (check_sizes(n, d, p) != NODE_OK) return 0;
  return carve(svm_plan(n, d, chunk_size(n, d, p)), nullptr, nullptr);
}

int node_svm_fit(int n, int d, int p, const float* x, const int32_t* labels, const int32_t* row_fold,
                 const node_svm_problem* problems, double eps, int max_iter, float* weights, node_svm_result* results, void* ws,
                 size_t ws_bytes, void* stream) {
  TRY(check_sizes(n, d, p));
  if (!x || !labels || !row_fold || !problems || !weights || !results || !ws) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if (!(eps > 0.0) || !(eps < 1.0)) return fail(NODE_ERR_ARG, "svm eps=%g: eps must lie in (0, 1)", eps);
  if (max_iter < 0) return fail(NODE_ERR_ARG, "svm max_iter=%d: max_iter must be >= 0", max_iter);
  const int pc = chunk_size(n, d, p);
  const size_t need = carve(svm_plan(n, d, pc), nullptr, nullptr);
  if (ws_bytes < need) return fail(NODE_ERR_WORKSPACE, "svm workspace too small: %zu < %zu", ws_bytes, need);
  for (int c0 = 0; c0 < p; c0 += pc) {
    const int cnt = p - c0 < pc ? p - c0 : pc;
    TRY(fit_chunk(n, d, cnt, x, labels, row_fold, problems + c0, eps, max_iter, weights + (size_t)c0 * (d + 1), results + c0, ws,
                  (hipStream_t)stream));
  }
  return NODE_OK;
}

int node_svm_cv_score(int n, int d, int p, int n_groups, int k, const float* x, const int32_t* labels, const int32_t* row_fold,
                      const node_svm_problem* problems, const float* weights, const int32_t* group_problems, int neg_class,
                      int32_t* correct, int32_t* held, int32_t* pred, void* stream) {
  TRY(check_sizes(n, d, p));
  if (n_groups < 1 || k < 1) return fail(NODE_ERR_SHAPE, "svm score n_groups=%d k=%d: every size must be >= 1", n_groups, k);
  if (!x || !labels || !row_fold || !problems || !weights || !group_problems || !correct || !held)
    return fail(NODE_ERR_NULL, "a required pointer is NULL");
  launch_svm_cv_score(n, d, n_groups, k, x, labels, row_fold, problems, weights, group_problems, neg_class, correct, held, pred,
                      (hipStream_t)stream);
  return launch_ok("k_svm_cv_score");
}

}  // extern "C"
