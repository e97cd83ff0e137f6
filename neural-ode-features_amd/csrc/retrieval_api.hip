// C ABI of the retrieval evaluation (include/node_hip.h: node_retrieval_workspace_bytes / node_retrieval_ap / node_rank_ap):
// argument checks and the launch plan of kernels_retrieval.hip.  Reference: evaluate.py:308-361.
//
// node_retrieval_ap runs the queries in chunks of RET_CHUNK rows: scores of the chunk into the workspace, then its ranking.
// The workspace therefore holds min(nq, RET_CHUNK) x nd scores (<= 256 MiB), whatever the number of queries.
#include "host_common.h"

using namespace node;

namespace {

constexpr int RET_CHUNK = 4096;

int check_sizes(int nq, int nd, int d) {
  if (nq < 1 || nd < 1 || d < 1) return fail(NODE_ERR_SHAPE, "retrieval shape nq=%d nd=%d d=%d: every size must be >= 1", nq, nd, d);
  if (nd > RET_MAX_ND)
    return fail(NODE_ERR_UNSUPPORTED, "retrieval database of %d items: at most %d are supported (one row's sort keys in LDS)", nd,
                 RET_MAX_ND);
  return NODE_OK;
}

size_t score_bytes(int nq, int nd) {
  const size_t rows = nq < RET_CHUNK ? (size_t)nq : (size_t)RET_CHUNK;
  return (rows * (size_t)nd * sizeof(float) + 255) & ~(size_t)255;
}

int launch_ok(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
  return NODE_OK;
}

int check_rank_args(const int32_t* q_labels, const int32_t* x_labels, int k, const double* ap, const double* ap_k) {
  if (!q_labels || !x_labels || !ap || !ap_k) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if (k < 1) return fail(NODE_ERR_ARG, "retrieval k=%d: k must be >= 1", k);
  return NODE_OK;
}

}  // namespace

extern "C" {

size_t node_retrieval_workspace_bytes(int nq, int nd, int d) {
  if (check_sizes(nq, nd, d) != NODE_OK) return 0;
  return score_bytes(nq, nd);
}

int node_retrieval_ap(int nq, int nd, int d, const float* q, const float* x, const int32_t* q_labels, const int32_t* x_labels,
                      int k, double* ap, double* ap_k, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_sizes(nq, nd, d);
  if (rc != NODE_OK) return rc;
  if (!q || !x || !ws) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  rc = check_rank_args(q_labels, x_labels, k, ap, ap_k);
  if (rc != NODE_OK) return rc;
  if (ws_bytes < score_bytes(nq, nd))
    return fail(NODE_ERR_WORKSPACE, "retrieval workspace too small: %zu < %zu", ws_bytes, score_bytes(nq, nd));
  hipStream_t st = (hipStream_t)stream;
  float* scores = (float*)ws;
  for (int q0 = 0; q0 < nq; q0 += RET_CHUNK) {
    const int rows = nq - q0 < RET_CHUNK ? nq - q0 : RET_CHUNK;
    launch_retrieval_scores(q + (size_t)q0 * d, x, scores, rows, nd, d, st);
    if ((rc = launch_ok("k_ret_scores")) != NODE_OK) return rc;
    launch_retrieval_rank(scores, rows, nd, q_labels + q0, x_labels, k, ap + q0, ap_k + q0, st);
    if ((rc = launch_ok("k_ret_rank")) != NODE_OK) return rc;
  }
  return NODE_OK;
}

int node_rank_ap(int nq, int nd, const float* scores, const int32_t* q_labels, const int32_t* x_labels, int k, double* ap,
                 double* ap_k, void* ws, size_t ws_bytes, void* stream) {
  (void)ws;
  (void)ws_bytes;
  int rc = check_sizes(nq, nd, 1);
  if (rc != NODE_OK) return rc;
  if (!scores) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  rc = check_rank_args(q_labels, x_labels, k, ap, ap_k);
  if (rc != NODE_OK) return rc;
  launch_retrieval_rank(scores, nq, nd, q_labels, x_labels, k, ap, ap_k, (hipStream_t)stream);
  return launch_ok("k_ret_rank");
}

}  // extern "C"
