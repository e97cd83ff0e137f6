// C ABI of the `norm='batch'` classifier head (include/node_hip.h: node_bnhead_fwd / node_bnhead_bwd) on the kernels of
// kernels_bnhead.hip: two launches each way, no workspace beyond the caller's scratch for the statistics' partials.
#include "host_common.h"
#include "batchnorm.h"
#include "stem_plan.h"
#include <cstring>

using namespace node;

namespace {

int check_head_shape(const node_bnfunc_shape* sh) {
  if (!sh) return fail(NODE_ERR_NULL, "shape is NULL");
  if (sh->n <= 0 || sh->h <= 0 || sh->w <= 0 || sh->channels <= 0) return fail(NODE_ERR_SHAPE, "bad bnhead shape");
  const int C = sh->channels;
  if (C < 64 || C % 64 != 0 || C > 4096)
    return fail(NODE_ERR_UNSUPPORTED, "the batch-norm head takes channels a multiple of 64 in [64, 4096], as the batch-norm trunk and "
                 "dynamics in front of it (got %d)", C);
  const size_t elems = (size_t)sh->n * sh->h * sh->w * C;
  if (elems >= ((size_t)1 << 31)) return fail(NODE_ERR_UNSUPPORTED, "bnhead tensors must stay under 2^31 elements");
  return NODE_OK;
}

SBnHeadArgs head_args(const node_bnfunc_shape* sh, const float* z, const float* gamma, const float* beta, const float* scale, float* stats) {
  SBnHeadArgs a;
  memset(&a, 0, sizeof(a));
  a.z = z; a.gamma = gamma; a.beta = beta; a.scale = scale; a.stats = stats;
  a.N = sh->n; a.C = sh->channels; a.HW = sh->h * sh->w; a.eps = sh->eps;
  a.chunk_samples = bnhead_chunk_samples(a.N, a.C);
  a.nchunk = (a.N + a.chunk_samples - 1) / a.chunk_samples;
  return a;
}

int check_f32(const void* p, const char* what, bool required) {
  if (!p) return required ? fail(NODE_ERR_NULL, "%s is NULL", what) : NODE_OK;
  if (((uintptr_t)p) & 3) return fail(NODE_ERR_ARG, "%s must be 4-byte aligned", what);
  return NODE_OK;
}

}  // namespace

extern "C" {

size_t node_bnhead_scratch_bytes(const node_bnfunc_shape* shape) {
  if (check_head_shape(shape) != NODE_OK) return 0;
  const SBnHeadArgs a = head_args(shape, nullptr, nullptr, nullptr, nullptr, nullptr);
  return (size_t)a.nchunk * 2 * a.C * sizeof(double);
}

int node_bnhead_fwd(const node_bnfunc_shape* shape, const float* z, const float* gamma, const float* beta, const float* scale,
                    float* pooled, float* stats, void* scratch, void* stream) {
  int rc = check_head_shape(shape);
  if (rc != NODE_OK) return rc;
  if ((rc = check_f32(z, "z", true)) != NODE_OK || (rc = check_f32(gamma, "gamma", true)) != NODE_OK ||
      (rc = check_f32(beta, "beta", true)) != NODE_OK || (rc = check_f32(scale, "scale", false)) != NODE_OK ||
      (rc = check_f32(pooled, "pooled", true)) != NODE_OK || (rc = check_f32(stats, "stats", true)) != NODE_OK)
    return rc;
  if (!scratch) return fail(NODE_ERR_NULL, "scratch is NULL");
  if (((uintptr_t)scratch) & 7) return fail(NODE_ERR_ARG, "scratch must be 8-byte aligned");
  SBnHeadArgs a = head_args(shape, z, gamma, beta, scale, stats);
  a.pooled = pooled; a.part = static_cast<float*>(scratch);
  hipStream_t st = (hipStream_t)stream;
  launch_bnhead_stats(a, st);
  if ((rc = launch_ok("bnhead_stats")) != NODE_OK) return rc;
  launch_bnhead_apply(a, st);
  return launch_ok("bnhead_apply");
}

size_t node_bnhead_slices_scratch_bytes(const node_bnfunc_shape* shape, int slices) {
  if (check_head_shape(shape) != NODE_OK) return 0;
  if (slices <= 0 || slices > 65535) { fail(NODE_ERR_UNSUPPORTED, "the sliced batch-norm head takes 1 to 65535 slices (got %d)", slices); return 0; }
  return (size_t)slices * node_bnhead_scratch_bytes(shape);
}

int node_bnhead_fwd_slices(const node_bnfunc_shape* shape, int slices, const float* z, const float* gamma, const float* beta,
                           float* pooled, float* stats, void* scratch, void* stream) {
  int rc = check_head_shape(shape);
  if (rc != NODE_OK) return rc;
  if (slices <= 0 || slices > 65535) return fail(NODE_ERR_UNSUPPORTED, "the sliced batch-norm head takes 1 to 65535 slices (got %d)", slices);
  if ((rc = check_f32(z, "z", true)) != NODE_OK || (rc = check_f32(gamma, "gamma", true)) != NODE_OK ||
      (rc = check_f32(beta, "beta", true)) != NODE_OK || (rc = check_f32(pooled, "pooled", true)) != NODE_OK ||
      (rc = check_f32(stats, "stats", true)) != NODE_OK)
    return rc;
  if (!scratch) return fail(NODE_ERR_NULL, "scratch is NULL");
  if (((uintptr_t)scratch) & 7) return fail(NODE_ERR_ARG, "scratch must be 8-byte aligned");
  // (the shape is a SLICE's: head_args picks the chunking node_bnhead_fwd picks for it; a slice's partials take the
  //  nchunk * 2 * C floats at the head of its node_bnhead_scratch_bytes share)
  SBnHeadArgs a = head_args(shape, z, gamma, beta, nullptr, stats);
  a.pooled = pooled; a.part = static_cast<float*>(scratch);
  hipStream_t st = (hipStream_t)stream;
  launch_bnhead_stats_slices(a, slices, st);
  if ((rc = launch_ok("bnhead_stats_slices")) != NODE_OK) return rc;
  launch_bnhead_apply_slices(a, slices, st);
  return launch_ok("bnhead_apply_slices");
}

int node_bnhead_bwd(const node_bnfunc_shape* shape, const float* z, const float* gamma, const float* beta, const float* scale,
                    const float* stats, const float* g_pooled, float* dz, float* dgamma, float* dbeta, void* scratch, void* stream) {
  int rc = check_head_shape(shape);
  if (rc != NODE_OK) return rc;
  if ((rc = check_f32(z, "z", true)) != NODE_OK || (rc = check_f32(gamma, "gamma", true)) != NODE_OK ||
      (rc = check_f32(beta, "beta", true)) != NODE_OK || (rc = check_f32(scale, "scale", false)) != NODE_OK ||
      (rc = check_f32(stats, "stats", true)) != NODE_OK || (rc = check_f32(g_pooled, "g_pooled", true)) != NODE_OK ||
      (rc = check_f32(dz, "dz", true)) != NODE_OK || (rc = check_f32(dgamma, "dgamma", true)) != NODE_OK ||
      (rc = check_f32(dbeta, "dbeta", true)) != NODE_OK)
    return rc;
  if (!scratch) return fail(NODE_ERR_NULL, "scratch is NULL");
  if (((uintptr_t)scratch) & 7) return fail(NODE_ERR_ARG, "scratch must be 8-byte aligned");
  SBnHeadArgs a = head_args(shape, z, gamma, beta, scale, const_cast<float*>(stats));
  a.g_pooled = g_pooled; a.dz = dz; a.dgamma = dgamma; a.dbeta = dbeta; a.gpart = static_cast<double*>(scratch);
  hipStream_t st = (hipStream_t)stream;
  launch_bnhead_bwd_stats(a, st);
  if ((rc = launch_ok("bnhead_bwd_stats")) != NODE_OK) return rc;
  launch_bnhead_bwd_dx(a, st);
  return launch_ok("bnhead_bwd_dx");
}

}  // extern "C"
