// C ABI of the `ode` stem's hand-off (include/node_hip.h: node_pool_fwd / node_pool_bwd): argument checks and the launches of
// kernels_pool.hip.  Reference: model.py:181-196 (`ODEDownsample.maxpool`), model.py:36 (the trajectory's plane means).  Every
// refusal happens before the first HIP call; one launch per call.
#include "host_common.h"

using namespace node;

namespace {

int check_pool_shape(const node_pool_shape* sh, PoolArgs* out) {
  if (!sh) return fail(NODE_ERR_NULL, "pool: shape is NULL");
  if (sh->t < 1 || sh->n < 1 || sh->c < 1)
    return fail(NODE_ERR_UNSUPPORTED, "pool shape t=%d n=%d c=%d: slices, batch and channels must be >= 1", sh->t, sh->n, sh->c);
  if (sh->h < 2 || sh->w < 2 || sh->h > 32768 || sh->w > 32768)      // h w and every index inside a plane stay an int
    return fail(NODE_ERR_UNSUPPORTED, "pool plane h=%d w=%d: a 4x4 stride-2 padding-1 window takes sides from 2 to 32768", sh->h, sh->w);
  const int64_t planes = (int64_t)sh->n * sh->c;
  if (planes * sh->t > ((int64_t)1 << 40) / ((int64_t)sh->h * sh->w))
    return fail(NODE_ERR_UNSUPPORTED, "pool t=%d n=%d c=%d h=%d w=%d: more than 2^40 elements", sh->t, sh->n, sh->c, sh->h, sh->w);
  if (out) *out = PoolArgs{sh->t, sh->h, sh->w, (sh->h - 2) / 2 + 1, (sh->w - 2) / 2 + 1, planes};
  return NODE_OK;
}

int launched(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
  return NODE_OK;
}

}  // namespace

extern "C" {

int node_pool_fwd(const node_pool_shape* shape, const float* x, float* pooled, uint8_t* argmax, float* means, void* stream) {
  PoolArgs a;
  TRY(check_pool_shape(shape, &a));
  if (!x || !pooled) return fail(NODE_ERR_NULL, "pool_fwd: x and pooled are required");
  if (((uintptr_t)x | (uintptr_t)pooled | (uintptr_t)means) & 3) return fail(NODE_ERR_ARG, "pool_fwd: x, pooled and means must be 4-byte aligned");
  // float4 rows, float2 / uchar2 output pairs: W % 4 == 0 makes every plane and row of x a multiple of 16 bytes and OW even
  const bool vec = a.w % 4 == 0 && !((uintptr_t)x & 15) && !((uintptr_t)pooled & 7) && !((uintptr_t)argmax & 1);
  launch_pool_fwd(a, vec, x, pooled, argmax, means, (hipStream_t)stream);
  return launched("k_pool_fwd");
}

int node_pool_bwd(const node_pool_shape* shape, const float* grad_y, const uint8_t* argmax, float* d_x, void* stream) {
  PoolArgs a;
  TRY(check_pool_shape(shape, &a));
  if (!grad_y || !argmax || !d_x) return fail(NODE_ERR_NULL, "pool_bwd: grad_y, argmax and d_x are required");
  if (((uintptr_t)grad_y | (uintptr_t)d_x) & 3) return fail(NODE_ERR_ARG, "pool_bwd: grad_y and d_x must be 4-byte aligned");
  const bool vec = a.w % 4 == 0 && !((uintptr_t)d_x & 15);
  launch_pool_bwd(a, vec, grad_y, argmax, d_x, (hipStream_t)stream);
  return launched("k_pool_bwd");
}

}  // extern "C"
