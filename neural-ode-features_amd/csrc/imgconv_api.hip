// C ABI of the image convolution in front of the ODE block (include/node_hip.h: node_imgconv_fwd / node_imgconv_bwd): argument
// checks and the launches of kernels_imgconv.hip.  Reference: model.py:119-126, 185, 203.  Every refusal happens before the
// first HIP call.
#include "host_common.h"

using namespace node;

namespace {

int check_imgconv_shape(const node_imgconv_shape* sh, ImgConvArgs* out) {
  if (!sh) return fail(NODE_ERR_NULL, "imgconv: shape is NULL");
  if (sh->n < 1) return fail(NODE_ERR_SHAPE, "imgconv shape n=%d: the batch must be >= 1", sh->n);
  if (sh->in_ch < 1 || sh->in_ch > 4) return fail(NODE_ERR_UNSUPPORTED, "imgconv in_ch=%d: 1 to 4 input channels are instantiated", sh->in_ch);
  if (sh->filters < 64 || sh->filters % 64 || sh->filters > 65536)      // grid.y of the forward, filters * (K + 1) as an int
    return fail(NODE_ERR_UNSUPPORTED, "imgconv filters=%d: the kernels take multiples of 64 up to 65536", sh->filters);
  if (sh->h < 4 || sh->w < 4 || (sh->h & 1) || (sh->w & 1))
    return fail(NODE_ERR_UNSUPPORTED, "imgconv image h=%d w=%d: even sides >= 4 are instantiated", sh->h, sh->w);
  const int64_t np = (int64_t)sh->n * (sh->h / 2) * (sh->w / 2);
  if (np > (1 << 29) || (int64_t)sh->n * sh->in_ch * sh->h * sh->w > (1ll << 31) - 1)
    return fail(NODE_ERR_UNSUPPORTED, "imgconv n=%d h=%d w=%d: more output pixels than the kernels index", sh->n, sh->h, sh->w);
  if (out) *out = ImgConvArgs{sh->n, sh->h, sh->w, sh->h / 2, sh->w / 2, sh->filters, (int)np};
  return NODE_OK;
}

size_t ws_bytes_of(const ImgConvArgs& a, int in_ch) {
  return (size_t)imgconv_slabs(a.np) * a.filters * (16 * in_ch + 1) * sizeof(float);
}

int launched(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
  return NODE_OK;
}

}  // namespace

extern "C" {

size_t node_imgconv_workspace_bytes(const node_imgconv_shape* shape) {
  ImgConvArgs a;
  if (check_imgconv_shape(shape, &a) != NODE_OK) return 0;
  return ws_bytes_of(a, shape->in_ch);
}

int node_imgconv_fwd(const node_imgconv_shape* shape, const float* x, const float* weight, const float* bias, float* y, void* stream) {
  ImgConvArgs a;
  TRY(check_imgconv_shape(shape, &a));
  if (!x || !weight || !y) return fail(NODE_ERR_NULL, "imgconv_fwd: x, weight and y are required");
  launch_imgconv_fwd(a, shape->in_ch, x, weight, bias, y, (hipStream_t)stream);
  return launched("k_imgconv_fwd");
}

int node_imgconv_bwd(const node_imgconv_shape* shape, const float* x, const float* weight, const float* grad_y, float* d_weight,
                     float* d_bias, float* d_x, void* ws, size_t ws_bytes, void* stream) {
  ImgConvArgs a;
  TRY(check_imgconv_shape(shape, &a));
  if (!x || !weight || !grad_y || !d_weight) return fail(NODE_ERR_NULL, "imgconv_bwd: x, weight, grad_y and d_weight are required");
  const size_t need = ws_bytes_of(a, shape->in_ch);
  if (!ws || ws_bytes < need) return fail(NODE_ERR_WORKSPACE, "imgconv_bwd: workspace too small (%zu < %zu bytes)", ws ? ws_bytes : (size_t)0, need);
  if (((uintptr_t)ws & 3) || ((uintptr_t)d_x & 7)) return fail(NODE_ERR_ARG, "imgconv_bwd: ws must be 4-byte and d_x 8-byte aligned");
  launch_imgconv_wgrad(a, shape->in_ch, x, grad_y, d_weight, d_bias, (float*)ws, (hipStream_t)stream);
  TRY(launched("k_imgconv_wgrad"));
  if (d_x) {
    launch_imgconv_dgrad(a, shape->in_ch, weight, grad_y, d_x, (hipStream_t)stream);
    TRY(launched("k_imgconv_dgrad"));
  }
  return NODE_OK;
}

}  // extern "C"
