// The theta-segment stage derivative as a launch of its own (theta_finalize.h has the body and what it computes).
#include "theta_finalize.h"

namespace node {

__global__ __launch_bounds__(256) void k_theta_finalize(ThetaFinalizeArgs a, Dims d) {
  if (a.ctrl->done) return;
  theta_finalize_body<256>(a, d, blockIdx.x, gridDim.x);
}

void launch_theta_finalize(const Dims& d, const ThetaFinalizeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_theta_finalize, dim3(theta_finalize_blocks(d, a)), dim3(256), 0, s, a, d);
}

}  // namespace node
