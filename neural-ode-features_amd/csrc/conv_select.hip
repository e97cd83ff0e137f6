// WHICH fp32 3x3 convolution kernel serves a geometry: Dims::wino (make_dims) names the family -- 0 the direct implicit GEMM
// (kernels_conv_direct.hip), 1 the 1-D Winograd F(2,3) kernel (kernels_conv_wino1d.hip), 2 the 2-D Winograd F(2x2,3x3) kernel
// (kernels_conv_wino2d.hip) -- and the launch, the LDS size and the packed-filter size all follow it here.  Within a family the M tile
// (Dims::BM) picks the instantiation; that stays with the kernel.  k_conv3x3_small (kernels_conv_small.hip) is the solver's choice
// (Dims::small), not this selector's.
#include "conv_common.h"

namespace node {

// tuning (tools/kbench.hip): forced M tile / kernel family, read by make_dims
int g_conv_bm = -1;
int g_conv_wino = -1;

// WHICH instance serves a geometry: a pure function of Dims.  node_describe_dims reports it; launch_conv and the families' launchers
// switch on it, so the description cannot drift from what is launched.
int conv_kernel_for(const Dims& d) {
  if (d.wino == 2) return NODE_CONV_W2_128;   // (make_dims admits the 2-D kernel at 128-row tiles only)
  if (d.wino) return d.BM == 64 ? NODE_CONV_W1_64 : d.BM == 128 ? NODE_CONV_W1_128 : NODE_CONV_W1_256;
  return d.BM == 64 ? NODE_CONV_DIRECT_64 : d.BM == 128 ? NODE_CONV_DIRECT_128 : NODE_CONV_DIRECT_256;
}

void launch_conv(const Dims& d, const ConvArgs& a, hipStream_t s) {
  const int k = conv_kernel_for(d);
  switch (k) {
    case NODE_CONV_W2_128: launch_conv_w2(d, a, s); return;
    case NODE_CONV_W1_64: case NODE_CONV_W1_128: case NODE_CONV_W1_256: launch_conv_w(d, a, k, s); return;
    default: launch_conv_direct(d, a, k, s); return;
  }
}

size_t conv_lds_bytes(const Dims& d, int /*mode*/) { return d.wino == 2 ? conv_w2_lds_bytes(d) : d.wino ? conv_w_lds_bytes(d) : conv_direct_lds_bytes(d); }

// packed-weight elements of one conv layer (forward or dgrad operand)
size_t conv_packed_elems(const Dims& d) {
  if (d.wino == 2) return (size_t)d.ntile * ((d.C + KCW - 1) / KCW) * (16 * BN * KCW);
  return d.wino ? (size_t)d.ntile * ((d.C + KCW - 1) / KCW) * 3 * (4 * BN * KCW) : (size_t)d.ntile * d.nchunk * 9 * (KCH * BN);
}

}  // namespace node
