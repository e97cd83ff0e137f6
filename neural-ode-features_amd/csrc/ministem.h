// The `minimal` stem (model.py:129-145, `MinimalConvDownsample`) as gfx950 kernels: internal declarations shared by
// kernels_ministem.hip (kernels + launchers) and ministem_api.hip (the C ABI entry points).
//
//     Conv2d(in_ch, 24, 3, 1) | GroupNorm(24, 24) + ReLU | Conv2d(24, 24, 4, 2, 1) | GroupNorm(24, 24) + ReLU | Conv2d(24, filters, 4, 2, 1)
//
// 24 channels: the work is small (under 2 GFLOP at [128, 3, 32, 32] -> 256) and bound by traffic and launches, so the kernels
// are register-tiled fp32 FMA loops -- exact fp32 products, no operand conversion, no 64-column tiles to pad to -- on NHWC
// fp32 tensors of channel pitch 24 (96 bytes a pixel: six 16-byte loads).  GroupNorm(24, 24) has groups of ONE channel: its
// statistics are per (sample, channel) plane, and one workgroup per (sample, four channels) holds every reduction of a plane in a
// fixed order.
// Nothing is accumulated with atomics.
#pragma once
#include "node_internal.h"

namespace node {

constexpr int MINI_C = 24;          // the stem's middle channel count, and the channel pitch inside the workspace
constexpr int MINI_COB = 32;        // output channels per block of the 4x4 weight gradient (a register tile per thread) and data gradient (an LDS block)
constexpr int MINI_FCO = 8;         // output channels per thread of the forward 4x4 convolution

// where element (sample n, channel c, pixel p) of a 4x4 convolution's output gradient lies: n * sn + c * sc + p * sp
// (the caller's NCHW cotangent: sn = C HW, sc = HW, sp = 1;  NHWC of pitch 24 in the workspace: sn = 24 HW, sc = 1, sp = 24)
struct MiniDy {
  const float* p;
  long long sn;
  int sc, sp;
};

// first layer.  x NCHW [N][Cin][H][W]; w0 [24][Cin][3][3]; h0 NHWC [N][(H - 2)(W - 2)][24]
void launch_mini_conv0_fwd(const float* x, const float* w0, const float* b0, float* h0, int N, int Cin, int H, int W, hipStream_t s);
// GroupNorm(24, 24) + ReLU of an NHWC plane set, a = relu(GN(h)): one workgroup per (sample, four channels); stats [N][24][2]
// (mean, 1 / sigma)
void launch_mini_gn_fwd(const float* h, const float* gamma, const float* beta, float* a, float* stats, int N, int HW, float eps, hipStream_t s);
// Conv2d(24, Cout, 4, 2, 1) with bias.  in: NHWC [N][IH IW][24]; w: [Cout][24][4][4]; out: NHWC of pitch 24 (nchw = 0, Cout = 24)
// or NCHW [N][Cout][OH OW] (nchw = 1)
void launch_mini_conv4_fwd(const float* in, const float* w, const float* bias, float* out, int N, int IH, int IW, int OH, int OW, int Cout,
                           int nchw, hipStream_t s);
// its data gradient: d_in NHWC [N][IH IW][24] (every element written) from dy [N][Cout][OH OW]
void launch_mini_conv4_dgrad(MiniDy dy, const float* w, float* d_in, int N, int IH, int IW, int OH, int OW, int Cout, hipStream_t s);
// its weight gradient as split-K slabs [nsplit][Cout][24][16] (PyTorch's filter layout per slab); rows_per_split rows of dy each
void launch_mini_conv4_wgrad(MiniDy dy, const float* in, float* slab, int N, int IH, int IW, int OH, int OW, int Cout, int nsplit,
                             int rows_per_split, hipStream_t s);
// GroupNorm(24, 24) + ReLU backward, in place: d holds the activation's gradient and receives the gradient of h.
// gpart [N][2][24]: per-sample (dgamma, dbeta); bpart [N][24]: per-sample sums of the gradient of h (the bias gradient of the
// convolution in front: zero up to rounding, with one channel per group)
void launch_mini_gn_bwd(const float* h, const float* a, const float* gamma, const float* stats, float* d, float* gpart, float* bpart,
                        int N, int HW, hipStream_t s);
// first layer's weight gradient per sample (one workgroup per kernel row): slab [N][24][9 Cin]
void launch_mini_conv0_wgrad(const float* x, const float* dh0, float* slab, int N, int Cin, int H, int W, hipStream_t s);
// the transposed first layer: dx NCHW [N][Cin][H][W] (every element written)
void launch_mini_conv0_dgrad(const float* dh0, const float* w0, float* dx, int N, int Cin, int H, int W, hipStream_t s);
// per-channel sums of an NCHW tensor: db [C] = sum over (n, p) of g[n][c][p]
void launch_mini_chansum(const float* g, float* db, int N, int C, int HW, hipStream_t s);
// out[i] = sum over s < ns of src[s * stride + i], i < count, s ascending
struct MiniSumJob { const float* src; float* out; int ns; long long stride; int count; };
struct MiniSumArgs { MiniSumJob job[9]; int njobs; };
void launch_mini_sums(const MiniSumArgs& a, hipStream_t s);

}  // namespace node
