// BatchNorm (batch statistics, no running buffers: nn.BatchNorm2d(C, track_running_stats=False), model.py:274) over an NHWC
// tensor [rows = N H W][C] for the stem's kernel family, and the time channel of ConcatConv2d (model.py:313-323) for its
// gather GEMMs: internal declarations shared by kernels_batchnorm.hip (kernels + launchers) and bnfunc_api.hip (the C ABI).
#pragma once
#include "stem.h"

namespace node {

// A BatchNorm pass works on (chunk of rows) x (64 channels) per workgroup; statistics are taken in two stages: every
// workgroup writes its chunk's partials, every CONSUMER combines the partials of its 64 channels in one fixed order.
//
// The normalised tensor is  u = h + t * T[class(pixel)][c]  when T is given: h is what the gather GEMM wrote (filter
// w[:, 1:], bias in its epilogue), and the time channel of ConcatConv2d -- a constant plane t in front of a zero-padded
// 3x3 filter -- is the additive term t * (sum of w[co, 0, ky, kx] over the taps inside the image): nine values per output
// channel, class = 3 * (top, middle, bottom row) + (left, middle, right column).  Every pass that reads h adds it on the
// fly, so the term costs no pass over the tensor.  t is a DEVICE scalar.
struct SBnArgs {
  const float* h;          // fp32 NHWC [rows][C]
  const float* T;          // nullable [9][C]
  const float* t;          // device scalar (read only with T)
  const float* gamma;
  const float* beta;
  float* part;             // forward [nchunk][2][C]: (chunk mean, centred second moment)
  float* stats;            // [2][C]: batch mean, 1 / sqrt(biased variance + eps): written by the apply pass, read by the backward
  int rows, C, H, W;
  int chunk_rows, nchunk;  // chunk_rows % 32 == 0
  int relu;
  float eps;
  // apply: y = [relu](xhat gamma + beta) as triples and / or fp32 NHWC
  bf16_t* a3;
  size_t a_plane;
  float* y;
  // backward: da = dL/dy
  const float* da;
  double* gpart;           // [nchunk][2][C]: (sum dy, sum dy xhat) of the chunk, fp64 (kernels_batchnorm.hip says why)
  float* dh;               // nullable fp32 NHWC gradient of u
  bf16_t* dh3;             // nullable triples of the same
  size_t dh_plane;
  float* dgamma;           // nullable [C] (written by the chunk-0 workgroups of the dx pass)
  float* dbeta;
  float* clsp;             // nullable [nchunk][9][C]: per-chunk sums of the gradient of u over the pixels of each class
  double* dtp;             // with clsp: [nchunk][C / 64], the workgroup's share of sum du * (T - T[interior]) (fp64: the sum cancels heavily)
  // multipliers of a solve's driver (bnsolve_api.hip); 1.0f, the default, is exact.  The gradient is linear in the cotangent, so a
  // sign on `da` of the FIRST backward pass of an evaluation reaches every gradient it returns.
  float out_scale = 1.0f;  // on the fp32 output `y` of the apply pass (the triples are not scaled)
  float da_scale = 1.0f;   // on every read of `da` in the two backward passes
  // the residual trunk (bntrunk_api.hip): h also is the block's shortcut, so its gradient is du + skip.  Not with clsp.
  const float* skip = nullptr;   // nullable fp32 NHWC, added to du before the fp32 store and the triple split (dx pass only)
  // slices (bndownconv_api.hip; the two forward passes only): rows = slices * rows_per_slice, statistics per (slice, channel).  Chunks
  // never straddle a slice: nchunk = slices * chunks_per_slice, chunk slice * chunks_per_slice + k starts at row slice * rows_per_slice +
  // k * chunk_rows (any row: not a multiple of 32 or of chunk_rows in general), the last chunk of every slice may be short; part stays
  // [nchunk][2][C], stats becomes [slices][2][C].  With chunk_rows what one slice alone would take, every slice has the bits of its
  // own unsliced call.  0 or 1: the unsliced passes, which read neither of the other two.
  int slices = 1;
  int rows_per_slice = 0;
  int chunks_per_slice = 0;
};
// rows per chunk for a tensor of `rows` x C: <= 128 chunks, enough (chunk, channel block) pairs to cover the device
int bn_chunk_rows(int rows, int C);
// the same for a tensor of the stems (bnstem_api.hip): at most NODE_TUNE_BNSTEM_MAXCHUNK chunks at C = 64 (unset or 0: 128, at which
// it is bn_chunk_rows)
int bnstem_chunk_rows(int rows, int C);
void launch_bn_stats(const SBnArgs& a, hipStream_t s);
void launch_bn_apply(const SBnArgs& a, hipStream_t s);
void launch_bn_bwd_stats(const SBnArgs& a, hipStream_t s);
void launch_bn_bwd_dx(const SBnArgs& a, hipStream_t s);

// once per forward: the x part w[:, 1:] of both ConcatConv2d filters [C][C + 1][3][3] -> triples in both operand layouts
// (as k_stem_prep does for a contiguous filter), the time tables T[9][C], the zero rows of `nzero` triples tensors
struct SBnPrepArgs {
  const float* w[2];
  bf16_t* wf[2];
  bf16_t* wd[2];
  float* T[2];
  int C;
  bf16_t* zero[3]; size_t zero_plane[3]; int nzero;
};
void launch_bn_prep(const SBnPrepArgs& a, hipStream_t s);

// once per backward: split-K slabs [ns][9][C][C] -> dW[:, 1:] of the [C][C + 1][3][3] filters; the class sums -> dW[:, 0],
// the bias gradients, and d_t = sum over both convolutions of du * T (fixed order; device scalar)
struct SBnReduceArgs {
  const float* slab0; const float* slab1;
  int ns0, ns1;
  float* dw0; float* dw1;
  float* db0; float* db1;
  const float* clsp0; const float* clsp1;
  const double* dtp0; const double* dtp1;
  int nchunk, C;
  const float* t;
  float* d_t;              // nullable
  int want_params;
};
void launch_bn_reduce(const SBnReduceArgs& a, hipStream_t s);

// The classifier head of a `norm='batch'` net (kernels_bnhead.hip): pooled[n][c] = scale[n][c] * mean_px relu(BatchNorm(z)) on the
// NCHW tensor z [N][C][HW] as the net's body leaves it.  A workgroup = (channel, chunk of S samples), a wave = one (n, c) plane
// at a time (HW contiguous floats: whole cache lines).  Two launches each way, statistics in the two stages of the passes above.
constexpr int BNHEAD_MAX_CHUNKS = 32;
struct SBnHeadArgs {
  const float* z;          // fp32 NCHW [N][C][HW]
  const float* gamma;
  const float* beta;
  const float* scale;      // nullable [N][C]: the dropout mask / (1 - p)
  float* pooled;           // [N][C]
  float* stats;            // [2][C]: batch mean, 1 / sqrt(biased variance + eps): written by the apply pass, read by the backward
  float* part;             // forward [nchunk][2][C]: (chunk mean, centred second moment)
  const float* g_pooled;   // backward [N][C]
  float* dz;               // backward [N][C][HW]
  double* gpart;           // backward [nchunk][2][C]: (sum dy, sum dy xhat) of the chunk, fp64
  float* dgamma;           // [C] (written by the chunk-0 workgroups of the dx pass)
  float* dbeta;
  int N, C, HW;
  int chunk_samples, nchunk;   // nchunk <= BNHEAD_MAX_CHUNKS
  float eps;
};
int bnhead_chunk_samples(int N, int C);      // samples per chunk: <= BNHEAD_MAX_CHUNKS chunks, about 2048 workgroups at most
void launch_bnhead_stats(const SBnHeadArgs& a, hipStream_t s);
void launch_bnhead_apply(const SBnHeadArgs& a, hipStream_t s);
// the two forward passes for `slices` tensors [N][C][HW] behind one another, statistics per slice (a.scale unused: forward only)
void launch_bnhead_stats_slices(const SBnHeadArgs& a, int slices, hipStream_t s);
void launch_bnhead_apply_slices(const SBnHeadArgs& a, int slices, hipStream_t s);
void launch_bnhead_bwd_stats(const SBnHeadArgs& a, hipStream_t s);
void launch_bnhead_bwd_dx(const SBnHeadArgs& a, hipStream_t s);

// The small passes of a whole solve around these dynamics (bnsolve_api.hip); n % 4 == 0, 16-byte aligned tensors.
// *out = sum a[i] * b[i]: two launches, fp64 partials [BN_DOT_BLOCKS] in a fixed order
constexpr int BN_DOT_BLOCKS = 128;
void launch_bn_dot(const float* a, const float* b, size_t n, double* part, float* out, hipStream_t s);
void launch_bn_add(float* y, const float* x, size_t n, hipStream_t s);      // y += x
void launch_bn_set_scalar(float* dst, float v, hipStream_t s);               // *dst = v (a device scalar: the time of an evaluation)

}  // namespace node
