// The `minimal` stem with norm = 'batch' (model.py:129-145 with model.py:274: nn.BatchNorm2d(24, track_running_stats=False) in the
// two norm slots): the BatchNorm + ReLU passes on the stem's fp32 NHWC tensors [rows = N H W][24] of channel pitch 24.  Internal
// declarations shared by kernels_bnministem.hip (kernels + launchers) and bnministem_api.hip (the C ABI); the convolutions are
// ministem.h's, used as they are.
//
// The conventions are batchnorm.h's: statistics in two stages (every workgroup writes its chunk's mean and centred second moment,
// every consumer combines the partials of its channels by Chan's formula in one fixed order), the backward's sums in two stages
// with fp64 partials, no atomics, the same bits run to run.  What differs is the shape of a workgroup: a pixel is 96 bytes = six
// 16-byte channel quads, so a workgroup is 192 threads = 32 rows x 6 quads (BNMINI_TRIP rows per trip of its loop) over ALL 24
// channels of a chunk of rows, and consecutive threads read consecutive 16-byte words: every trip is one contiguous 3 KB piece.
#pragma once
#include "ministem.h"

namespace node {

constexpr int BNMINI_TRIP = 32;                      // rows a workgroup covers per trip of its loop
constexpr int BNMINI_THREADS = BNMINI_TRIP * 6;      // one thread per (row of the trip, channel quad)
constexpr int BNMINI_MAX_CHUNKS = 128;             // the default cap on the chunks of a pass (NODE_TUNE_BNMINI_MAXCHUNK: another, to measure)

struct BnMiniArgs {
  const float* h;          // fp32 NHWC [rows][24]: the convolution's output (bias included)
  const float* gamma;
  const float* beta;
  float* part;             // forward [nchunk][2][24]: (chunk mean, centred second moment)
  float* stats;            // [2][24]: batch mean, 1 / sqrt(biased variance + eps): written by the apply pass, read by the backward
  float* a;                // apply: relu(xhat gamma + beta), fp32 NHWC [rows][24]
  int rows;
  int chunk_rows, nchunk;  // chunk_rows % BNMINI_TRIP == 0, nchunk <= the cap in force
  float eps;
  // backward
  float* d;                // in: the activation's gradient; out (dx pass, in place): the gradient of h
  double* gpart;           // [nchunk][2][24]: (sum dy, sum dy xhat) of the chunk, fp64 (kernels_batchnorm.hip says why)
  float* dgamma;           // nullable [24] (written by the chunk-0 workgroup of the dx pass)
  float* dbeta;
  float* bpart;            // nullable [nchunk][24]: the chunk's column sums of the gradient of h (the bias gradient of the convolution
                           // in front: zero up to rounding)
};
// rows per chunk for a tensor of `rows` x 24: a multiple of BNMINI_TRIP, at most BNMINI_MAX_CHUNKS chunks (or the cap of the environment)
int bnmini_chunk_rows(int rows);
void launch_bnmini_stats(const BnMiniArgs& a, hipStream_t s);
void launch_bnmini_apply(const BnMiniArgs& a, hipStream_t s);
void launch_bnmini_bwd_stats(const BnMiniArgs& a, hipStream_t s);
void launch_bnmini_bwd_dx(const BnMiniArgs& a, hipStream_t s);

}  // namespace node
