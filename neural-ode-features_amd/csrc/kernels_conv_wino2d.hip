// ============================================================================
// k_conv3x3_w2 -- 2-D Winograd F(2x2, 3x3): each 2x2 output tile comes from a 4x4 input patch through
// sixteen component products instead of 36 multiplies per channel pair (2.25 x fewer MFMAs than the
// direct kernel, 1.5 x fewer than k_conv3x3_w):
//     V = B^T d B  (4x4, at staging time)    U = G g G^T  (4x4, once per solve: k_pack_weights_w2)
//     M_c[tile, co] = sum_ci V_c[tile, ci] * U_c[ci, co],  c = (xi, nu)           (MFMA, K = channels only)
//     Y = A^T M A  (2x2, in the epilogue)
// Workgroup = 32 tiles (128 pixels = whole samples) x 64 output channels x 16 components; wave w owns
// components 2w, 2w+1 for both column halves (four accumulators).  No two waves share a filter
// operand, so U never touches LDS: two pieces ahead it goes from L2 straight into registers (eight
// float4 per lane and K chunk).  The A image [tile][component][16 channels] is triple-buffered in LDS,
// which leaves ONE barrier per K chunk of 32 MFMAs per wave.  The 4x4 input transform is split over
// the four lanes of a quad: each lane loads one patch row, transforms it along x, and gets the one other
// row it needs for the transform along y through a DPP quad permute.  The epilogue folds the sixteen
// component tiles in two rounds (eight at a time through LDS) and then runs the shared tail.
// Requires even H and W and 128-pixel tiles; other geometries use k_conv3x3_w / k_conv3x3.
// ============================================================================
#include <hip/hip_runtime.h>

namespace node {
// This file instantiates conv_epilogue_tail once, so masked_colsum_tile has ONE call site here; the compiler then specialises that
// local function for its caller and forms the tap strides of the column sums differently than in the files with three tails.  `used`
// keeps the function externally visible, which gives k_conv3x3_w2 the instruction stream it had in kernels_conv.hip, bit for bit
// (profiles/conv_pointwise_split_equiv.txt, section 2).  Costs one unreferenced device function; DESIGN 9 lists dropping it.
// The declaration must stay IN FRONT OF every project include: behind the definition (node_internal.h) the attribute is ignored, the
// file still compiles, and k_conv3x3_w2 silently goes back to the 3 784-instruction stream.
__attribute__((used)) __device__ void masked_colsum_tile(const float* tile, int ld, int HW, const unsigned char* flg, int ncols, int ngrp,
                                                         int tid, float* red, float* out, int out_ld);
}  // namespace node

#include "conv_common.h"
#include <cstring>

namespace node {

constexpr int SST2 = 16 * ASTW + 4;   // floats per tile of the A image: 16 components x 20, + 4: 81 16-B units (odd)

__global__ __launch_bounds__(512) void k_conv3x3_w2(ConvArgs a, Dims d) {
  if (a.et.ctrl != nullptr && a.et.ctrl->done) return;   // a step enqueued past the end of the interval (Ctrl::done)

  PSTAMP(a.stamps, 0, "s_memrealtime");
  PSTAMP(a.stamps, 1, "s_memtime");
  constexpr int THREADS = 512;
  constexpr int TT = 32;             // tiles per workgroup
  constexpr int BM = 128;            // pixels per workgroup
  constexpr int ABUF = TT * SST2;
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  // XCD-aware tile order (speed-neutral, traffic only): blocks b and b + 8 share an XCD and its 4 MB L2.  In launch
  // order an XCD sees every column tile, i.e. the whole packed filter (4.2 MB at C = 256: 8 copies = 33.6 MB of
  // the 50.9 MB this kernel fetched per launch); giving each XCD two column tiles x a quarter of the pixel tiles
  // fetches the filter 4 x and the activations 2 x instead: the minimum over such partitions.
  int mtile = blockIdx.x, nt = blockIdx.y;
  {
    const int gx = gridDim.x, gy = gridDim.y, L = blockIdx.x + gx * blockIdx.y;
    if (gy == 4 && (gx & 3) == 0) {
      const int xcd = L & 7, slot = L >> 3;      // slot 0 .. gx/2 - 1
      nt = (xcd & 1) * 2 + (slot & 1);
      mtile = (xcd >> 1) * (gx >> 2) + (slot >> 1);
    }
  }
  // whole samples per tile, or (Dims::csplit workgroups per sample, images larger than 128 pixels) one 32-tile
  // band of ONE sample: whole tile rows, 128 consecutive pixels; GroupNorm is then a separate pointwise pass and
  // this kernel stores its raw tile
  const int csp = d.csplit;
  const int n0 = csp ? mtile / csp : mtile * d.S;
  const int band = csp ? mtile - n0 * csp : 0;
  const int c0 = nt * d.BNE;
  const int nsamp = csp ? 1 : min(d.S, d.N - n0);
  const int TW = d.W >> 1, TH = d.H >> 1;
  const int TPS = TH * TW;           // tiles per sample
  const int tiles_valid = csp ? TT : nsamp * TPS;
  const bool fwd = a.mode != CM_BWD_RELU_GN;
  const int ncols = min(d.BNE, d.C - c0);

  float* Abuf = smem;                // 3 x ABUF: chunk c in buffer c % 3
  // the tables sit behind BOTH the activation buffers and the epilogue's transform region: the first waves out
  // of the main loop write that region while the last ones still read the tables
  const int epi_end = 2 * BM * CT2 + 2 * d.S * BN + 32 * 64 * 2 + 8 * TT * CT2;
  int* ptab = reinterpret_cast<int*>(smem + max(3 * ABUF, epi_end));   // [TT] pixel row (in the tile) of output pixel (2 th, 2 tw), -1 if none
  int* qtab = ptab + TT;                                  // [TT] the same pixel's index inside its sample
  if (tid < TT) {
    int pr = -1, q = 0;
    if (csp) {
      const int thl = tid / TW, tw = tid - thl * TW;
      pr = (2 * thl) * d.W + 2 * tw;
      q = band * BM + pr;
    } else if (tid < d.S * TPS) {
      const int s = tid / TPS, rem = tid - s * TPS;
      const int th = rem / TW, tw = rem - th * TW;
      q = (2 * th) * d.W + 2 * tw;
      pr = s * d.HW + q;
    }
    ptab[tid] = pr;
    qtab[tid] = q;
  }

  // ---- staging descriptor: thread = (tile, channel quad, patch row r).  The four patch pixels are fetched with
  //      global loads "scalar base + 32-bit lane offset": the base (workgroup's first sample + chunk) moves on
  //      the scalar unit, the lane offsets are fixed for the whole kernel, and a pixel outside the image (or a
  //      tile past the batch) points at the row of C zeros the host keeps behind the tensor -- so the requests
  //      are branch-free (exact vmcnt bookkeeping; with exec-masked loads the compiler waited for the youngest
  //      request at every use) and cost no VALU per chunk.  Range-checked buffer loads did the same but issued
  //      ~100 cycles slower each (measured). ----
  const int sr = tid & 3, sq4 = (tid >> 2) & 3, stile = tid >> 4;
  // component (xi = sr, nu = 0).  ds_write_b128 is serviced in groups of 8 contiguous lanes with banks (a/4) % 32:
  // the four patch rows of a quad sit 80 floats apart (= 16 banks), so rows 0/2 and 1/3 collided (2-way, measured
  // as 31 % of all LDS cycles); the channel quad of rows 2 and 3 is stored at position sq4 ^ 2 instead, and the
  // readers of those components (xi = 2, 3) swap their lane halves to match.
  const int slofs = stile * SST2 + (sr * 4) * ASTW + ((sq4 ^ (sr & 2)) * 4);
  const float* abase = a.in + (size_t)n0 * d.HW * d.C;
  const unsigned zoff = (unsigned)(((size_t)(d.N - n0) * d.HW * d.C + sq4 * 4) * sizeof(float));   // the zero row
  unsigned svoff[4] = {zoff, zoff, zoff, zoff};   // byte offsets of the four patch pixels of row sr
  if (stile < tiles_valid) {
    const int s = csp ? 0 : stile / TPS, rem = csp ? band * TT + stile : stile - s * TPS;
    const int th = rem / TW, tw = rem - th * TW;
    const int sy = 2 * th - 1 + sr;
    if (sy >= 0 && sy < d.H) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int x = 2 * tw - 1 + i;
        if (x >= 0 && x < d.W) svoff[i] = (unsigned)((((s * d.HW) + sy * d.W + x) * d.C + sq4 * 4) * 4);
      }
    }
  }

  // ---- operand offsets: wave w = the four components (xi = w >> 1, nu = 0..3) of column half w & 1, so the
  //      nu half of the output transform happens in registers before anything goes through LDS ----
  const int wxi = wave >> 1, wnn = wave & 1;
  const int arow = l31 * SST2 + (4 * wxi) * ASTW + 8 * (hi ^ (wxi >> 1));   // + nu * ASTW, + 4 g  (xi >= 2: quads 0,1 <-> 2,3, see slofs)
  const int nchunk = (d.C + KCW - 1) / KCW;
  const float* wbase = a.wpacked + (size_t)nt * nchunk * (16 * BN * KCW);
  const int bofs = ((4 * wxi) * BN + wnn * 32 + l31) * KCW + 8 * hi;   // [comp][col][16]: + nu * BN*KCW, + 4 g

  f32x16 acc[4];   // [nu]
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

  // no zero fill: every (tile, component, channel) slot is rewritten for each chunk and the pads are never read

  float4 areg[2][4];   // patch rows of chunks q+1 and q+2 (set = chunk parity): requested two chunks ahead, the
                       // activations come from HBM / MALL and one chunk (~2500 cycles) did not cover them
  // CBASE is clamped by the callers (requests run up to three chunks ahead; C % 32 == 0 here: no ragged chunk)
#define ALOAD1(DST, CBASE, I)                                                              \
  DST[I] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(abase + (CBASE)) + svoff[I]);
  // x transform of this lane's patch row, then the y transform with ONE other row of the quad:
  //   xi = 0: e(0) - e(2)   xi = 1: e(1) + e(2)   xi = 2: e(2) - e(1)   xi = 3: e(3) - e(1)    (lane r = xi owns e(r))
  // Row xi = 3 is the NEGATIVE of the textbook B^T row (e(1) - e(3)); k_pack_weights_w2 negates the same row of the
  // filter transform, so the products are unchanged.  That makes every lane's result "own + (+/-) the other row":
  // two instructions per element -- a DPP-fused XOR that fetches the other row and sets its sign, and an add --
  // instead of four (mov_dpp, two multiplies by +/-1, fma).  The transform is the main loop's VALU bill, and a
  // VALU instruction costs ~11 cycles of this wave's issue time next to the partner's MFMA stream.
#define QPX(v) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (v)), 0x5A /* quad_perm [2,2,1,1] */, 0xf, 0xf, true) ^ spmask)
  const int spmask = sr == 1 ? 0 : (int)0x80000000;   // the other row enters negated except for xi = 1
  // one transformed column nu of the patch row: 4 channels, one 16-B LDS write
#define AWRITE1(SRC, ABASE, NU)                                                            \
  {                                                                                        \
    const float4 pl = (NU) == 0 ? SRC[0] : (NU) == 2 ? SRC[2] : SRC[1];                    \
    const float4 pr = (NU) == 0 ? SRC[2] : (NU) == 2 ? SRC[1] : (NU) == 1 ? SRC[2] : SRC[3]; \
    const float sg = (NU) == 1 ? 1.f : -1.f;                                               \
    const float e0 = pl.x + sg * pr.x, e1 = pl.y + sg * pr.y, e2 = pl.z + sg * pr.z, e3 = pl.w + sg * pr.w; \
    *reinterpret_cast<float4*>((ABASE) + slofs + (NU) * ASTW) =                            \
        make_float4(e0 + QPX(e0), e1 + QPX(e1), e2 + QPX(e2), e3 + QPX(e3));              \
  }

  // filter operands [register set][nu 4 x group 2]: the set of chunk q+1 fills while
  // chunk q computes
  float4 pb[2][8];
#define BLOAD1(SET, PQ, G, J)                                                               \
  pb[SET][(J) * 2 + (G)] = *reinterpret_cast<const float4*>(wbase + (size_t)(PQ) * (16 * BN * KCW) + bofs + 4 * (G) + (J) * (BN * KCW));

#define SB __builtin_amdgcn_sched_barrier(0)
  __syncthreads();  // zero fill + tables visible
  // Prologue requests in the steady state's order (filter group 0, activations, filter group 1), pinned: the
  // compiler merges the wait state of the loop entry into every iteration, so a different order here would
  // cost a wait for the youngest request in every chunk.
  {
    float4 areg0[4];
    const int cbl1 = min(KCW, d.C - KCW), cbl2 = min(2 * KCW, d.C - KCW);
    ALOAD1(areg0, 0, 0) ALOAD1(areg0, 0, 1) ALOAD1(areg0, 0, 2) ALOAD1(areg0, 0, 3)
    ALOAD1(areg[1], cbl1, 0) ALOAD1(areg[1], cbl1, 1) ALOAD1(areg[1], cbl1, 2) ALOAD1(areg[1], cbl1, 3)
    SB;
    BLOAD1(0, 0, 0, 0) BLOAD1(0, 0, 0, 1) BLOAD1(0, 0, 0, 2) BLOAD1(0, 0, 0, 3)
    SB;
    BLOAD1(0, 0, 1, 0) BLOAD1(0, 0, 1, 1) BLOAD1(0, 0, 1, 2) BLOAD1(0, 0, 1, 3)
    SB;
    ALOAD1(areg[0], cbl2, 0) ALOAD1(areg[0], cbl2, 1) ALOAD1(areg[0], cbl2, 2) ALOAD1(areg[0], cbl2, 3)
    SB;
    AWRITE1(areg0, Abuf, 0) AWRITE1(areg0, Abuf, 1) AWRITE1(areg0, Abuf, 2) AWRITE1(areg0, Abuf, 3)
    SB;
  }
  __syncthreads();
  PSTAMP(a.stamps, 2, "s_memtime");

  float4 pa0[4], pa1[4];
#define LOADA2(PA, AB, G)                                                                  \
  do {                                                                                     \
    _Pragma("unroll") for (int nu_ = 0; nu_ < 4; ++nu_)                                    \
      PA[nu_] = *reinterpret_cast<const float4*>((AB) + arow + nu_ * ASTW + 4 * (G));      \
  } while (0)
  // Half a k step: the two MFMAs of components nu = 2 CC, 2 CC + 1.  MFMA intrinsics carry no chain, so
  // instruction selection may float them past a sched_barrier and the memory operations behind it; the empty
  // asm that "uses" the accumulators ties the pair to its place.
#define HSTEP(CC, PA, SET, G, E)                                                                                             \
  acc[2 * (CC)] = __builtin_amdgcn_mfma_f32_32x32x2f32(PA[2 * (CC)].E, pb[SET][(2 * (CC)) * 2 + (G)].E, acc[2 * (CC)], 0, 0, 0);                 \
  acc[2 * (CC) + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(PA[2 * (CC) + 1].E, pb[SET][(2 * (CC) + 1) * 2 + (G)].E, acc[2 * (CC) + 1], 0, 0, 0); \
  asm volatile("" : "+v"(acc[2 * (CC)]), "+v"(acc[2 * (CC) + 1]) :: "memory");

  LOADA2(pa0, Abuf, 0);
#ifdef NODE_STAMPS
  unsigned long long tk_prev, tk_acc[4] = {0, 0, 0, 0};
#define TICK0 asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tk_prev)::"memory")
#define TICK(k) do { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); tk_acc[k] += t_ - tk_prev; tk_prev = t_; } while (0)
#else
#define TICK0 do { } while (0)
#define TICK(k) do { } while (0)
#endif
  // One piece = one K chunk (16 channels): 16 half steps of two MFMAs, each followed by ONE staging item, so
  // that neither the vector-memory issue (16 cycles of address path per 16-B request), the LDS writes nor the
  // transform VALU come as a burst in which the matrix pipe idles:
  //   half steps  0- 3 (group 0, k = 0,1): the four group-0 filter requests of chunk q+1 (other register set)
  //   half steps  4- 7 (group 0, k = 2,3): transform + LDS write of the four columns of chunk q+1's patch row
  //   half steps  8-11 (group 1, k = 0,1): the four activation requests of chunk q+3 (into the registers just freed)
  //   -- lgkmcnt(0) + barrier (the LDS writes have had four half steps to drain), group-0 operands of q+1 --
  //   half steps 12-15 (group 1, k = 2,3): the four group-1 filter requests of chunk q+1
  // Every request is unconditional and at least half a chunk ahead of its use; the in-order vmcnt waits the
  // compiler derives are exact (8 / 8 / 4 younger requests).  Buffer (q + 1) % 3 was last read in chunk q-2,
  // which every wave had left before anyone passed the previous barrier.  The pieces alternate between the two
  // filter register sets; an odd chunk count gets a phantom piece (activations out of range = zero).
#ifdef W2_NO_BLOAD
#define LB(...)
#else
#define LB(...) BLOAD1(__VA_ARGS__)
#endif
#ifdef W2_NO_ALOAD
#define LA(...)
#else
#define LA(...) ALOAD1(__VA_ARGS__)
#endif
#ifdef W2_NO_AWRITE
#define LW(...)
#else
#define LW(...) AWRITE1(__VA_ARGS__)
#endif
#define PIECE2(SET, NSET)                                                                  \
  {                                                                                        \
    float* Anxt = Abuf + abuf_n * ABUF;                                                    \
    const int q1 = min(chunk + 1, nchunk - 1);                                             \
    const int cb2 = min((chunk + 3) * KCW, d.C - KCW);                                                   \
    LOADA2(pa1, Acur, 1); SB;                                                              \
    HSTEP(0, pa0, SET, 0, x) LB(NSET, q1, 0, 0) SB;                                    \
    HSTEP(1, pa0, SET, 0, x) LB(NSET, q1, 0, 1) SB;                                    \
    HSTEP(0, pa0, SET, 0, y) LB(NSET, q1, 0, 2) SB;                                    \
    HSTEP(1, pa0, SET, 0, y) LB(NSET, q1, 0, 3) SB;                                    \
    TICK(0);                                                                               \
    HSTEP(0, pa0, SET, 0, z) LW(areg[NSET], Anxt, 0) SB;                                    \
    HSTEP(1, pa0, SET, 0, z) LW(areg[NSET], Anxt, 1) SB;                                    \
    HSTEP(0, pa0, SET, 0, w) LW(areg[NSET], Anxt, 2) SB;                                    \
    HSTEP(1, pa0, SET, 0, w) LW(areg[NSET], Anxt, 3) SB;                                    \
    TICK(1);                                                                               \
    HSTEP(0, pa1, SET, 1, x) LB(NSET, q1, 1, 0) SB;                                        \
    HSTEP(1, pa1, SET, 1, x) LB(NSET, q1, 1, 1) SB;                                        \
    HSTEP(0, pa1, SET, 1, y) LB(NSET, q1, 1, 2) SB;                                        \
    HSTEP(1, pa1, SET, 1, y) LB(NSET, q1, 1, 3) SB;                                        \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                     \
    __builtin_amdgcn_s_barrier();                                                          \
    SB;                                                                                    \
    TICK(2);                                                                               \
    LOADA2(pa0, Anxt, 0); SB;                                                              \
    HSTEP(0, pa1, SET, 1, z) LA(areg[NSET], cb2, 0) SB;                                    \
    HSTEP(1, pa1, SET, 1, z) LA(areg[NSET], cb2, 1) SB;                                    \
    HSTEP(0, pa1, SET, 1, w) LA(areg[NSET], cb2, 2) SB;                                    \
    HSTEP(1, pa1, SET, 1, w) LA(areg[NSET], cb2, 3) SB;                                    \
    TICK(3);                                                                               \
    Acur = Anxt;                                                                           \
    abuf_n = abuf_n == 2 ? 0 : abuf_n + 1;                                                 \
    ++chunk;                                                                               \
  }
  {
    int abuf_n = 1;
    float* Acur = Abuf;
    TICK0;
    for (int chunk = 0; chunk < nchunk;) {
      PIECE2(0, 1)
      PIECE2(1, 0)
#ifdef NODE_STAMPS
      if (chunk == 2) PSTAMP(a.stamps, 11, "s_memtime");   // end of the first loop iteration (cold instruction cache)
#endif
    }
  }
#ifdef NODE_STAMPS
  if (a.stamps != nullptr && (threadIdx.x & 63) == 0)
    for (int k = 0; k < 4; ++k)
      a.stamps[((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 16 + 12 + k] = tk_acc[k];
#endif
  PSTAMP(a.stamps, 3, "s_memtime");

  // bias + t * tmap of the pixel-tile elements this thread finalises (column tid & 63, tiles (tid >> 6) + 8 i, 2x2
  // pixels each): requested here, consumed after the two transform rounds (the kernel is at its register limit,
  // so they are not held across the main loop)
  float tmv[16];
  int ptl[4];
  {
    const int col = tid & 63;
    const int ccol = c0 + min(col, ncols - 1);   // clamped: the requests below stay unconditional (independent, one wait)
    const float tval = fwd ? eval_time(a.et) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) ptl[i] = ptab[(tid >> 6) + 8 * i];
    if (fwd) {   // wave-uniform
      const float bias = a.bias[ccol];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int q = qtab[(tid >> 6) + 8 * i];
#pragma unroll
        for (int e = 0; e < 4; ++e) tmv[4 * i + e] = a.tmap[(size_t)(q + (e >> 1) * d.W + (e & 1)) * d.C + ccol];
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) tmv[k] = bias + tval * tmv[k];
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) tmv[k] = 0.f;
    }
  }

  // ---- output transform Y = A^T M A: the nu half in registers, the xi half through LDS ----
  //   T[xi][0] = M[xi][0] + M[xi][1] + M[xi][2]     T[xi][1] = M[xi][1] - M[xi][2] - M[xi][3]
  //   Y[0][j] = T[0][j] + T[1][j] + T[2][j]         Y[1][j] = T[1][j] - T[2][j] - T[3][j]
  float* Ct = smem;  // [BM][CT2]
  float* Mt = smem + 2 * BM * CT2 + 2 * d.S * BN + 32 * 64 * 2;   // T [xi 4][j 2][TT][CT2], behind the region the tail uses
  float y[4][4];     // [tile i][pixel e = 2 * row + col]
  {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float m12 = acc[1][r] + acc[2][r], d12 = acc[1][r] - acc[2][r];
      const int row = (r & 3) + 8 * (r >> 2) + 4 * hi;
      Mt[((wxi * 2 + 0) * TT + row) * CT2 + wnn * 32 + l31] = acc[0][r] + m12;
      Mt[((wxi * 2 + 1) * TT + row) * CT2 + wnn * 32 + l31] = d12 - acc[3][r];
    }
  }
  __syncthreads();
  {
    const int col = tid & 63;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int tl = (tid >> 6) + 8 * i;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float t0 = Mt[((0 * 2 + j) * TT + tl) * CT2 + col], t1 = Mt[((1 * 2 + j) * TT + tl) * CT2 + col];
        const float t2 = Mt[((2 * 2 + j) * TT + tl) * CT2 + col], t3 = Mt[((3 * 2 + j) * TT + tl) * CT2 + col];
        y[i][j] = (t0 + t1) + t2;
        y[i][2 + j] = (t1 - t2) - t3;
      }
    }
  }
  {
    const int col = tid & 63;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (ptl[i] >= 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) Ct[(ptl[i] + (e >> 1) * d.W + (e & 1)) * CT2 + col] = y[i][e] + tmv[4 * i + e];
      }
  }
  __syncthreads();
  PSTAMP(a.stamps, 6, "s_memtime");
  if (a.raw_out) {   // split mode: the band's 128 pixels x ncols, as they are (conv + bias + t * tmap, or the raw data gradient)
    const int colq = (tid & 15) * 4, rr = tid >> 4;
    const bool vec_ok = ((c0 & 3) == 0) && ((ncols & 3) == 0);
    for (int p = rr; p < BM; p += THREADS / 16) {
      const float* src = Ct + p * CT2 + colq;
      const size_t off = ((size_t)n0 * d.HW + (size_t)band * BM + p) * d.C + c0 + colq;
      if (vec_ok) {
        if (colq < ncols) *reinterpret_cast<float4*>(a.raw_out + off) = make_float4(src[0], src[1], src[2], src[3]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (colq + i < ncols) a.raw_out[off + i] = src[i];
      }
    }
    PSTAMP(a.stamps, 4, "s_memtime");
    PSTAMP(a.stamps, 5, "s_memrealtime");
    return;
  }
  conv_epilogue_tail<THREADS, BM>(a, d, smem, n0, c0, nsamp, ncols, mtile);
  PSTAMP(a.stamps, 4, "s_memtime");
  PSTAMP(a.stamps, 5, "s_memrealtime");
}

size_t conv_w2_lds_bytes(const Dims& d) {
  const size_t main_loop = 3 * (size_t)32 * SST2;
  const size_t epi = 2 * (size_t)128 * CT2 + 2 * (size_t)d.S * BN + 32 * 64 * 2 + 8 * (size_t)32 * CT2;
  return ((main_loop > epi ? main_loop : epi) + 64) * sizeof(float);   // + the two tile tables
}

// 2-D filter transform + packing: packed[nt][chunk16][comp = xi*4 + nu][col 64][k 16],  U = G g G^T
struct PackJobs { const float* w[4]; float* packed[4]; int dgrad[4]; };
__global__ __launch_bounds__(256) void k_pack_weights_w2(PackJobs jobs, int C, int BNE, int ntile, int nchunk) {
  // blockIdx.y = job: the forward / data-gradient packings of both conv layers leave in one launch per solve
  const float* __restrict__ w = jobs.w[blockIdx.y];
  float* __restrict__ packed = jobs.packed[blockIdx.y];
  const int dgrad = jobs.dgrad[blockIdx.y];
  // thread = (nt, chunk, col, k): reads the nine taps of its (co, ci) pair ONCE and writes all sixteen components
  // (consecutive threads -> consecutive k, col: every component's store is contiguous across the wave)
  const size_t total = (size_t)ntile * nchunk * BN * KCW;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int kk = idx % KCW;
    size_t r = idx / KCW;
    const int col = r % BN; r /= BN;
    const int ch = r % nchunk;
    const int nt = r / nchunk;
    const int kidx = ch * KCW + kk, nidx = nt * BNE + col;
    float g[3][3];
    const bool on = col < BNE && kidx < C && nidx < C;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
        g[kh][kw] = !on ? 0.f
                        : dgrad ? w[(((size_t)kidx * (C + 1) + 1 + nidx) * 3 + (2 - kh)) * 3 + (2 - kw)]
                                : w[(((size_t)nidx * (C + 1) + 1 + kidx) * 3 + kh) * 3 + kw];
    auto G = [](int a, int b) -> float {   // rows of G: [1,0,0], [.5,.5,.5], [.5,-.5,.5], [0,0,1]
      return a == 0 ? (b == 0 ? 1.f : 0.f) : a == 1 ? 0.5f : a == 2 ? (b == 1 ? -0.5f : 0.5f) : (b == 2 ? 1.f : 0.f);
    };
    float* dst = packed + (((size_t)(nt * nchunk + ch) * 16) * BN + col) * KCW + kk;   // + comp * BN * KCW
#pragma unroll
    for (int comp = 0; comp < 16; ++comp) {
      const int xi = comp >> 2, nu = comp & 3;
      float v = 0.f;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) v += G(xi, kh) * g[kh][kw] * G(nu, kw);
      if (xi == 3) v = -v;   // the kernel's input transform uses the negated row xi = 3 (see AWRITE1)
      dst[(size_t)comp * BN * KCW] = v;
    }
  }
}
void launch_pack_weights_w2_multi(const Dims& d, const float* const* w, float* const* packed, const int* dgrad, int count,
                                 hipStream_t s) {
  PackJobs jobs;
  memset(&jobs, 0, sizeof(jobs));
  for (int i = 0; i < count; ++i) { jobs.w[i] = w[i]; jobs.packed[i] = packed[i]; jobs.dgrad[i] = dgrad[i]; }
  const int nchunk = (d.C + KCW - 1) / KCW;
  const size_t total = (size_t)d.ntile * nchunk * BN * KCW;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_pack_weights_w2, dim3(blocks, count), dim3(256), 0, s, jobs, d.C, d.BNE, d.ntile, nchunk);
}
void launch_pack_weights_w2(const Dims& d, const float* w, float* packed, int dgrad, hipStream_t s) {
  launch_pack_weights_w2_multi(d, &w, &packed, &dgrad, 1, s);
}

// 2-D Winograd (128-pixel tiles, even H and W); weights packed by launch_pack_weights_w2
void launch_conv_w2(const Dims& d, const ConvArgs& a, hipStream_t s) {
  static bool attr[MAX_DEVICES];
  allow_full_lds((const void*)k_conv3x3_w2, attr);
  hipLaunchKernelGGL(k_conv3x3_w2, dim3(d.mtiles, d.ntile), dim3(512), conv_w2_lds_bytes(d), s, a, d);
}

}  // namespace node
