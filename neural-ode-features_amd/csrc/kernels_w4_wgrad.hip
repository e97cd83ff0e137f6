// Winograd F(4x4,3x3) pipeline: the weight gradients in the transform domain -- k_w4_wgrad (fp32 MFMA), k_w4_wgrad128b (bf16
// triples, long filters), k_w4_wgrad64h (fp16 pairs) -- and k_w4_gemm64h_wgrad64h, the fp16-pair weight gradient and the conv-1 data
// gradient's component GEMMs of an augmented evaluation as one launch.  gfx950 (MI355X / CDNA4) only.  See wino4.h for the data layouts.
#include "w4_gemm.h"
#include <cstring>

namespace node {

// ----------------------------------------------------------------------------
// k_w4_wgrad: the weight gradients of BOTH conv layers of an augmented evaluation in the F(4x4,3x3) domain,
//   dU_c[ci][co] = sum_rows V_c[row][ci] Z_c[row][co]        c = 0..35, rows = samples x 4 tiles
// with V = B^T d B the forward conv's own row operand (as its GroupNorm pass left it for k_w4_gemm64 -- no second copy)
// and Z = A dz A^T of the conv output's cotangent (written by the pass that produces dz, wino4.h).  dW = G^T dU G
// happens in k_theta_finalize.  2.4 GFLOP per layer instead of the F(2x2,3x3) domain's 4.3, and NO split-K slabs:
// the decomposition mirrors k_w4_gemm64 -- a wave owns one whole component of a (128 ci x 32 co) tile over the WHOLE
// reduction (four 32x32 accumulators), eight workgroups share a tile, workgroup j takes components 4j .. 4j+3 and two of
// the four accumulator blocks of component 32 + j/2, whose reduction range its four waves split and sum through LDS:
// 1024 + 128 MFMAs per wave, every SIMD of the chip the same; every result element is written once.
// Operands: a lane's 16 B of V hold FOUR ci of one row -- they feed four MFMAs with four different accumulator blocks
// (block e = channels 8 g + 4 hi + e: any assignment of channels to MFMA rows is as good as another), so V is read in
// the layout the conv wants; a lane's 16 B of Z hold four ROWS of one co ([comp][co/32][sample][co%32][tile]: one
// contiguous 1 KB per wave request).  Workgroup j of every tile runs on XCD j: its 4.5 components of V and Z stream
// through that XCD's L2 once.  Needs N % 8 == 0, C % 128 == 0.
// (Round 3, measured: the same kernel on the bf16 pipe -- both operands split into exact bf16 triples in registers, as
// k_w4_gemm64b does -- takes the same 42 us: at 94 MB of operands and results per launch the memory side, not the
// matrix pipe, bounds it.  So it stays on the fp32 instructions.)
// ----------------------------------------------------------------------------
struct W4WgOps { float4 a0, a1, a2, a3, z; };
template <int NSUB>
__device__ __forceinline__ void w4_wg_mac(float16_t (&acc)[4], const W4WgOps& o, int sub0) {
#define W4WG_STEP(A, ZC)                                                                    \
  if (NSUB == 4) {                                                                           \
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.x, ZC, acc[0], 0, 0, 0);                  \
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.y, ZC, acc[1], 0, 0, 0);                  \
    acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.z, ZC, acc[2], 0, 0, 0);                  \
    acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.w, ZC, acc[3], 0, 0, 0);                  \
  } else {                                                                                   \
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(sub0 ? A.z : A.x, ZC, acc[0], 0, 0, 0);     \
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(sub0 ? A.w : A.y, ZC, acc[1], 0, 0, 0);     \
  }
  W4WG_STEP(o.a0, o.z.x) W4WG_STEP(o.a1, o.z.y) W4WG_STEP(o.a2, o.z.z) W4WG_STEP(o.a3, o.z.w)
#undef W4WG_STEP
}
// operands of reduction unit q (eight rows = samples 2q, 2q+1): pa / pz point at unit 0 of this lane
__device__ __forceinline__ void w4_wg_load(W4WgOps& o, const float* pa, const float4* pz, int q, size_t rbs) {
  const float4* a = reinterpret_cast<const float4*>(pa + (size_t)(q >> 2) * rbs + (q & 3) * 64);
  o.a0 = a[0]; o.a1 = a[1]; o.a2 = a[2]; o.a3 = a[3];
  o.z = pz[(size_t)q * 64];
}
// acc += sum over units [q0, q0 + nq): a ring of R units in registers, each refilled right behind the MFMAs that
// consumed it.  nq must be a multiple of R.
template <int R, int NSUB>
__device__ __forceinline__ void w4_wg_run(float16_t (&acc)[4], const float* pa, const float4* pz, int q0, int nq, size_t rbs, int sub0) {
  W4WgOps ring[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    w4_wg_load(ring[i], pa, pz, q0 + i, rbs);
    __builtin_amdgcn_sched_barrier(0);
  }
  int q = q0;
  for (; q + R < q0 + nq; q += R) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      w4_wg_mac<NSUB>(acc, ring[i], sub0);
      __builtin_amdgcn_sched_barrier(0);   // the refill stays behind the MFMAs that read the old contents
      w4_wg_load(ring[i], pa, pz, q + R + i, rbs);
    }
  }
#pragma unroll
  for (int i = 0; i < R; ++i) {
    w4_wg_mac<NSUB>(acc, ring[i], sub0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int R>
__global__ __launch_bounds__(256) void k_w4_wgrad(W4WgradArgs a) {
  if (a.ctrl != nullptr && a.ctrl->done) return;
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [4 waves][2 blocks][4 r4][64 lanes][4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int C = a.C, N = a.N;
  const int nCO = C >> 5, per_layer = (C >> 7) * nCO;
  const int j = blockIdx.x & 7, tile = blockIdx.x >> 3;
  const int layer = tile / per_layer, tl = tile - layer * per_layer;
  const int cit = tl / nCO, cot = tl - cit * nCO;
  const float* __restrict__ V = layer ? a.V2 : a.V1;
  const float4* __restrict__ Z = reinterpret_cast<const float4*>(layer ? a.Z2 : a.Z1);
  float* __restrict__ dU = a.dU + (size_t)layer * 36 * C * C;
  const int g = l31 >> 1, hic = l31 & 1;                       // accumulator row j <-> channels 8 g + 4 hic + e (block e)
  const size_t cs = (size_t)4 * N * C, rbs = (size_t)(C >> 3) * 256;   // floats per component / per 8-sample row block of V
  const int Q = N >> 1;                                        // reduction units of eight rows
  const float* pa0 = V + (size_t)(cit * 16 + g) * 256 + h * 32 + hic * 16;
  const float4* pz0 = Z + (size_t)cot * N * 32 + h * 32 + l31;
  const size_t zcs = (size_t)nCO * N * 32;                     // float4s per component of Z

  // --- this wave's own component over the whole reduction.  a.sharev (NODE_TUNE_W4_SHAREV, nCO % 4 == 0): the four waves of a
  // workgroup take ONE component and four neighbouring co tiles -- they walk the same V blocks (the 128-ci operand, 80 % of the
  // launch's operand bytes) in lock-step and share them inside the CU -- instead of four components of one tile.
  {
    const bool sharev = a.sharev != 0 && (nCO & 3) == 0;
    const int comp = 4 * j + (sharev ? (cot & 3) : wave);
    const int ocot = sharev ? (cot & ~3) + wave : cot;
    float16_t acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[e][r] = 0.f;
    w4_wg_run<R, 4>(acc, pa0 + (size_t)comp * cs, Z + (size_t)ocot * N * 32 + h * 32 + l31 + (size_t)comp * zcs, 0, Q, rbs, 0);
    float* o = dU + ((size_t)comp * C + cit * 128) * C + ocot * 32 + l31;
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = (r & 3) + 8 * (r >> 2) + 4 * h;          // accumulator row -> ci = 8 (m >> 1) + 4 (m & 1) + e
        st_wt(o + (size_t)(8 * (m >> 1) + 4 * (m & 1) + e) * C, acc[e][r]);
      }
  }
  // --- two accumulator blocks of a shared component: reduction range [wave Q/4, (wave+1) Q/4) per wave
  {
    const int scomp = 32 + (j >> 1), sub0 = j & 1;             // blocks e = 2 sub0, 2 sub0 + 1
    const int nq = Q >> 2, q0 = wave * nq;
    float16_t acc[4];
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[e][r] = 0.f;
    if (nq % 4 == 0) w4_wg_run<4, 2>(acc, pa0 + (size_t)scomp * cs, pz0 + (size_t)scomp * zcs, q0, nq, rbs, sub0);
    else for (int q = q0; q < q0 + nq; ++q) w4_wg_run<1, 2>(acc, pa0 + (size_t)scomp * cs, pz0 + (size_t)scomp * zcs, q, 1, rbs, sub0);
    float* red = smem + wave * 2048;
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4)
        *reinterpret_cast<float4*>(red + e * 1024 + (r4 * 64 + lane) * 4) =
            make_float4(acc[e][4 * r4], acc[e][4 * r4 + 1], acc[e][4 * r4 + 2], acc[e][4 * r4 + 3]);
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int u = tid + it * 256;
      const int e = u >> 8, r4 = (u >> 6) & 3;
      float4 s = *reinterpret_cast<const float4*>(smem + e * 1024 + (r4 * 64 + lane) * 4);
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const float4 v = *reinterpret_cast<const float4*>(smem + w * 2048 + e * 1024 + (r4 * 64 + lane) * 4);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      }
      const int ee = 2 * sub0 + e;
      float* o = dU + ((size_t)scomp * C + cit * 128) * C + cot * 32 + l31;
      const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = i + 8 * r4 + 4 * h;                       // register 4 r4 + i of the block
        st_wt(o + (size_t)(8 * (m >> 1) + 4 * (m & 1) + ee) * C, sv[i]);
      }
    }
  }
}

// ----------------------------------------------------------------------------
// k_w4_wgrad128b: k_w4_wgrad's sums on the bf16 matrix pipe at fp32 accuracy, as an LDS-tiled GEMM (the skeleton of
// k_w4_gemm128b): a workgroup owns a (128 ci x 128 co) tile of ONE component of one layer, its waves 64 x 64 quarters,
// and walks the reduction (rows = samples x 4 tiles) in K = 16 units.  The exact bf16 split costs more here than in the
// forward GEMM -- BOTH operands are fp32 activations -- and in k_w4_wgrad's decomposition (a wave = a 128 x 32 tile of its
// own component) every wave would split the same 128 ci x 16 rows again for each of the C / 32 column tiles (measured
// earlier in round 3: no faster than fp32).  Here an operand element is split once per 128-wide tile: per unit a wave
// splits 16 values per lane (88 VALU instructions) under its 24 MFMAs.
// Operands without a transposed copy: a loader lane's eight 16-B loads of V ([s 2][t 4] x four channels e) hold, for
// each e, the eight reduction rows of one channel -- the K half of an MFMA row operand -- so accumulator block e =
// channels 8 g + 4 hic + e as in k_w4_wgrad; its two 16-B loads of Z hold the eight rows of one output channel.
// Waves 0 / 1 load and split the V patch of the first / second sample of the K half (half of every block's LDS entries each),
// waves 2 / 3 two 32-column blocks of Z each.  Needs N % 4 == 0 (whole units; the launcher asks for N % 8) and C % 128 == 0.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void k_w4_wgrad128b(W4WgradArgs a) {
  if (a.ctrl != nullptr && a.ctrl->done) return;
  extern __shared__ __attribute__((aligned(16))) w4_u32x4 tile_lds[];   // [2 stages][A 4 e blocks x 3 parts | B 4 column blocks x 3 parts][64 lanes]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int C = a.C, N = a.N;
  const int nCT = C >> 7, nT = nCT * nCT;            // tiles per (layer, component)
  // XCD j (= blockIdx % 8): components 4 j .. 4 j + 3 of layer 0, then of layer 1, then half of the tiles of component 32 + j / 2
  // of either layer
  const int j = blockIdx.x & 7, i = blockIdx.x >> 3;
  int layer, comp, tile;
  if (i < 8 * nT) { layer = i / (4 * nT); const int r = i - layer * 4 * nT; comp = 4 * j + r / nT; tile = r % nT; }
  else { const int r = i - 8 * nT; layer = r / (nT >> 1); comp = 32 + (j >> 1); tile = (j & 1) * (nT >> 1) + r % (nT >> 1); }
  const int cit = tile / nCT, cot = tile - cit * nCT;
  const float* __restrict__ V = layer ? a.V2 : a.V1;
  const float4* __restrict__ Z = reinterpret_cast<const float4*>(layer ? a.Z2 : a.Z1);
  float* __restrict__ dU = a.dU + (size_t)layer * 36 * C * C;
  const size_t cs = (size_t)4 * N * C, rbs = (size_t)(C >> 3) * 256;   // floats per component / per 8-sample row block of V
  const int g = l31 >> 1, hic = l31 & 1;
  // unit u = samples 4 u .. 4 u + 3: this lane's K half h = samples 4 u + 2 h, + 1 (row block u / 2, s = 4 (u & 1) + 2 h + s')
  const float* pa = V + (size_t)comp * cs + (size_t)(cit * 16 + g) * 256 + (2 * h) * 32 + hic * 16;
  const float4* pz = Z + (size_t)comp * (size_t)(C >> 5) * N * 32 + (size_t)(4 * cot) * N * 32 + (2 * h) * 32 + l31;
  const int U = N >> 2;
  auto blk = [&](int stage, int kind, int b, int part) { return tile_lds + ((((stage * 2 + kind) * 4 + b) * 3 + part) * 64 + lane); };
  // What this wave loads for unit u, four 16-B requests each: wave 0 / 1 the V patch of sample s' = 0 / 1 of the lane's K half
  // ([t 4] x four channels e: the first / second four of the eight reduction rows of the four blocks e -- it writes the
  // first / second 8 bytes of their lanes' LDS entries), waves 2 / 3 two column blocks of Z ([block 2][s' 2]).  Requests as
  // inline asm with hand-placed waits, two register sets that are never copied, as in k_w4_gemm128b (left to the compiler
  // this loop waited for vmcnt(0) at the top of every unit: no prefetch at all).
  const bool ldv = wave < 2;
  const char* pvb = reinterpret_cast<const char*>(pa + (wave & 1) * 32);
  const char* pz0 = reinterpret_cast<const char*>(pz + (size_t)(2 * (wave & 1)) * N * 32);
  const char* pz1 = pz0 + (size_t)N * 32 * 16;
#define W4WG_FETCH(L, UU)                                                                                              \
  {                                                                                                                    \
    const int u_ = (UU) < U ? (UU) : U - 1; /* clamped: the last units prefetch one nobody consumes */                 \
    if (ldv) {                                                                                                         \
      const char* p_ = pvb + ((size_t)(u_ >> 1) * rbs + (u_ & 1) * 128) * 4;                                           \
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(L##0) : "v"(p_) : "memory");                               \
      asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=v"(L##1) : "v"(p_) : "memory");                     \
      asm volatile("global_load_dwordx4 %0, %1, off offset:32" : "=v"(L##2) : "v"(p_) : "memory");                     \
      asm volatile("global_load_dwordx4 %0, %1, off offset:48" : "=v"(L##3) : "v"(p_) : "memory");                     \
    } else {                                                                                                           \
      const char* q0_ = pz0 + (size_t)u_ * 2048;                                                                       \
      const char* q1_ = pz1 + (size_t)u_ * 2048;                                                                       \
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(L##0) : "v"(q0_) : "memory");                              \
      asm volatile("global_load_dwordx4 %0, %1, off offset:512" : "=v"(L##1) : "v"(q0_) : "memory");                   \
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(L##2) : "v"(q1_) : "memory");                              \
      asm volatile("global_load_dwordx4 %0, %1, off offset:512" : "=v"(L##3) : "v"(q1_) : "memory");                   \
    }                                                                                                                  \
  }
  // wait until only the younger set's four requests are in flight; NALL: wait for everything
#define W4WG_WAIT(L, NALL)                                                                                              \
  {                                                                                                                     \
    if (NALL) asm volatile("s_waitcnt vmcnt(0)" : "+v"(L##0), "+v"(L##1), "+v"(L##2), "+v"(L##3) : : "memory");         \
    else asm volatile("s_waitcnt vmcnt(4)" : "+v"(L##0), "+v"(L##1), "+v"(L##2), "+v"(L##3) : : "memory");              \
  }
#define W4WG_PUT(STAGE, KIND, B, SP)                                        \
  {                                                                         \
    *blk(STAGE, KIND, B, 0) = __builtin_bit_cast(w4_u32x4, (SP).h);         \
    *blk(STAGE, KIND, B, 1) = __builtin_bit_cast(w4_u32x4, (SP).m);         \
    *blk(STAGE, KIND, B, 2) = __builtin_bit_cast(w4_u32x4, (SP).l);         \
  }
  // V waves: the split of (block e, block e + 1) x four rows each; the first 8 bytes of a part belong to block e, the last to e + 1
#define W4WG_PUT_HALVES(STAGE, E, SP)                                                                                     \
  {                                                                                                                       \
    const w4_u32x4 h_ = __builtin_bit_cast(w4_u32x4, (SP).h), m_ = __builtin_bit_cast(w4_u32x4, (SP).m),                  \
                   l_ = __builtin_bit_cast(w4_u32x4, (SP).l);                                                             \
    typedef unsigned w4_u32x2_ __attribute__((ext_vector_type(2)));                                                       \
    w4_u32x2_* d0_ = reinterpret_cast<w4_u32x2_*>(blk(STAGE, 0, E, 0)) + (wave & 1);                                      \
    w4_u32x2_* d1_ = reinterpret_cast<w4_u32x2_*>(blk(STAGE, 0, (E) + 1, 0)) + (wave & 1);                                \
    d0_[0] = w4_u32x2_{h_[0], h_[1]};   d1_[0] = w4_u32x2_{h_[2], h_[3]};                                                 \
    d0_[128] = w4_u32x2_{m_[0], m_[1]}; d1_[128] = w4_u32x2_{m_[2], m_[3]};   /* parts are 64 lanes x 16 B apart */       \
    d0_[256] = w4_u32x2_{l_[0], l_[1]}; d1_[256] = w4_u32x2_{l_[2], l_[3]};                                               \
  }
#define W4WG_F4(A, B, C, D) make_float4(A, B, C, D)
#define W4WG_STASH(L, STAGE)                                                                                                  \
  {                                                                                                                           \
    if (ldv) {                                                                                                                \
      const W4Split s0_ = w4_split8(W4WG_F4((L##0).x, (L##1).x, (L##2).x, (L##3).x), W4WG_F4((L##0).y, (L##1).y, (L##2).y, (L##3).y)); \
      W4WG_PUT_HALVES(STAGE, 0, s0_)                                                                                          \
      const W4Split s1_ = w4_split8(W4WG_F4((L##0).z, (L##1).z, (L##2).z, (L##3).z), W4WG_F4((L##0).w, (L##1).w, (L##2).w, (L##3).w)); \
      W4WG_PUT_HALVES(STAGE, 2, s1_)                                                                                          \
    } else {                                                                                                                  \
      const W4Split s0_ = w4_split8(W4WG_F4((L##0).x, (L##0).y, (L##0).z, (L##0).w), W4WG_F4((L##1).x, (L##1).y, (L##1).z, (L##1).w)); \
      W4WG_PUT(STAGE, 1, 2 * (wave & 1), s0_)                                                                                 \
      const W4Split s1_ = w4_split8(W4WG_F4((L##2).x, (L##2).y, (L##2).z, (L##2).w), W4WG_F4((L##3).x, (L##3).y, (L##3).z, (L##3).w)); \
      W4WG_PUT(STAGE, 1, 2 * (wave & 1) + 1, s1_)                                                                             \
    }                                                                                                                         \
  }
  const int wr = wave >> 1, wc = wave & 1;
  float16_t acc[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[r][c][q] = 0.f;

  // units in flight: at the top of an even unit u, la holds unit u + 1 and lb unit u + 2 (la's requests the older)
  w4_f32x4 la0, la1, la2, la3, lb0, lb1, lb2, lb3;
  W4WG_FETCH(la, 0)
  W4WG_WAIT(la, 1)
  W4WG_STASH(la, 0)
  W4WG_FETCH(la, 1)
  W4WG_FETCH(lb, 2)
  __syncthreads();
#define W4WG_STEP(ST, L, UNEXT)                                                                                   \
  {                                                                                                               \
    w4_u32x4 fa[2][3], fb[2][3];                                                                                  \
    _Pragma("unroll") for (int r = 0; r < 2; ++r) _Pragma("unroll") for (int q = 0; q < 3; ++q) {                 \
      fa[r][q] = *blk(ST, 0, 2 * wr + r, q);                                                                      \
      fb[r][q] = *blk(ST, 1, 2 * wc + r, q);                                                                      \
    }                                                                                                             \
    w4c_mac(acc, fa, fb);                                                                                         \
    W4WG_WAIT(L, 0)                                                                                               \
    W4WG_STASH(L, (ST) ^ 1) /* the next unit -> the other stage (everybody left it at the last barrier) */        \
    W4WG_FETCH(L, UNEXT)                                                                                          \
    __syncthreads();                                                                                              \
  }
  for (int u = 0; u < U; u += 2) {   // (U = N / 4 is even: N % 8 == 0)
    W4WG_STEP(0, la, u + 3)
    W4WG_STEP(1, lb, u + 4)
  }
  W4WG_WAIT(la, 1)                    // nothing may still be landing in registers the epilogue reuses
  W4WG_WAIT(lb, 1)
#undef W4WG_STEP
#undef W4WG_FETCH
#undef W4WG_WAIT
#undef W4WG_PUT
#undef W4WG_PUT_HALVES
#undef W4WG_F4
#undef W4WG_STASH
  // block (e = 2 wr + r, column block 2 wc + c): accumulator row m = (q & 3) + 8 (q >> 2) + 4 h <-> ci = 8 (m >> 1) + 4 (m & 1) + e
  float* o = dU + ((size_t)comp * C + cit * 128) * C + cot * 128 + l31;
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int m = (q & 3) + 8 * (q >> 2) + 4 * h;
        st_wt(o + (size_t)(8 * (m >> 1) + 4 * (m & 1) + 2 * wr + r) * C + 32 * (2 * wc + c), acc[r][c][q]);
      }
}

// one 1 KB LDS-DMA piece (lane-linear destination) as inline asm: the compiler neither counts it nor drains it in front of LDS reads
__device__ __forceinline__ void w4wh_dma(const unsigned char* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

// ----------------------------------------------------------------------------
// k_w4_wgrad64h: k_w4_wgrad's sums on fp16 PAIRS (wino4.h): dU_c[ci][co] = 2^-(ev + ez) sum_rows V_c[row][ci] Z_c[row][co] with both
// operands as the GroupNorm passes left them -- V pairs (the forward GEMM's own row operand) and Z pairs in the SAME layout
// ([comp][rb][g2][part][s][hi][t][8 halves]: rows x 16 channels per 1 KB) -- three v_mfma_f32_32x32x16_f16 per 32 x 32 block and
// 16 rows: 14.5 GFLOP on the 2.5 PFLOP/s pipe instead of 4.8 GFLOP on the 157 TFLOP/s one.  The reduction runs over ROWS, so an
// MFMA operand is eight rows of one channel: the [row][channel] images go through LDS as they are (LDS-DMA, 1 KB per wave
// instruction, no registers) and come out transposed by ds_read_b64_tr_b16 -- a group of 16 lanes reads 4 rows (the four tiles
// of one sample) x 16 channels and each lane receives its channel's four rows.
//   workgroup = one 128 ci x 128 co tile of one (layer, component), waves = 64 x 64 quarters; K step = 16 rows = half a row block
//   (four samples): 8 KB of V + 8 KB of Z per step through a ring of W4WH_NST stages, W4WH_D steps in flight, ONE s_barrier per step
//   behind a counted s_waitcnt (the DMA pieces are inline asm: the compiler neither drains them in front of every LDS read nor
//   knows of them -- the counted waits are the only ordering, as in k_w4_gemm64l).  Odd 16-channel blocks sit in the image with
//   their samples' 128-B slots swapped pairwise (s ^ 1, applied on the DMA's per-lane SOURCE address): the two blocks a 32-lane
//   half reads then fall on different banks.  (layer, component) pairs are dealt to XCDs nine each, the tiles of a pair together:
//   its 1 MB of operands stays in that XCD's L2 for the second tile that reads it.  Two workgroups per CU.
// Needs N % 8 == 0 (whole row blocks), C % 128 == 0.
// ----------------------------------------------------------------------------
constexpr int W4WH_NST = 4, W4WH_D = 3, W4WH_STAGE = 16384;
struct W4WgradHArgs {
  const unsigned* V[2]; const unsigned* Z[2];   // per layer (Z[1] / V[1] nullable: one layer)
  float* dU; const Ctrl* ctrl; int N, C, layers;
  const int* v_exp[2]; const int* z_exp;
};
typedef short w4_s16x4 __attribute__((ext_vector_type(4)));
typedef short w4_s16x8 __attribute__((ext_vector_type(8)));
__global__ __launch_bounds__(256, 2) void k_w4_wgrad64h(W4WgradHArgs a) {
#define W4_BLOCK blockIdx.x
#include "w4_wgrad64h_body.inc"
#undef W4_BLOCK
}
bool w4_wgrad_f16_fits(int N, int C) {
  const W4Switches& sw = w4_switches();
  return sw.f16 != 0 && w4_select_wgrad(sw, N, C, true, W4Operands::Pairs) == W4Wgrad::F16_64;
}
void launch_w4_wgrad_f16(const unsigned* V1, const unsigned* Z1, const unsigned* V2, const unsigned* Z2, float* dU, const Ctrl* ctrl, int N, int C,
                         const int* v1_exp, const int* v2_exp, const int* z_exp, hipStream_t s) {
  static bool attr[MAX_DEVICES] = {};
  W4WgradHArgs a;
  memset(&a, 0, sizeof(a));
  a.V[0] = V1; a.Z[0] = Z1; a.V[1] = V2; a.Z[1] = Z2; a.dU = dU; a.ctrl = ctrl; a.N = N; a.C = C;
  a.layers = V2 != nullptr ? 2 : 1;
  a.v_exp[0] = v1_exp; a.v_exp[1] = v2_exp; a.z_exp = z_exp;
  const int T = (C >> 7) * (C >> 7);
  allow_full_lds(reinterpret_cast<const void*>(k_w4_wgrad64h), attr);
  hipLaunchKernelGGL(k_w4_wgrad64h, dim3(36 * a.layers * T), dim3(256), (size_t)W4WH_NST * W4WH_STAGE, s, a);
}

// ----------------------------------------------------------------------------
// k_w4_gemm64h_wgrad64h: an augmented evaluation's weight gradient (k_w4_wgrad64h) and its conv-1 data gradient's component GEMMs
// (k_w4_gemm64h) as ONE launch, a concatenated grid: the first `split` workgroups run one kernel's body, the rest the other's, each
// on its own index W4_BLOCK = blockIdx.x minus its offset.  Both grids are multiples of 8, so a workgroup of either half keeps its
// blockIdx & 7 -> XCD role and its work decomposition.  Neither half reads what the other writes (the weight gradient: V pairs, Z
// pairs -> dU; the GEMM: W4V, U pairs -> M) and NOTHING waits across workgroups: the halves only share the chip, so that one half's
// ring fill, store tail and kernel boundary are covered by the other half's streams.  Both bodies are 256 threads; each tests
// ctrl->done in front of its first request and returns as a whole workgroup (no barrier is left behind a returning wave).  The bodies
// are the stand-alone kernels' text (w4_gemm64h_body.inc, w4_wgrad64h_body.inc): same sums in the same order, same bits.
// Registers: the launch is allocated for the larger half.  MINB = 1: the GEMM's own budget (one wave per SIMD, ring depth 4) -- the
// weight gradient's workgroups then run ONE per CU instead of two; MINB = 2: at most 256 registers, two workgroups of either half
// per CU, the GEMM's ring at depth D = 2 (two waves per SIMD keep as many requests in flight as one wave at depth 4).
// profiles/wgrad_paired_ab.txt has the register counts and what was measured.
// ----------------------------------------------------------------------------
struct W4PairArgs {
  const unsigned* Vh; const unsigned* Uh; float* M; const int* v_exp; const int* u_exp; W4Geom gm; int mode;   // the GEMM's
  W4WgradHArgs w;                                                                                              // the weight gradient's
  unsigned split; int wgrad_first;    // workgroups of the half that comes first in the grid / which half that is
};
template <int D, int MINB>
__global__ __launch_bounds__(256, MINB) void k_w4_gemm64h_wgrad64h(W4PairArgs pa) {
  const bool head = blockIdx.x < pa.split;
  const unsigned block = head ? blockIdx.x : blockIdx.x - pa.split;
#define W4_BLOCK block
  if (head == (pa.wgrad_first == 0)) {
    const unsigned* __restrict__ Vh = pa.Vh;
    const unsigned* __restrict__ Uh = pa.Uh;
    float* __restrict__ M = pa.M;
    const Ctrl* ctrl = pa.w.ctrl;
    const W4Geom gm = pa.gm;
    const int mode = pa.mode;
    const int* v_exp = pa.v_exp;
    const int* u_exp = pa.u_exp;
    unsigned long long* const stamps = nullptr;
#include "w4_gemm64h_body.inc"
  } else {
    const W4WgradHArgs& a = pa.w;
#include "w4_wgrad64h_body.inc"
  }
#undef W4_BLOCK
}
// variant (NODE_TUNE_WGRAD_PAIRED): bit 0 set; bit 1: the GEMM's workgroups first (default: the weight gradient's); bit 2: MINB = 1
void launch_w4_pair_f16_64(const unsigned* Vh, const unsigned* Uh, float* M, const W4Geom& gm, int mode, const int* gv_exp, const int* gu_exp,
                           const unsigned* V1, const unsigned* Z1, const unsigned* V2, const unsigned* Z2, float* dU, const Ctrl* ctrl,
                           const int* v1_exp, const int* v2_exp, const int* z_exp, int variant, hipStream_t s) {
  static bool attr[3][MAX_DEVICES] = {};
  W4PairArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.Vh = Vh; pa.Uh = Uh; pa.M = M; pa.v_exp = gv_exp; pa.u_exp = gu_exp; pa.gm = gm; pa.mode = mode;
  pa.w.V[0] = V1; pa.w.Z[0] = Z1; pa.w.V[1] = V2; pa.w.Z[1] = Z2; pa.w.dU = dU; pa.w.ctrl = ctrl; pa.w.N = gm.N; pa.w.C = gm.C;
  pa.w.layers = 2;
  pa.w.v_exp[0] = v1_exp; pa.w.v_exp[1] = v2_exp; pa.w.z_exp = z_exp;
  const unsigned gemm_blocks = (gm.N / 16) * (gm.C >> 6) * 8, wgrad_blocks = 72 * (gm.C >> 7) * (gm.C >> 7);   // (the stand-alone launchers' grids)
  pa.wgrad_first = (variant & 2) == 0;
  pa.split = pa.wgrad_first ? wgrad_blocks : gemm_blocks;
  const dim3 grid(gemm_blocks + wgrad_blocks);
  const size_t lds = (size_t)W4WH_NST * W4WH_STAGE;      // the weight gradient's ring; the GEMM half uses the first 32 KB
  if ((variant & 4) != 0 && (gm.C >> 4) % 4 == 0) {
    allow_full_lds(reinterpret_cast<const void*>(k_w4_gemm64h_wgrad64h<4, 1>), attr[0]);
    hipLaunchKernelGGL((k_w4_gemm64h_wgrad64h<4, 1>), grid, dim3(256), lds, s, pa);
  } else if ((variant & 4) != 0) {
    allow_full_lds(reinterpret_cast<const void*>(k_w4_gemm64h_wgrad64h<2, 1>), attr[1]);
    hipLaunchKernelGGL((k_w4_gemm64h_wgrad64h<2, 1>), grid, dim3(256), lds, s, pa);
  } else {
    allow_full_lds(reinterpret_cast<const void*>(k_w4_gemm64h_wgrad64h<2, 2>), attr[2]);
    hipLaunchKernelGGL((k_w4_gemm64h_wgrad64h<2, 2>), grid, dim3(256), lds, s, pa);
  }
}

void launch_w4_wgrad(const W4WgradArgs& a_in, hipStream_t s) {
  const W4Switches& sw = w4_switches();
  W4WgradArgs a = a_in;
  a.sharev = sw.sharev;
  if (w4_select_wgrad(sw, a.N, a.C, a.V2 != nullptr, W4Operands::Fp32) == W4Wgrad::Bf16_128) {
    const int nT = (a.C >> 7) * (a.C >> 7);
    hipLaunchKernelGGL(k_w4_wgrad128b, dim3(8 * (8 * nT + nT)), dim3(256), 2 * 24 * 64 * 16, s, a);
    return;
  }
  const int grid = (a.V2 != nullptr ? 2 : 1) * (a.C >> 7) * (a.C >> 5) * 8;     // (layer = tile / tiles per layer)
  const size_t lds = 4 * 2048 * sizeof(float);
  if (a.N % 16 == 0) hipLaunchKernelGGL(k_w4_wgrad<8>, dim3(grid), dim3(256), lds, s, a);
  else hipLaunchKernelGGL(k_w4_wgrad<4>, dim3(grid), dim3(256), lds, s, a);
}

}  // namespace node
