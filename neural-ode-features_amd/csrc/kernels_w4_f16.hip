// Winograd F(4x4,3x3) pipeline, stage 2: the 36 component GEMMs on fp16 PAIRS -- k_w4_gemm64h (operands straight from L2, the
// training step's kernel), k_w4_gemm128h and k_w4_gemm256h (LDS-tiled, long reductions).  gfx950 (MI355X / CDNA4) only.
// See wino4.h for the operand format and the data layouts, w4_select.hip for which batch takes which kernel.
#include "w4_gemm.h"

namespace node {

// ----------------------------------------------------------------------------
// k_w4_gemm64h: k_w4_gemm64b's products on fp16 PAIRS (wino4.h): both operands arrive split -- V pairs written by the GroupNorm
// pass in front, U pairs by k_w4_pack -- so a K = 16 step of a 32 x 32 block is three v_mfma_f32_32x32x16_f16 (l h, h l, h h) on
// registers the loads delivered: no conversion, no subtraction, no vector instruction at all between the MFMAs (k_w4_gemm64b: six
// MFMAs and ~44 VALU instructions per row block and step, the matrix pipe busy 45 % of a wave's life).  Same decomposition, XCD
// placement and M layout as k_w4_gemm64b: a wave owns a 64 x 64 tile of one component over the whole reduction; eight workgroups
// share a tile (workgroup j: components 4 j .. 4 j + 3 and half a tile of component 32 + j / 2, K range cut over its waves).
// The result leaves unscaled: M = acc * 2^-(v_exp + u_exp).
// ----------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void k_w4_gemm64h(const unsigned* __restrict__ Vh, const unsigned* __restrict__ Uh, float* __restrict__ M,
                                                    const Ctrl* ctrl, W4Geom gm, int mode, const int* v_exp, const int* u_exp, unsigned long long* stamps) {
#define W4_BLOCK blockIdx.x
#include "w4_gemm64h_body.inc"
#undef W4_BLOCK
}

// ----------------------------------------------------------------------------
// k_w4_gemm128h: k_w4_gemm64h's products as an LDS-tiled GEMM (the skeleton of k_w4_gemm128b): a workgroup owns a 128 x 128 tile of
// ONE component, its waves 64 x 64 quarters; per K = 16 step each wave fetches ONE quarter of the tile's operands -- its 32-row block
// of V pairs and its 32-column block of U pairs, parts h and l: four 16-B requests per lane, already the MFMA fragments -- and
// the 16 KB of the step go through a four-stage LDS ring (one barrier per step), so a CU takes in 16 KB per step where
// k_w4_gemm64h's four independent 64 x 64 tiles take 32 KB.  Why: at long reductions k_w4_gemm64h, like k_w4_gemm64b, re-reads its
// operands from the Infinity Cache (371 against 262 us at cfg 5).  (At SHORT reductions k_w4_gemm64h stays: its launch runs at the
// memory system's pace for its bytes -- DESIGN.md 4.3; the texture path looked like its limit and is not, profiles/r06_gemm64v_ab.txt.)
// Requests as inline asm with hand-placed waits, NSET register sets in flight that are never copied (k_w4_gemm128b).  (Measured and
// removed, round 6: the same tile with the operands brought by LDS-DMA -- no staging instructions -- 14.1 - 17.9 us against
// k_w4_gemm64h's 12.8 at cfg 2: a CU's four DMA streams deliver less than its register loads do.)
// Work: components 0..31 give 32 nT tiles (nT = rows / 128 x C / 128); XCD j takes 4 j .. 4 j + 3 one after the other, and every
// workgroup adds one EIGHTH of a tile of component 32 + j / 2 (a 32 x 64 block, K range cut over its four waves and summed through
// LDS, operands straight into registers: k_w4_gemm64h's shared component), so every workgroup does the same work.
// Needs rows % 128 == 0 (N % 32 == 0), C % 128 == 0, nT even.
// ----------------------------------------------------------------------------
struct W4GLoad { w4_u32x4 a0, a1, b0, b1; };
#define W4G_FETCH(L, PA, PB)                                                                        \
  {                                                                                                 \
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"((L).a0) : "v"(PA) : "memory");            \
    asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"((L).a1) : "v"(PA) : "memory"); \
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"((L).b0) : "v"(PB) : "memory");            \
    asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"((L).b1) : "v"(PB) : "memory"); \
  }
#define W4G_WAIT(N, L) asm volatile("s_waitcnt vmcnt(" #N ")" : "+v"((L).a0), "+v"((L).a1), "+v"((L).b0), "+v"((L).b1) : : "memory")
template <int WPC>
__global__ __launch_bounds__(256, WPC) void k_w4_gemm128h(const unsigned* __restrict__ Vh, const unsigned* __restrict__ Uh, float* __restrict__ M,
                                                           const Ctrl* ctrl, W4Geom gm, const int* v_exp, const int* u_exp, int tail) {
  if (ctrl != nullptr && ctrl->done) return;   // a step enqueued past the end of the interval (Ctrl::done)
  extern __shared__ __attribute__((aligned(16))) w4_u32x4 gtile[];   // [4 stages][A 4 row blocks x 2 parts | B 4 column blocks x 2 parts][64 lanes]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int nCT = gm.C >> 7, nRT = gm.R >> 7, nT = nRT * nCT, G2 = gm.G8 >> 1, CB = gm.C >> 5, nRB = gm.RB;
  const int j = blockIdx.x & 7, i = blockIdx.x >> 3;            // XCD, slot: 4 nT slots per XCD
  // tail != 0 (behind k_w4_gemm256h, which multiplies components 0..31): the grid is the 4 nT tiles of components 32..35 themselves, a pair
  // of XCDs per component, and there is no shared piece
  const int comp = tail ? 32 + (j >> 1) : 4 * j + i / nT, tile = tail ? (j & 1) * (nT >> 1) + i : i % nT;
  const int RT = tile / nCT, CT = tile - RT * nCT;
  const float inv = ldexpf(1.f, -(*v_exp + *u_exp));
  const int a_off = ((l31 >> 2) * 8) + hi * 4 + (l31 & 3);      // lane (row = 4 s + t, k-half hi): its 16 B inside a 1 KB part of V
  // --- the shared component's piece: component 32 + j / 2; the pair of XCDs holds 8 nT workgroups = nT tiles x 8 pieces (4 row blocks x 2 column halves)
  const int sidx = (j & 1) * 4 * nT + i;
  const int stile = sidx >> 3, spiece = sidx & 7;
  const int scomp = 32 + (j >> 1);
  const int srb = 4 * (stile / nCT) + (spiece >> 1);             // its 32-row block
  const int scb = 4 * (stile % nCT) + 2 * (spiece & 1);          // the first of its two 32-column blocks
  const int sng = G2 >> 2;                                       // K steps per wave
  W4HCursor scu;
  scu.a[0] = reinterpret_cast<const w4_u32x4*>(Vh) + (((size_t)scomp * nRB + srb) * G2 + (size_t)wave * sng) * 128 + a_off; scu.a[1] = scu.a[0];
  scu.b[0] = reinterpret_cast<const w4_u32x4*>(Uh) + (((size_t)scomp * CB + scb) * G2 + (size_t)wave * sng) * 128 + lane;
  scu.b[1] = reinterpret_cast<const w4_u32x4*>(Uh) + (((size_t)scomp * CB + scb + 1) * G2 + (size_t)wave * sng) * 128 + lane;

  // this lane's requests of step g2: V at pa + g2 * 2 KB (+ 1 KB: part l), U at pb + g2 * 2 KB (+ 1 KB)
  const char* pa = reinterpret_cast<const char*>(reinterpret_cast<const w4_u32x4*>(Vh) + (((size_t)comp * nRB + 4 * RT + wave) * G2) * 128 + a_off);
  const char* pb = reinterpret_cast<const char*>(reinterpret_cast<const w4_u32x4*>(Uh) + (((size_t)comp * CB + 4 * CT + wave) * G2) * 128 + lane);
  auto blk = [&](int stage, int kind, int b, int part) { return gtile + (((stage * 2 + kind) * 4 + b) * 2 + part) * 64 + lane; };
#define W4G_STASH(L, STAGE)                   \
  {                                           \
    *blk(STAGE, 0, wave, 0) = (L).a0;         \
    *blk(STAGE, 0, wave, 1) = (L).a1;         \
    *blk(STAGE, 1, wave, 0) = (L).b0;         \
    *blk(STAGE, 1, wave, 1) = (L).b1;         \
  }
  const int wr = wave >> 1, wc = wave & 1;
  float16_t acc[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[r][c][q] = 0.f;

  // FOUR register sets, never copied (step s travels in set s % 4), FOUR LDS stages (step s sits in stage s % 4), TWO fragment sets:
  // step k multiplies fragments read from LDS a step earlier while step k + 1's travel LDS -> registers, stashes step k + 2 (requested
  // four steps ago) and requests step k + 6 -- one barrier per step, nothing a wave waits for was issued less than a step ago.
  // (Reads past the reduction's end land in the buffers' slack: W4_SLACK.)
  W4GLoad l0, l1, l2, l3;
  W4HStage fA, fB;
  W4G_FETCH(l0, pa, pb)
  W4G_FETCH(l1, pa + 2048, pb + 2048)
  W4G_FETCH(l2, pa + 4096, pb + 4096)
  W4G_FETCH(l3, pa + 6144, pb + 6144)
  W4G_WAIT(12, l0);
  W4G_STASH(l0, 0)
  W4G_FETCH(l0, pa + 8192, pb + 8192)
  W4G_WAIT(12, l1);
  W4G_STASH(l1, 1)
  W4G_FETCH(l1, pa + 10240, pb + 10240)
  pa += 6 * 2048; pb += 6 * 2048;            // -> step 6
  __syncthreads();
#define W4G_FRAGS(F, ST)                                                                          \
  _Pragma("unroll") for (int r = 0; r < 2; ++r) _Pragma("unroll") for (int q = 0; q < 2; ++q) {   \
    (F).a[r][q] = *blk(ST, 0, 2 * wr + r, q);                                                     \
    (F).b[r][q] = *blk(ST, 1, 2 * wc + r, q);                                                     \
  }
  W4G_FRAGS(fA, 0)
  // step k: FCUR = fragments of step k, FNEXT <- stage (k + 1) % 4, LSET = set (k + 2) % 4 -> stage (k + 2) % 4, then refilled with step k + 6
#define W4G_STEP(FCUR, FNEXT, STN, LSET, STS)                                                     \
  {                                                                                               \
    W4G_FRAGS(FNEXT, STN)                                                                         \
    w4h_mac<2>(acc, FCUR);                                                                        \
    W4G_WAIT(12, LSET);                                                                           \
    W4G_STASH(LSET, STS)                                                                          \
    W4G_FETCH(LSET, pa, pb)                                                                       \
    pa += 2048; pb += 2048;                                                                       \
    __syncthreads();                                                                              \
  }
  for (int k = 0; k < G2; k += 4) {   // (G2 = C / 16 is a multiple of 4: C % 128 == 0 gives 8)
    W4G_STEP(fA, fB, 1, l2, 2)
    W4G_STEP(fB, fA, 2, l3, 3)
    W4G_STEP(fA, fB, 3, l0, 0)
    W4G_STEP(fB, fA, 0, l1, 1)
  }
  W4G_WAIT(0, l0);                    // nothing may still be landing in registers the epilogue reuses
  W4G_WAIT(0, l1);
  W4G_WAIT(0, l2);
  W4G_WAIT(0, l3);
#undef W4G_FRAGS
#undef W4G_STEP
#undef W4G_STASH
  {
    const int rt = 2 * RT + wr, ct = 2 * CT + wc;                // this wave's 64 x 64 quarter
    const size_t sstride = (size_t)(gm.C >> 5) * 36 * 128;       // floats per sample of M
    float* m0 = M + ((size_t)(rt * 16 + hi) * (gm.C >> 5) + 2 * ct) * (36 * 128) + (size_t)comp * 128 + l31;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      float* o = m0 + (size_t)(2 * (q >> 2)) * sstride + (q & 3) * 32;
      st_wt(o, acc[0][0][q] * inv);
      st_wt(o + 36 * 128, acc[0][1][q] * inv);
      st_wt(o + 8 * sstride, acc[1][0][q] * inv);
      st_wt(o + 8 * sstride + 36 * 128, acc[1][1][q] * inv);
    }
  }
  // --- the shared piece: rows srb (32), column blocks scb, scb + 1; K range [wave sng, (wave + 1) sng) per wave
  if (!tail) {
    float16_t sa[2][2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int q = 0; q < 16; ++q) sa[0][c][q] = 0.f;
    if (sng % 4 == 0) w4h_run<4, 1>(sa, scu, sng);
    else if (sng % 2 == 0) w4h_run<2, 1>(sa, scu, sng);
    else w4h_run<1, 1>(sa, scu, sng);
    float* smem = reinterpret_cast<float*>(gtile);               // (everybody left the ring at the loop's last barrier)
    float* red = smem + wave * 2048;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4)
        *reinterpret_cast<float4*>(red + c * 1024 + (r4 * 64 + lane) * 4) =
            make_float4(sa[0][c][4 * r4], sa[0][c][4 * r4 + 1], sa[0][c][4 * r4 + 2], sa[0][c][4 * r4 + 3]);
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int u = tid + it * 256;
      const int blk2 = u >> 8, r4 = (u >> 6) & 3;
      float4 sm = *reinterpret_cast<const float4*>(smem + blk2 * 1024 + (r4 * 64 + lane) * 4);
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const float4 v = *reinterpret_cast<const float4*>(smem + w * 2048 + blk2 * 1024 + (r4 * 64 + lane) * 4);
        sm.x += v.x; sm.y += v.y; sm.z += v.z; sm.w += v.w;
      }
      float* mrow = M + ((size_t)(srb * 8 + 2 * r4 + hi) * (gm.C >> 5) + scb + blk2) * (36 * 128) + (size_t)scomp * 128 + l31;
      st_wt(mrow, sm.x * inv);
      st_wt(mrow + 32, sm.y * inv);
      st_wt(mrow + 64, sm.z * inv);
      st_wt(mrow + 96, sm.w * inv);
    }
  }
}
#undef W4G_FETCH
#undef W4G_WAIT

// ----------------------------------------------------------------------------
// k_w4_gemm256h (long reductions, rows % 256 == 0, C % 256 == 0): k_w4_gemm128h with FOUR times the tile.  What holds k_w4_gemm128h at
// 43 % matrix duty (cfg 5) is not the LDS (half its fragment reads removed: -2 %; three quarters of its writes: -5 %; profiles/
// r06_gemm256h.txt) but operand DELIVERY: 16 KB per 192 matrix cycles and workgroup, 18 % of it cold in L2, requested 1.1 us ahead.
// Here a workgroup owns a 256 x 256 tile of one component, ONE wave per SIMD, each wave a 128 x 128 quarter: sixteen 32 x 32 accumulators
// (256 registers), 48 MFMAs per K = 16 step and wave against 16 fragment reads -- half the LDS and half the global bytes per MFMA, and
// a step lasts 768 matrix cycles, so the same four steps of look-ahead are 1.5 us.  Per step a wave requests TWO row blocks and TWO
// column blocks (both parts: eight 16-B requests per lane, inline asm, FOUR register sets in flight, counted waits), four 32 KB LDS
// stages; the step is cut in four quadrants so that fragment halves travel under MFMAs (details at the loop).
// Components 0..31 only (32 nT tiles: XCD j takes components 4 j .. 4 j + 3); components 32..35 follow as k_w4_gemm128h<..>(tail = 1).
// ----------------------------------------------------------------------------
struct W4KLoad { w4_u32x4 a00, a01, a10, a11, b00, b01, b10, b11; };      // [block 0 | 1][part h | l] of V, of U
#define W4K_FETCH(L)                                                                                     \
  {                                                                                                      \
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"((L).a00) : "v"(pa0) : "memory");               \
    asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"((L).a01) : "v"(pa0) : "memory");   \
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"((L).a10) : "v"(pa1) : "memory");               \
    asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"((L).a11) : "v"(pa1) : "memory");   \
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"((L).b00) : "v"(pb0) : "memory");               \
    asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"((L).b01) : "v"(pb0) : "memory");   \
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"((L).b10) : "v"(pb1) : "memory");               \
    asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"((L).b11) : "v"(pb1) : "memory");   \
    pa0 += 2048; pa1 += 2048; pb0 += 2048; pb1 += 2048;                                                  \
  }
#define W4K_WAIT(N, L)                                                                                                         \
  asm volatile("s_waitcnt vmcnt(" #N ")" : "+v"((L).a00), "+v"((L).a01), "+v"((L).a10), "+v"((L).a11), "+v"((L).b00), "+v"((L).b01), \
               "+v"((L).b10), "+v"((L).b11) : : "memory")
struct W4KB { w4_u32x4 v[2][2]; };      // a fragment half: two row (or column) blocks, parts h | l
__global__ __launch_bounds__(256, 1) void k_w4_gemm256h(const unsigned* __restrict__ Vh, const unsigned* __restrict__ Uh, float* __restrict__ M,
                                                        const Ctrl* ctrl, W4Geom gm, const int* v_exp, const int* u_exp) {
  if (ctrl != nullptr && ctrl->done) return;   // a step enqueued past the end of the interval (Ctrl::done)
  extern __shared__ __attribute__((aligned(16))) w4_u32x4 ktile[];   // [4 stages][A | B][8 blocks][2 parts][64 lanes]: 128 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const int nCT = gm.C >> 8, nRT = gm.R >> 8, nT = nRT * nCT, G2 = gm.G8 >> 1, CB = gm.C >> 5, nRB = gm.RB;
  const int j = blockIdx.x & 7, i = blockIdx.x >> 3;            // XCD, slot: 4 nT slots per XCD
  const int comp = 4 * j + i / nT, tile = i % nT;
  const int RT = tile / nCT, CT = tile - RT * nCT;
  const float inv = ldexpf(1.f, -(*v_exp + *u_exp));
  const int a_off = ((l31 >> 2) * 8) + hi * 4 + (l31 & 3);      // lane (row = 4 s + t, k-half hi): its 16 B inside a 1 KB part of V
  const size_t blk_bytes = (size_t)G2 * 2048;                   // one 32-row / 32-column block over the whole reduction
  const char* pa0 = reinterpret_cast<const char*>(reinterpret_cast<const w4_u32x4*>(Vh) + (((size_t)comp * nRB + 8 * RT + 2 * wave) * G2) * 128 + a_off);
  const char* pa1 = pa0 + blk_bytes;
  const char* pb0 = reinterpret_cast<const char*>(reinterpret_cast<const w4_u32x4*>(Uh) + (((size_t)comp * CB + 8 * CT + 2 * wave) * G2) * 128 + lane);
  const char* pb1 = pb0 + blk_bytes;
  auto blk = [&](int stage, int kind, int b, int part) { return ktile + (((stage * 2 + kind) * 8 + b) * 2 + part) * 64 + lane; };
#define W4K_STASH(L, STAGE)                       \
  {                                               \
    *blk(STAGE, 0, 2 * wave, 0) = (L).a00;        \
    *blk(STAGE, 0, 2 * wave, 1) = (L).a01;        \
    *blk(STAGE, 0, 2 * wave + 1, 0) = (L).a10;    \
    *blk(STAGE, 0, 2 * wave + 1, 1) = (L).a11;    \
    *blk(STAGE, 1, 2 * wave, 0) = (L).b00;        \
    *blk(STAGE, 1, 2 * wave, 1) = (L).b01;        \
    *blk(STAGE, 1, 2 * wave + 1, 0) = (L).b10;    \
    *blk(STAGE, 1, 2 * wave + 1, 1) = (L).b11;    \
  }
  const int wr = wave >> 1, wc = wave & 1;
  float16_t acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[r][c][q] = 0.f;
  // fragments travel as HALVES of the wave's quarter: two row blocks (W4K_AH: half H of its four) or two column blocks (W4K_BH), both parts
#define W4K_AH(F, ST, H) \
  _Pragma("unroll") for (int b = 0; b < 2; ++b) _Pragma("unroll") for (int q = 0; q < 2; ++q) (F).v[b][q] = *blk(ST, 0, 4 * wr + 2 * (H) + b, q);
#define W4K_BH(F, ST, H) \
  _Pragma("unroll") for (int b = 0; b < 2; ++b) _Pragma("unroll") for (int q = 0; q < 2; ++q) (F).v[b][q] = *blk(ST, 1, 4 * wc + 2 * (H) + b, q);
  // one quadrant: acc[2 RH + r][2 CH + c] += A x B; per 32 x 32 tile the products (l,h), (h,l), (h,h) in this order (k_w4_gemm64h), four
  // independent MFMAs between two on the same accumulator
#define W4K_MAC1(AF, BF, RH, CH, PA, PB)                                                            \
  _Pragma("unroll") for (int r = 0; r < 2; ++r) _Pragma("unroll") for (int c = 0; c < 2; ++c)       \
      acc[2 * (RH) + r][2 * (CH) + c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(w4_f16x8, (AF).v[r][PA]), __builtin_bit_cast(w4_f16x8, (BF).v[c][PB]), acc[2 * (RH) + r][2 * (CH) + c], 0, 0, 0);
#define W4K_MAC(AF, BF, RH, CH) { W4K_MAC1(AF, BF, RH, CH, 1, 0) W4K_MAC1(AF, BF, RH, CH, 0, 1) W4K_MAC1(AF, BF, RH, CH, 0, 0) }
  // FOUR register sets, never copied (step s travels in set s % 4: requested four steps before it is waited for -- with two sets the loop
  // ran 3100 cycles per step against 1536 of matrix work: 18 % of the requests are cold in L2 and come back after ~3 us), FOUR LDS stages
  // (step s sits in stage s % 4).  A step is four quadrants in snake order -- (A0,B0) (A0,B1) (A1,B1) (A1,B0) -- so that each transition
  // brings ONE new fragment half under the MFMAs of the quadrant before (64 fragment registers live, not 112): step k reads B1, A1, B0
  // again, then -- under its last quadrant -- A0 and B0 of step k + 1 (stashed in step k - 1, behind that step's barrier); between the
  // quadrants set (k + 2) % 4 goes to stage (k + 2) % 4 and is refilled with step k + 6.  One barrier per step.
  // (Reads past the reduction's end land in the buffers' slack: W4_SLACK.)
  W4KLoad l0, l1, l2, l3;
  W4KB xa, ya, xb, yb;      // xa: A0;  ya: A1;  xb / yb: B0 and B1, their roles swapping every step
  W4K_FETCH(l0)
  W4K_FETCH(l1)
  W4K_FETCH(l2)
  W4K_FETCH(l3)
  W4K_WAIT(24, l0);
  W4K_STASH(l0, 0)
  W4K_FETCH(l0)
  W4K_WAIT(24, l1);
  W4K_STASH(l1, 1)
  W4K_FETCH(l1)
  __syncthreads();
  W4K_AH(xa, 0, 0)
  W4K_BH(xb, 0, 0)
  // step k in stage ST, next stage STN; B0 in B0R on entry, B1 goes to B1R; on exit B0 of step k + 1 sits in B1R
#define W4K_FENCE __builtin_amdgcn_sched_barrier(0);   /* the order below IS the schedule: left alone the compiler sinks every fragment read
                                                          to a few MFMAs before its use, and with one wave per SIMD nothing covers the LDS latency */
// Everything that is not an MFMA goes in pieces of FOUR instructions behind groups of four MFMAs (one part product of a quadrant): the matrix
// pipe works 128 cycles on a group while the vector / memory issue it blocks for 32 of them is free for the rest.  (As ONE block between two
// quadrants -- wait, eight staging writes, eight requests, their pointer sums, four fragment reads -- the same instructions cost ~330 cycles
// of a drained pipe per step: 14 of a round's 108 us, measured by leaving them out.)
#define W4K_STASH_A(L, STAGE) { *blk(STAGE, 0, 2 * wave, 0) = (L).a00; *blk(STAGE, 0, 2 * wave, 1) = (L).a01; *blk(STAGE, 0, 2 * wave + 1, 0) = (L).a10; *blk(STAGE, 0, 2 * wave + 1, 1) = (L).a11; }
#define W4K_STASH_B(L, STAGE) { *blk(STAGE, 1, 2 * wave, 0) = (L).b00; *blk(STAGE, 1, 2 * wave, 1) = (L).b01; *blk(STAGE, 1, 2 * wave + 1, 0) = (L).b10; *blk(STAGE, 1, 2 * wave + 1, 1) = (L).b11; }
#define W4K_FETCH_A(L)                                                                                   \
  {                                                                                                      \
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"((L).a00) : "v"(pa0) : "memory");               \
    asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"((L).a01) : "v"(pa0) : "memory");   \
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"((L).a10) : "v"(pa1) : "memory");               \
    asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"((L).a11) : "v"(pa1) : "memory");   \
    pa0 += 2048; pa1 += 2048;                                                                            \
  }
#define W4K_FETCH_B(L)                                                                                   \
  {                                                                                                      \
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"((L).b00) : "v"(pb0) : "memory");               \
    asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"((L).b01) : "v"(pb0) : "memory");   \
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"((L).b10) : "v"(pb1) : "memory");               \
    asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"((L).b11) : "v"(pb1) : "memory");   \
    pb0 += 2048; pb1 += 2048;                                                                            \
  }
#define W4K_STEP(ST, STN, B0R, B1R, LSET, STS)                                                      \
  {                                                                                                 \
    W4K_BH(B1R, ST, 1)                                                                              \
    W4K_FENCE                                                                                       \
    W4K_MAC1(xa, B0R, 0, 0, 1, 0) W4K_FENCE                                                         \
    W4K_AH(ya, ST, 1)             W4K_FENCE                                                         \
    W4K_MAC1(xa, B0R, 0, 0, 0, 1) W4K_FENCE                                                         \
    W4K_MAC1(xa, B0R, 0, 0, 0, 0) W4K_FENCE                                                         \
    W4K_MAC1(xa, B1R, 0, 1, 1, 0) W4K_FENCE                                                         \
    W4K_WAIT(24, LSET);                                                                             \
    W4K_STASH_A(LSET, STS)        W4K_FENCE                                                         \
    W4K_MAC1(xa, B1R, 0, 1, 0, 1) W4K_FENCE                                                         \
    W4K_STASH_B(LSET, STS)        W4K_FENCE                                                         \
    W4K_MAC1(xa, B1R, 0, 1, 0, 0) W4K_FENCE                                                         \
    W4K_FETCH_A(LSET)             W4K_FENCE                                                         \
    W4K_MAC1(ya, B1R, 1, 1, 1, 0) W4K_FENCE                                                         \
    W4K_FETCH_B(LSET)             W4K_FENCE                                                         \
    W4K_MAC1(ya, B1R, 1, 1, 0, 1) W4K_FENCE                                                         \
    W4K_BH(B0R, ST, 0)            W4K_FENCE                                                         \
    W4K_MAC1(ya, B1R, 1, 1, 0, 0) W4K_FENCE                                                         \
    W4K_AH(xa, STN, 0)            W4K_FENCE                                                         \
    W4K_MAC1(ya, B0R, 1, 0, 1, 0) W4K_FENCE                                                         \
    W4K_BH(B1R, STN, 0)           W4K_FENCE                                                         \
    W4K_MAC1(ya, B0R, 1, 0, 0, 1) W4K_FENCE                                                         \
    W4K_MAC1(ya, B0R, 1, 0, 0, 0) W4K_FENCE                                                         \
    __syncthreads();                                                                                \
  }
  for (int k = 0; k < G2; k += 4) {   // (G2 = C / 16 is a multiple of 4)
    W4K_STEP(0, 1, xb, yb, l2, 2)
    W4K_STEP(1, 2, yb, xb, l3, 3)
    W4K_STEP(2, 3, xb, yb, l0, 0)
    W4K_STEP(3, 0, yb, xb, l1, 1)
  }
  W4K_WAIT(0, l0);                    // nothing may still be landing in registers the epilogue reuses
  W4K_WAIT(0, l1);
  W4K_WAIT(0, l2);
  W4K_WAIT(0, l3);
#undef W4K_STEP
#undef W4K_STASH_A
#undef W4K_STASH_B
#undef W4K_FETCH_A
#undef W4K_FETCH_B
#undef W4K_FENCE
#undef W4K_MAC
#undef W4K_MAC1
#undef W4K_AH
#undef W4K_BH
#undef W4K_STASH
  {
    // (the lane's output coordinates are formed HERE, from a lane id the compiler cannot trace back: kept alive across the loop they spill)
    int lane2 = (int)threadIdx.x;
    asm volatile("" : "+v"(lane2));
    const int l31e = lane2 & 31, hie = (lane2 >> 5) & 1;
    const size_t sstride = (size_t)(gm.C >> 5) * 36 * 128;       // floats per sample of M
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rb = 8 * RT + 4 * wr + r;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int cb = 8 * CT + 4 * wc + c;
        float* m0 = M + ((size_t)(rb * 8 + hie) * (gm.C >> 5) + cb) * (36 * 128) + (size_t)comp * 128 + l31e;
#pragma unroll
        for (int q = 0; q < 16; ++q) st_wt(m0 + (size_t)(2 * (q >> 2)) * sstride + (q & 3) * 32, acc[r][c][q] * inv);
      }
    }
  }
}
#undef W4K_FETCH
#undef W4K_WAIT

void launch_w4_gemm_f16_64(const unsigned* Vh, const unsigned* Uh, float* M, const Ctrl* ctrl, const W4Geom& gm, int mode, const int* v_exp,
                           const int* u_exp, unsigned long long* stamps, hipStream_t s) {
  const int grid = (gm.N / 16) * (gm.C >> 6) * 8;
  const size_t lds = 4 * 2048 * sizeof(float);
  // the ring's depth divides the K = 16 steps of the reduction
  if ((gm.C >> 4) % 4 == 0) hipLaunchKernelGGL(k_w4_gemm64h<4>, dim3(grid), dim3(256), lds, s, Vh, Uh, M, ctrl, gm, mode, v_exp, u_exp, stamps);
  else hipLaunchKernelGGL(k_w4_gemm64h<2>, dim3(grid), dim3(256), lds, s, Vh, Uh, M, ctrl, gm, mode, v_exp, u_exp, stamps);
}
// (at cfg 2 the LDS-tiled kernel takes 14.4 us against k_w4_gemm64h's 12.7: profiles/r06_w4h_kernels.txt -- long reductions only)
void launch_w4_gemm_f16_128(const unsigned* Vh, const unsigned* Uh, float* M, const Ctrl* ctrl, const W4Geom& gm, const int* v_exp,
                            const int* u_exp, bool tail, hipStream_t s) {
  static bool attr[MAX_DEVICES] = {};
  const int nT = (gm.N / 32) * (gm.C >> 7);
  const size_t lds = 4 * 16 * 64 * 16;      // four stages of sixteen 1 KB blocks
  allow_full_lds(reinterpret_cast<const void*>(k_w4_gemm128h<2>), attr);
  hipLaunchKernelGGL(k_w4_gemm128h<2>, dim3((tail ? 4 : 32) * nT), dim3(256), lds, s, Vh, Uh, M, ctrl, gm, v_exp, u_exp, tail ? 1 : 0);
}
void launch_w4_gemm_f16_256(const unsigned* Vh, const unsigned* Uh, float* M, const Ctrl* ctrl, const W4Geom& gm, const int* v_exp,
                            const int* u_exp, hipStream_t s) {
  static bool attr[MAX_DEVICES] = {};
  const int nT2 = (gm.N / 64) * (gm.C >> 8);
  allow_full_lds(reinterpret_cast<const void*>(k_w4_gemm256h), attr);
  hipLaunchKernelGGL(k_w4_gemm256h, dim3(32 * nT2), dim3(256), 4 * 32 * 64 * 16, s, Vh, Uh, M, ctrl, gm, v_exp, u_exp);
}

}  // namespace node
