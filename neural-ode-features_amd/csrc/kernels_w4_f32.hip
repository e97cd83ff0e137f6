// Winograd F(4x4,3x3) pipeline, stage 2: the 36 component GEMMs on fp32 MFMA -- k_w4_gemm, k_w4_gemm64, k_w4_gemm_small.
// gfx950 (MI355X / CDNA4) only.  See wino4.h for the data layouts, w4_select.hip for which batch takes which kernel.
#include "w4_gemm.h"

namespace node {

// ----------------------------------------------------------------------------
// k_w4_gemm: M_c[rows, C] = V_c[rows, C] x U_c[C, C] for the 36 components -- the first version, kept for batches that
// are a multiple of 8 but not of 16 (k_w4_gemm64 below is 2 - 4 us faster where it applies).
// Workgroup = one 32-row block x one pair of 32-column blocks x NINE components (grid = N/8 x C/64 x 4): eight
// waves take one component each over the whole K range (two accumulators sharing the row operand), the ninth
// component is cut into eight K slices, one per wave, and summed through LDS -- 288 MFMAs per wave, 576 per SIMD,
// no wave idles.  No operand is shared between waves, so nothing is staged through LDS: every (component, block,
// eight channels) operand is a contiguous 1 KB block and one 16-B load per lane feeds four MFMA k-steps; four
// loads deep in registers.  Per eight MFMAs a wave issues three vector loads and nothing else.
// ----------------------------------------------------------------------------
constexpr int W4_DEPTH = 4;    // operand sets in flight in the main loop (C % 64 == 0: C / 8 is a multiple)
constexpr int W4_SDEPTH = 4;   // ... in a K slice of the shared component

__device__ __forceinline__ void w4_mac(float16_t& acc0, float16_t& acc1, const float4& a, const float4& b0, const float4& b1) {
  acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc1, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc1, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc1, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc1, 0, 0, 0);
}

// acc += V[comp, rb, g0 .. g0+ng) x U[comp, cb0 / cb0+1, g0 .. g0+ng).  A ring of W4_DEPTH operand sets: each set is
// refilled, right behind the MFMAs that consumed it, with the block W4_DEPTH ahead -- unconditionally, so the last
// sets read up to W4_DEPTH blocks past the range (the buffers carry that much slack, see w4_v_elems / w4_u_elems).
template <int D>
struct W4Ring {
  float4 a[D], b0[D], b1[D];
  const float4 *qa, *q0, *q1;
};
// requests in the steady state's order, pinned: the compiler merges the wait state of the loop entry into every
// iteration, so any other order here would make each iteration wait for its youngest request
template <int D>
__device__ __forceinline__ void w4_ring_fill(W4Ring<D>& r, const float* pa, const float* pb0, const float* pb1) {
  r.qa = reinterpret_cast<const float4*>(pa);
  r.q0 = reinterpret_cast<const float4*>(pb0);
  r.q1 = reinterpret_cast<const float4*>(pb1);
#pragma unroll
  for (int i = 0; i < D; ++i) {
    r.a[i] = r.qa[i * 64];
    r.b0[i] = r.q0[i * 64];
    r.b1[i] = r.q1[i * 64];
    __builtin_amdgcn_sched_barrier(0);
  }
  r.qa += D * 64; r.q0 += D * 64; r.q1 += D * 64;
}
// GUARD: ng need not be a multiple of D and nothing is refilled (the K slices of the shared component: ng <= D)
template <int D, bool GUARD>
__device__ __forceinline__ void w4_ring_run(W4Ring<D>& r, float16_t& acc0, float16_t& acc1, int ng) {
  for (int g = 0; g < ng; g += D) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
      if (!GUARD || g + i < ng) w4_mac(acc0, acc1, r.a[i], r.b0[i], r.b1[i]);
      __builtin_amdgcn_sched_barrier(0);   // the refill stays behind the MFMAs that read the old contents
      if (!GUARD) {
        r.a[i] = r.qa[i * 64];
        r.b0[i] = r.q0[i * 64];
        r.b1[i] = r.q1[i * 64];
      }
    }
    r.qa += D * 64; r.q0 += D * 64; r.q1 += D * 64;
  }
}

// AB: timing-only ablation bits (1 no shared component, 2 no main loop, 4 no stores); only AB = 0 is instantiated
template <int AB>
__global__ __launch_bounds__(512) void k_w4_gemm(const float* __restrict__ V, const float* __restrict__ U, float* __restrict__ M,
                                                 const Ctrl* ctrl, W4Geom gm, int xmap) {
  if (ctrl != nullptr && ctrl->done) return;   // a step enqueued past the end of the interval (Ctrl::done)
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [8 waves][2 blocks][4 r4][64 lanes][4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int nCP = gm.C >> 6, nRB = gm.RB;
  // Workgroups b and b + 8 share an XCD (and its L2).  An XCD takes one component group and half of the column
  // pairs for every row block: its filter operands (9 components x nCP/2 pairs) stay resident in its L2 while the
  // row operands stream through, each fetched by two XCDs.
  int cg, rb, cp;
  {
    const int L = blockIdx.x;
    if (xmap == 1 && (nRB & 1) == 0) {   // (A/B) an XCD = one component group x HALF of the row blocks x every column pair
      const int xcd = L & 7, slot = L >> 3;
      cg = xcd >> 1;
      rb = (xcd & 1) * (nRB >> 1) + slot / nCP;
      cp = slot % nCP;
    } else if ((nCP & 1) == 0 && ((nRB * nCP * 4) & 7) == 0) {
      const int xcd = L & 7, slot = L >> 3, half = nCP >> 1;
      cg = xcd >> 1;
      rb = slot / half;
      cp = (xcd & 1) * half + slot % half;
    } else {
      cg = L & 3;
      const int r = L >> 2;
      cp = r % nCP;
      rb = r / nCP;
    }
  }
  const int G8 = gm.G8, CB = gm.C >> 5;
  const int a_off = (((l31 >> 2) * 8) + hi * 4 + (l31 & 3)) * 4;   // lane (row = 4 s + t, k-half hi) inside a V block
  const int b_off = lane * 4;
  auto vblk = [&](int comp) { return V + (((size_t)comp * nRB + rb) * G8) * 256 + a_off; };
  auto ublk = [&](int comp, int cb) { return U + (((size_t)comp * CB + cb) * G8) * 256 + b_off; };

  // --- this wave's own component, whole K range
  const int comp = cg * 9 + wave;
  {
    W4Ring<W4_DEPTH> ring;
    w4_ring_fill(ring, vblk(comp), ublk(comp, 2 * cp), ublk(comp, 2 * cp + 1));
    float16_t acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    if (!(AB & 2)) w4_ring_run<W4_DEPTH, false>(ring, acc0, acc1, G8);
    // M is [n][C/32][36][4 t][32 c] (wino4.h): accumulator register r of a lane holds row (r & 3) + 8 (r >> 2) + 4 hi
    // = tile r & 3 of sample 2 (r >> 2) + hi of this 8-sample row block
    const size_t sstride = (size_t)(gm.C >> 5) * 36 * 128;   // floats per sample
    float* mrow = M + ((size_t)(rb * 8 + hi) * (gm.C >> 5) + 2 * cp) * (36 * 128) + (size_t)comp * 128 + l31;
    if (!(AB & 4)) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float* q = mrow + (size_t)(2 * (r >> 2)) * sstride + (r & 3) * 32;
        q[0] = acc0[r];
        q[36 * 128] = acc1[r];
      }
    } else if (acc0[0] == 12345.f) mrow[0] = acc0[1] + acc1[2];
  }
  // --- the ninth component, shared: K slice [wave * G8/8, (wave+1) * G8/8) per wave, summed through LDS.
  // (Measured: running it first on operands requested together with the main loop's, or first in four waves and
  // last in the other four, with eight operand sets in flight, were both 1.3 - 2 us SLOWER than this order.)
  const int scomp = cg * 9 + 8;
  if (!(AB & 1)) {
    const int ng = G8 >> 3, g0 = wave * ng;
    W4Ring<W4_SDEPTH> sr;
    float16_t s0, s1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
    for (int gs = 0; gs < ng; gs += W4_SDEPTH) {   // (one round at C <= 256)
      w4_ring_fill(sr, vblk(scomp) + (size_t)(g0 + gs) * 256, ublk(scomp, 2 * cp) + (size_t)(g0 + gs) * 256,
                   ublk(scomp, 2 * cp + 1) + (size_t)(g0 + gs) * 256);
      w4_ring_run<W4_SDEPTH, true>(sr, s0, s1, min(W4_SDEPTH, ng - gs));
    }
    float* red = smem + wave * 2048;
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      *reinterpret_cast<float4*>(red + (r4 * 64 + lane) * 4) = make_float4(s0[4 * r4], s0[4 * r4 + 1], s0[4 * r4 + 2], s0[4 * r4 + 3]);
      *reinterpret_cast<float4*>(red + 1024 + (r4 * 64 + lane) * 4) = make_float4(s1[4 * r4], s1[4 * r4 + 1], s1[4 * r4 + 2], s1[4 * r4 + 3]);
    }
  }
  if (!(AB & 1)) {
    __syncthreads();
    const int blk = tid >> 8, r4 = (tid >> 6) & 3;
    float4 s = *reinterpret_cast<const float4*>(smem + blk * 1024 + (r4 * 64 + lane) * 4);
#pragma unroll
    for (int w = 1; w < 8; ++w) {
      const float4 v = *reinterpret_cast<const float4*>(smem + w * 2048 + blk * 1024 + (r4 * 64 + lane) * 4);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    // rows 8 r4 + 4 hi + (0..3) of the block = tiles 0..3 of sample 2 r4 + hi
    float* mrow = M + ((size_t)(rb * 8 + 2 * r4 + hi) * (gm.C >> 5) + 2 * cp + blk) * (36 * 128) + (size_t)scomp * 128 + l31;
    mrow[0] = s.x;
    mrow[32] = s.y;
    mrow[64] = s.z;
    mrow[96] = s.w;
  }
}

// ----------------------------------------------------------------------------
// k_w4_gemm64: the same products on 64 x 64 tiles, FOUR waves per workgroup (one per SIMD, up to 512 registers).
// A wave owns one whole component of its tile -- two row blocks x two column blocks, four accumulators -- so four
// 1 KB requests feed sixteen MFMAs (256 B per MFMA; k_w4_gemm: 384): the operand stream of a CU, which is what
// bounds these K = C products (L2-served: ~70 GB/s per CU, Infinity Cache ~33), shrinks from 864 to 608 KB.
// Eight workgroups share a tile: workgroup j takes components 4j .. 4j+3, and half a tile (32 rows) of component
// 32 + j/2, whose K range its four waves split and sum through LDS -- 512 + 64 MFMAs per wave, 576 per SIMD,
// every SIMD of the chip the same.  Workgroup j of every tile runs on XCD j: that XCD's 4.5 components of V and U
// (3.5 MB at N = 128, C = 256) stay in its L2, so each operand byte leaves HBM / Infinity Cache once per launch.
// Needs N % 16 == 0 and C % 64 == 0.
// ----------------------------------------------------------------------------
constexpr int W4_DEPTH64 = 8;

template <int D>
struct W4Ring4 {
  float4 a0[D], a1[D], b0[D], b1[D];
  const float4 *qa0, *qa1, *qb0, *qb1;
};

template <int AB>
__global__ __launch_bounds__(256) void k_w4_gemm64(const float* __restrict__ V, const float* __restrict__ U, float* __restrict__ M,
                                                   const Ctrl* ctrl, W4Geom gm) {
  if (ctrl != nullptr && ctrl->done) return;   // a step enqueued past the end of the interval (Ctrl::done)
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [4 waves][2 blocks][4 r4][64 lanes][4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int nCT = gm.C >> 6, nRB = gm.RB, G8 = gm.G8, CB = gm.C >> 5;
  const int j = blockIdx.x & 7, tile = blockIdx.x >> 3;
  const int rt = tile / nCT, ct = tile - rt * nCT;
  const int a_off = (((l31 >> 2) * 8) + hi * 4 + (l31 & 3)) * 4;   // lane (row = 4 s + t, k-half hi) inside a V block
  const int b_off = lane * 4;
  auto vblk = [&](int comp, int rb) { return V + (((size_t)comp * nRB + rb) * G8) * 256 + a_off; };
  auto ublk = [&](int comp, int cb) { return U + (((size_t)comp * CB + cb) * G8) * 256 + b_off; };

  // The shared component's first operand sets are requested BEFORE the own component's loop (one wave per SIMD:
  // nothing else would cover their latency behind it), and its MFMAs run while the own component's 18.9 MB of
  // result stores drain.
  const int scomp = 32 + (j >> 1), rb = 2 * rt + (j & 1);
  const int ng = G8 >> 2, g0 = wave * ng;
  const bool early = !(AB & 1) && ng % W4_SDEPTH == 0;
  W4Ring<W4_SDEPTH> sr;
  if (early) {
    w4_ring_fill(sr, vblk(scomp, rb) + (size_t)g0 * 256, ublk(scomp, 2 * ct) + (size_t)g0 * 256, ublk(scomp, 2 * ct + 1) + (size_t)g0 * 256);
    asm volatile("" ::: "memory");   // the compiler may not sink these requests to their first use behind the loop
  }
  // --- this wave's own component: the whole 64 x 64 tile over the whole K range
  {
    const int comp = 4 * j + wave;
    W4Ring4<W4_DEPTH64> r;
    r.qa0 = reinterpret_cast<const float4*>(vblk(comp, 2 * rt));
    r.qa1 = reinterpret_cast<const float4*>(vblk(comp, 2 * rt + 1));
    r.qb0 = reinterpret_cast<const float4*>(ublk(comp, 2 * ct));
    r.qb1 = reinterpret_cast<const float4*>(ublk(comp, 2 * ct + 1));
    // requests in the steady state's order, pinned (see w4_ring_fill)
#pragma unroll
    for (int i = 0; i < W4_DEPTH64; ++i) {
      r.a0[i] = r.qa0[i * 64]; r.a1[i] = r.qa1[i * 64]; r.b0[i] = r.qb0[i * 64]; r.b1[i] = r.qb1[i * 64];
      __builtin_amdgcn_sched_barrier(0);
    }
    r.qa0 += W4_DEPTH64 * 64; r.qa1 += W4_DEPTH64 * 64; r.qb0 += W4_DEPTH64 * 64; r.qb1 += W4_DEPTH64 * 64;
    float16_t c00, c01, c10, c11;
#pragma unroll
    for (int q = 0; q < 16; ++q) { c00[q] = 0.f; c01[q] = 0.f; c10[q] = 0.f; c11[q] = 0.f; }
    if (!(AB & 2))
      for (int g = 0; g < G8; g += W4_DEPTH64) {
#pragma unroll
        for (int i = 0; i < W4_DEPTH64; ++i) {
          const float4 a0 = r.a0[i], a1 = r.a1[i], b0 = r.b0[i], b1 = r.b1[i];
#define W4_STEP(E)                                                          \
  c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.E, b0.E, c00, 0, 0, 0);     \
  c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.E, b1.E, c01, 0, 0, 0);     \
  c10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.E, b0.E, c10, 0, 0, 0);     \
  c11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.E, b1.E, c11, 0, 0, 0);
          W4_STEP(x) W4_STEP(y) W4_STEP(z) W4_STEP(w)
#undef W4_STEP
          __builtin_amdgcn_sched_barrier(0);   // the refill stays behind the MFMAs that read the old contents
          r.a0[i] = r.qa0[i * 64]; r.a1[i] = r.qa1[i * 64]; r.b0[i] = r.qb0[i * 64]; r.b1[i] = r.qb1[i * 64];
        }
        r.qa0 += W4_DEPTH64 * 64; r.qa1 += W4_DEPTH64 * 64; r.qb0 += W4_DEPTH64 * 64; r.qb1 += W4_DEPTH64 * 64;
      }
    if (!(AB & 4)) {
      // M is [n][C/32][36][4 t][32 c] (wino4.h): register q of a lane = tile q & 3 of sample 2 (q >> 2) + hi of its row block
      const size_t sstride = (size_t)(gm.C >> 5) * 36 * 128;   // floats per sample
      float* m0 = M + ((size_t)(rt * 16 + hi) * (gm.C >> 5) + 2 * ct) * (36 * 128) + (size_t)comp * 128 + l31;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        float* o = m0 + (size_t)(2 * (q >> 2)) * sstride + (q & 3) * 32;
        o[0] = c00[q];
        o[36 * 128] = c01[q];
        o[8 * sstride] = c10[q];
        o[8 * sstride + 36 * 128] = c11[q];
      }
    } else if (c00[0] == 12345.f) M[0] = c00[1] + c01[2] + c10[3] + c11[4];
  }
  // --- half a tile of a shared component: rows [32 half, 32 half + 32), K slice [wave G8/4, (wave+1) G8/4) per wave
  if (!(AB & 1)) {
    float16_t s0, s1;
#pragma unroll
    for (int q = 0; q < 16; ++q) { s0[q] = 0.f; s1[q] = 0.f; }
    if (early) {
      w4_ring_run<W4_SDEPTH, false>(sr, s0, s1, ng);
    } else {
      for (int gs = 0; gs < ng; gs += W4_SDEPTH) {
        w4_ring_fill(sr, vblk(scomp, rb) + (size_t)(g0 + gs) * 256, ublk(scomp, 2 * ct) + (size_t)(g0 + gs) * 256,
                     ublk(scomp, 2 * ct + 1) + (size_t)(g0 + gs) * 256);
        w4_ring_run<W4_SDEPTH, true>(sr, s0, s1, min(W4_SDEPTH, ng - gs));
      }
    }
    float* red = smem + wave * 2048;
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      *reinterpret_cast<float4*>(red + (r4 * 64 + lane) * 4) = make_float4(s0[4 * r4], s0[4 * r4 + 1], s0[4 * r4 + 2], s0[4 * r4 + 3]);
      *reinterpret_cast<float4*>(red + 1024 + (r4 * 64 + lane) * 4) = make_float4(s1[4 * r4], s1[4 * r4 + 1], s1[4 * r4 + 2], s1[4 * r4 + 3]);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int u = tid + it * 256;
      const int blk = u >> 8, r4 = (u >> 6) & 3;
      float4 s = *reinterpret_cast<const float4*>(smem + blk * 1024 + (r4 * 64 + lane) * 4);
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const float4 v = *reinterpret_cast<const float4*>(smem + w * 2048 + blk * 1024 + (r4 * 64 + lane) * 4);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      }
      float* mrow = M + ((size_t)(rb * 8 + 2 * r4 + hi) * (gm.C >> 5) + 2 * ct + blk) * (36 * 128) + (size_t)scomp * 128 + l31;
      mrow[0] = s.x;
      mrow[32] = s.y;
      mrow[64] = s.z;
      mrow[96] = s.w;
    }
  }
}

// ----------------------------------------------------------------------------
// k_w4_gemm_small: the component GEMMs of a batch of at most 16 samples (the bs = 1 census, evaluate.py:97-142).  The
// throughput kernels give every wave a whole K range however few rows there are (23.9 us per launch at ONE sample);
// here a workgroup owns ONE 32 x 32 block of one component, its four waves split K (all operand requests of a wave in
// flight at once, 32 MFMAs at C = 256) and meet through LDS: 36 x C/32 x N8/8 workgroups, one memory round trip deep.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_w4_gemm_small(const float* __restrict__ V, const float* __restrict__ U, float* __restrict__ M,
                                                       const Ctrl* ctrl, W4Geom gm) {
  if (ctrl != nullptr && ctrl->done) return;
  __shared__ __attribute__((aligned(16))) float red[4 * 1024];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int CB = gm.C >> 5, G8 = gm.G8;
  const int cb = blockIdx.x % CB, comp = (blockIdx.x / CB) % W4_COMPS, rb = blockIdx.x / (CB * W4_COMPS);
  const int a_off = (((l31 >> 2) * 8) + hi * 4 + (l31 & 3)) * 4;
  const int ng = G8 >> 2, g0 = wave * ng;          // this wave's K quarter (C % 64 == 0: ng is a multiple of 2)
  const float4* pa = reinterpret_cast<const float4*>(V + (((size_t)comp * gm.RB + rb) * G8 + g0) * 256 + a_off);
  const float4* pb = reinterpret_cast<const float4*>(U + (((size_t)comp * CB + cb) * G8 + g0) * 256 + lane * 4);
  float16_t acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  for (int g = 0; g < ng; g += 8) {
    float4 a[8], b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {   // (clamped, not predicated: a masked request makes the compiler wait)
      const int gi = g + i < ng ? g + i : ng - 1;
      a[i] = pa[(size_t)gi * 64];
      b[i] = pb[(size_t)gi * 64];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (g + i < ng) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b[i].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b[i].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, b[i].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, b[i].w, acc, 0, 0, 0);
      }
  }
#pragma unroll
  for (int r4 = 0; r4 < 4; ++r4)
    *reinterpret_cast<float4*>(red + wave * 1024 + (r4 * 64 + lane) * 4) = make_float4(acc[4 * r4], acc[4 * r4 + 1], acc[4 * r4 + 2], acc[4 * r4 + 3]);
  __syncthreads();
  {   // thread (r4 = wave, lane): registers 4 r4 .. 4 r4 + 3 of the block = tiles 0..3 of sample 2 r4 + hi
    const int r4 = wave;
    float4 s = *reinterpret_cast<const float4*>(red + (r4 * 64 + lane) * 4);
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float4 v = *reinterpret_cast<const float4*>(red + w * 1024 + (r4 * 64 + lane) * 4);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    float* mrow = M + ((size_t)(rb * 8 + 2 * r4 + hi) * CB + cb) * (36 * 128) + (size_t)comp * 128 + l31;
    mrow[0] = s.x;
    mrow[32] = s.y;
    mrow[64] = s.z;
    mrow[96] = s.w;
  }
}

void launch_w4_gemm_small(const float* V, const float* U, float* M, const Ctrl* ctrl, const W4Geom& gm, hipStream_t s) {
  hipLaunchKernelGGL(k_w4_gemm_small, dim3(gm.RB * W4_COMPS * (gm.C >> 5)), dim3(256), 0, s, V, U, M, ctrl, gm);
}
void launch_w4_gemm_f32_wide(const float* V, const float* U, float* M, const Ctrl* ctrl, const W4Geom& gm, hipStream_t s) {
  static bool attr[MAX_DEVICES] = {};
  allow_full_lds(reinterpret_cast<const void*>(k_w4_gemm<0>), attr);
  // (xmap = 0: the workgroup -> XCD assignment that keeps an XCD's filter operands in its L2, see the kernel)
  hipLaunchKernelGGL(k_w4_gemm<0>, dim3(gm.RB * (gm.C >> 6) * 4), dim3(512), 8 * 2048 * sizeof(float), s, V, U, M, ctrl, gm, 0);
}
void launch_w4_gemm_f32_64(const float* V, const float* U, float* M, const Ctrl* ctrl, const W4Geom& gm, hipStream_t s) {
  hipLaunchKernelGGL(k_w4_gemm64<0>, dim3((gm.N / 16) * (gm.C >> 6) * 8), dim3(256), 4 * 2048 * sizeof(float), s, V, U, M, ctrl, gm);
}

}  // namespace node
