// Winograd F(4x4,3x3) pipeline, stage 2: MEASURED-AND-REJECTED variants of k_w4_gemm64b and the switches of the
// timing diagnostics.  Compiled and linked into libnode_hip_diag.so only (build.py --diag; tools/ and the `-m diag` tests load
// it with NODE_HIP_DIAG=1): the product library contains none of this file.  w4_select.hip reaches it through one hook
// (w4_diag_switches, launch_w4_gemm_variant).  gfx950 (MI355X / CDNA4) only.
#include "w4_gemm.h"
#include <cstdlib>

namespace node {

// ----------------------------------------------------------------------------
// k_w4_gemm32b (C = 256, NODE_TUNE_W4_HALF): k_w4_gemm64b's products with HALF-HEIGHT tiles and TWO waves per SIMD.
// What the counters say about k_w4_gemm64b (profiles/r05_pmc_w4_limiter.txt): the matrix pipe is busy 45 % of a wave's life --
// ~75 % inside the K loop, idle through a prologue (first operands: L2 latency) and an epilogue (stores, shared component,
// LDS reduction) that one tile per wave at one wave per SIMD cannot overlap with anything; neither the texture path nor the
// fabric is saturated.  Here a wave owns a 32 x 64 tile (one row block, two column blocks: 32 + 128 ring registers instead
// of 64 + 160), the kernel fits 256 registers, and a SIMD holds two waves of two different workgroups: one's prologue and
// epilogue run under the other's K loop.  Twice the workgroups (N / 8 row tiles x 4 column tiles x 8), each streaming the same
// filter blocks for half the rows (L1 -> L2 requests of the filter operand double: the texture path has the room).  The
// shared component 32 + j / 2 is dealt in 32 x 32 blocks (one per workgroup, K range cut over the four waves as before).
// Every output element is the same sum in the same order as in k_w4_gemm64b: bit-identical.
// MEASURED AND REJECTED (round 5, profiles/r05_w4_half_ab.txt): 24.3 us against 21.1 us by HIP events in the cfg-2 bench loop
// (24 300 vs 24 880 images/s, cfg 3 18 090 vs 18 560): the second wave's K loop does not hide the first one's prologue --
// both waves of a SIMD share ONE matrix pipe, so two K loops side by side each run at half rate, and the filter operand's
// requests double.  Diagnostics library only.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void k_w4_gemm32b(const float* __restrict__ V, const unsigned short* __restrict__ Ub, float* __restrict__ M,
                                                       const Ctrl* ctrl, W4Geom gm) {
  if (ctrl != nullptr && ctrl->done) return;   // a step enqueued past the end of the interval (Ctrl::done)
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [4 waves][4 r4][64 lanes][4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int nRB = gm.RB, G8 = gm.G8, G2 = G8 >> 1, CB = gm.C >> 5;      // C = 256: four 64-column tiles, eight 32-column blocks
  const int j = blockIdx.x & 7, tile = blockIdx.x >> 3;
  const int rb = tile >> 2, ct = tile & 3;                                // 32-row block, the workgroup's place among four
  const int a_off = (((l31 >> 2) * 8) + hi * 4 + (l31 & 3)) * 4;
  auto vblk = [&](int comp, int r) { return reinterpret_cast<const float4*>(V + (((size_t)comp * nRB + r) * G8) * 256 + a_off); };
  auto ublk = [&](int comp, int cb) { return reinterpret_cast<const w4_u32x4*>(Ub) + (((size_t)comp * CB + cb) * G2) * 192 + lane; };
  const size_t sstride = (size_t)CB * 36 * 128;   // floats per sample of M
  {
    // own component 4 j + ct (the workgroup's place names it, as NODE_TUNE_W4_SHAREV = 1 does in k_w4_gemm64b): the four waves walk
    // the same V block in lock-step, wave w multiplies it with column tile w
    const int comp = 4 * j + ct;
    W4BPtrs p;
    p.a[0] = vblk(comp, rb); p.a[1] = p.a[0];
    p.b[0] = ublk(comp, 2 * wave); p.b[1] = ublk(comp, 2 * wave + 1);
    float16_t acc[2][2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[0][c][q] = 0.f;
    w4b_run<W4B_DEPTH, 1>(acc, p, 0, G2);
    float* m0 = M + ((size_t)(rb * 8 + hi) * CB + 2 * wave) * (36 * 128) + (size_t)comp * 128 + l31;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      float* o = m0 + (size_t)(2 * (q >> 2)) * sstride + (q & 3) * 32;
      st_wt(o, acc[0][0][q]);
      st_wt(o + 36 * 128, acc[0][1][q]);
    }
  }
  {
    // a 32 x 32 block of the shared component: rows rb, column block 2 ct + (j & 1); K range [wave G2 / 4, (wave + 1) G2 / 4)
    const int scomp = 32 + (j >> 1), cb = 2 * ct + (j & 1);
    const int ng = G2 >> 2, g0 = wave * ng;
    W4BPtrs p;
    p.a[0] = vblk(scomp, rb); p.a[1] = p.a[0];
    p.b[0] = ublk(scomp, cb); p.b[1] = p.b[0];
    float16_t acc[2][2];
#pragma unroll
    for (int q = 0; q < 16; ++q) { acc[0][0][q] = 0.f; acc[0][1][q] = 0.f; }
    // (one column block: the second accumulator of w4b_mac<1> multiplies the same block again and is dropped -- 12 spare MFMAs
    //  per K step of a phase that is 1 / 9 of the work, for one code path)
    if (ng % 4 == 0) w4b_run<4, 1>(acc, p, g0, ng);
    else if (ng % 2 == 0) w4b_run<2, 1>(acc, p, g0, ng);
    else w4b_run<1, 1>(acc, p, g0, ng);
    float* red = smem + wave * 1024;
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4)
      *reinterpret_cast<float4*>(red + (r4 * 64 + lane) * 4) =
          make_float4(acc[0][0][4 * r4], acc[0][0][4 * r4 + 1], acc[0][0][4 * r4 + 2], acc[0][0][4 * r4 + 3]);
    __syncthreads();
    const int r4 = wave;      // 256 threads = 4 r4 x 64 lanes
    float4 sacc = *reinterpret_cast<const float4*>(smem + (r4 * 64 + lane) * 4);
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float4 v = *reinterpret_cast<const float4*>(smem + w * 1024 + (r4 * 64 + lane) * 4);
      sacc.x += v.x; sacc.y += v.y; sacc.z += v.z; sacc.w += v.w;
    }
    float* mrow = M + ((size_t)(rb * 8 + 2 * r4 + hi) * CB + cb) * (36 * 128) + (size_t)scomp * 128 + l31;
    st_wt(mrow, sacc.x);
    st_wt(mrow + 32, sacc.y);
    st_wt(mrow + 64, sacc.z);
    st_wt(mrow + 96, sacc.w);
  }
}

// ----------------------------------------------------------------------------
// k_w4_gemm64l (NODE_TUNE_W4_LDS, C = 256, N % 32 == 0): k_w4_gemm64b's products with the own component's operands brought into
// the CU ONCE.  What bounds k_w4_gemm64b is the bytes its waves load into registers (every operand block aliased onto one
// 80 KB footprint -- all L2 hits -- it takes 17.3 instead of 18.5 us): 160 KB per wave, 640 KB per CU for the own
// component.  Here a workgroup takes a 128 x 128 tile of one component (wave (r, c) its 64 x 64 quarter, as NODE_TUNE_W4_SHAREV = 2)
// and the 320 KB of operands of that tile arrive by LDS-DMA (global_load_lds_dwordx4: no registers, no staging instructions)
// in a ring of W4L_NS K = 16 steps of 20 KB (V: 4 row blocks x 2 KB fp32; U: 4 column blocks x 3 KB triples), W4L_D steps in
// flight; the LDS image of a block is in READER-lane order (the permutation sits on the DMA's per-lane source address), so a
// fragment is one conflict-free ds_read_b128.  One raw s_barrier per step behind a counted s_waitcnt vmcnt (never 0 inside the
// loop: cdna_hip_programming.md, Pipelining across barriers); a slot is refilled D + 1 steps after its reads were waited for.
// The shared component (1/9 of the work, no operand shared between waves) keeps k_w4_gemm64b's register path and early requests.
// ----------------------------------------------------------------------------
constexpr int W4L_SPS = 2;                          // K steps per ring slot = per barrier
constexpr int W4L_NS = 4, W4L_D = 3, W4L_STEP = 20 * 1024, W4L_SLOT = W4L_SPS * W4L_STEP, W4L_STEPS = 16, W4L_SLOTS = W4L_STEPS / W4L_SPS;
// one LDS-DMA piece as inline asm: the compiler, which does not count asm memory operations, then neither drains the ring
// (`s_waitcnt vmcnt(0)`) in front of every fragment read -- with the builtin it does: it cannot tell the reads from the pieces in
// flight -- nor knows of it: the counted waits of the loop are the only ordering (cdna_hip_programming.md 5.7: M0 is written in the
// statement that reads it)
__device__ __forceinline__ void w4l_dma(const unsigned char* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void w4l_wait_vm(int n) {   // (n is a compile-time constant after unrolling)
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
    case 15: asm volatile("s_waitcnt vmcnt(15)" ::: "memory"); break;
    case 20: asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); break;
    case 25: asm volatile("s_waitcnt vmcnt(25)" ::: "memory"); break;
    case 30: asm volatile("s_waitcnt vmcnt(30)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}
__global__ __launch_bounds__(256) void k_w4_gemm64l(const float* __restrict__ V, const unsigned short* __restrict__ Ub, float* __restrict__ M,
                                                    const Ctrl* ctrl, W4Geom gm, unsigned long long* stamps) {
  if (ctrl != nullptr && ctrl->done) return;   // a step enqueued past the end of the interval (Ctrl::done)
  extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];   // [W4L_NS][20 KB]; the shared component's reduction in slots 2, 3
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned long long* stp = stamps != nullptr ? stamps + ((size_t)blockIdx.x * 4 + wave) * 16 : nullptr;
  w4_stamp(stp, 0);
  const int l31 = lane & 31, hi = lane >> 5;
  const int nCT = gm.C >> 6, nRB = gm.RB, G8 = gm.G8, G2 = G8 >> 1, CB = gm.C >> 5;
  const int j = blockIdx.x & 7, tile = blockIdx.x >> 3;
  const int rt = tile / nCT, ct = tile - rt * nCT;
  const int a_off = (((l31 >> 2) * 8) + hi * 4 + (l31 & 3)) * 4;   // lane (row = 4 s + t, k-half hi) inside a V block
  auto vblk = [&](int comp, int rb) { return reinterpret_cast<const float4*>(V + (((size_t)comp * nRB + rb) * G8) * 256 + a_off); };
  auto ublk = [&](int comp, int cb) { return reinterpret_cast<const w4_u32x4*>(Ub) + (((size_t)comp * CB + cb) * G2) * 192 + lane; };

  // the shared component's operands, requested first (k_w4_gemm64b)
  constexpr int SH = 4;
  W4BStage shr[SH];
  {
    const int scomp = 32 + (j >> 1), srb = 2 * rt + (j & 1);
    W4BPtrs sp;
    sp.a[0] = vblk(scomp, srb); sp.a[1] = sp.a[0];
    sp.b[0] = ublk(scomp, 2 * ct); sp.b[1] = ublk(scomp, 2 * ct + 1);
#pragma unroll
    for (int i = 0; i < SH; ++i) {
      w4b_load<1>(shr[i], sp, wave * SH + i);
      __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("" ::: "memory");
  }

  // --- own component: the 128 x 128 tile (RT, CT) of component comp; wave (wr, wc) multiplies its 64 x 64 quarter
  const int comp = 4 * j + (tile & 3), RT = tile >> 3, CT = (tile >> 2) & 1;
  const int wr = wave >> 1, wc = wave & 1;
  // the five of a step's twenty 1-KB pieces this wave brings: pieces 0 .. 7 = V (row block p / 2, g block p % 2), 8 .. 19 = U
  // (column block (p - 8) / 3, part (p - 8) % 3); a piece's source advances by 2 KB (V) / 3 KB (U) per step
  const unsigned char* src[5];
  int adv[5], dst[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int p = 5 * wave + i;
    if (p < 8) {
      src[i] = reinterpret_cast<const unsigned char*>(vblk(comp, 4 * RT + (p >> 1))) + (p & 1) * 1024;
      adv[i] = 2048;
    } else {
      const int q = p - 8;
      src[i] = reinterpret_cast<const unsigned char*>(ublk(comp, 4 * CT + q / 3)) + (q % 3) * 1024;
      adv[i] = 3072;
    }
    dst[i] = p * 1024;
  }
  const unsigned slot0 = (unsigned)(size_t)(w4_lds_ptr_t)lsm;   // LDS byte address of the ring
  auto issue = [&](int sl) {                                      // ring slot sl = K steps [SPS sl, SPS sl + SPS)
#pragma unroll
    for (int k = 0; k < W4L_SPS; ++k) {
      const int step = sl * W4L_SPS + k;
#pragma unroll
      for (int i = 0; i < 5; ++i)
        w4l_dma(src[i] + (size_t)step * adv[i], slot0 + (unsigned)((sl % W4L_NS) * W4L_SLOT + k * W4L_STEP + dst[i]));
    }
  };
  auto fetch = [&](W4BStage& st, int step) {
    const unsigned char* slot = lsm + ((step / W4L_SPS) % W4L_NS) * W4L_SLOT + (step % W4L_SPS) * W4L_STEP + lane * 16;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int g = 0; g < 2; ++g) st.a[r][g] = *reinterpret_cast<const float4*>(slot + ((2 * wr + r) * 2 + g) * 1024);
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int q = 0; q < 3; ++q) st.b[c][q] = *reinterpret_cast<const w4_u32x4*>(slot + 8192 + ((2 * wc + c) * 3 + q) * 1024);
  };
  {
    float16_t acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[r][c][q] = 0.f;
#pragma unroll
    for (int sp = 0; sp < W4L_D; ++sp) issue(sp);
    w4_stamp(stp, 1);
    W4BStage st[2];
    w4l_wait_vm(5 * W4L_SPS * (W4L_D - 1));
    __builtin_amdgcn_s_barrier();
    issue(W4L_D);
    fetch(st[0], 0);
    W4Split cur[2], nxt[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) cur[r] = w4_split8(st[0].a[r][0], st[0].a[r][1]);
#pragma unroll
    for (int g = 0; g < W4L_STEPS; ++g) {
      if (g == 4) w4_stamp(stp, 2);
      W4BStage& cs = st[g & 1];
      W4BStage& ns = st[(g + 1) & 1];
      if (g + 1 < W4L_STEPS) {
        if ((g + 1) % W4L_SPS == 0) {                     // step g + 1 opens ring slot S
          const int S = (g + 1) / W4L_SPS;
          const int newest = (S + W4L_D - 1 < W4L_SLOTS - 1) ? S + W4L_D - 1 : W4L_SLOTS - 1;   // the youngest slot whose pieces are issued
          w4l_wait_vm(5 * W4L_SPS * (newest - S));            // this wave's pieces of slot S have landed
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // ... and its reads of slot S - 1 are in registers (that slot is refilled next)
          __builtin_amdgcn_s_barrier();
          if (S + W4L_D < W4L_SLOTS) issue(S + W4L_D);
        }
        fetch(ns, g + 1);
      }
      w4b_mac<2>(acc, cur, cs);
      if (g + 1 < W4L_STEPS) {
#pragma unroll
        for (int r = 0; r < 2; ++r) nxt[r] = w4_split8(ns.a[r][0], ns.a[r][1]);
        __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);    // eight MFMAs cover the fragment reads' latency ...
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // ... then one MFMA,
          __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);  //     up to six VALU instructions of the next step's split
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r = 0; r < 2; ++r) cur[r] = nxt[r];
    }
    w4_stamp(stp, 3);
    const int ort = 2 * RT + wr, oct = 2 * CT + wc;
    const size_t sstride = (size_t)(gm.C >> 5) * 36 * 128;   // floats per sample of M
    float* m0 = M + ((size_t)(ort * 16 + hi) * (gm.C >> 5) + 2 * oct) * (36 * 128) + (size_t)comp * 128 + l31;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      float* o = m0 + (size_t)(2 * (q >> 2)) * sstride + (q & 3) * 32;
      st_wt(o, acc[0][0][q]);
      st_wt(o + 36 * 128, acc[0][1][q]);
      st_wt(o + 8 * sstride, acc[1][0][q]);
      st_wt(o + 8 * sstride + 36 * 128, acc[1][1][q]);
    }
    w4_stamp(stp, 4);
  }
  // --- half a tile of a shared component (k_w4_gemm64b): rows [32 half, 32 half + 32), K range of wave `wave`
  {
    const int scomp = 32 + (j >> 1), rb = 2 * rt + (j & 1);
    float16_t acc[2][2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[0][c][q] = 0.f;
    W4Split cs[2];
#pragma unroll
    for (int i = 0; i < SH; ++i) {
      cs[0] = w4_split8(shr[i].a[0][0], shr[i].a[0][1]);
      w4b_mac<1>(acc, cs, shr[i]);
    }
    w4_stamp(stp, 5);
    float* smem = reinterpret_cast<float*>(lsm + 1 * W4L_SLOT);   // (ring slot 1, last K steps 10 and 11: read long ago by every wave)
    float* red = smem + wave * 2048;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4)
        *reinterpret_cast<float4*>(red + c * 1024 + (r4 * 64 + lane) * 4) =
            make_float4(acc[0][c][4 * r4], acc[0][c][4 * r4 + 1], acc[0][c][4 * r4 + 2], acc[0][c][4 * r4 + 3]);
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
      st_wt(mrow, s.x);
      st_wt(mrow + 32, s.y);
      st_wt(mrow + 64, s.z);
      st_wt(mrow + 96, s.w);
    }
  }
  if (stp != nullptr) {
    w4_stamp(stp, 6);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    w4_stamp(stp, 7);
  }
}

// acc += a * b over one K = 16 step, smallest products first
__device__ __forceinline__ void w4_mac6(float16_t& acc, const W4Split& a, const w4_u32x4& bh, const w4_u32x4& bm, const w4_u32x4& bl) {
  const w4_bf16x8 Bh = __builtin_bit_cast(w4_bf16x8, bh), Bm = __builtin_bit_cast(w4_bf16x8, bm), Bl = __builtin_bit_cast(w4_bf16x8, bl);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.l, Bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, Bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, Bm, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, Bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, Bm, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, Bh, acc, 0, 0, 0);
}

// ----------------------------------------------------------------------------
// k_w4_gemm64k (NODE_TUNE_W4_KSPLIT, C = 256, N % 16 == 0): k_w4_gemm64b's products with TWO waves per SIMD.  The timeline of
// k_w4_gemm64b (tools/w4_stamps.py): the chip holds ~1.65 GHz in the launch, where the 432 MFMAs of a wave are
// 8.4 us and the 768 KB a CU's waves request are 7.5 us of its texture path (64 B per clock) -- but with one wave per SIMD the two
// do not overlap: a wave that stands in a request (the path's queue is full) or in a wait issues no MFMA.  Here every 64 x 64 tile
// of a component is cut in two K halves, one wave each, so a SIMD holds two waves (<= 256 registers: a ring of two K steps
// instead of four -- the requests in flight per SIMD stay what they were) and one multiplies while the other stands.
//   workgroup (512 of them, two per CU) = component 4 j + c4, row tile rt, column tiles 2 p and 2 p + 1: wave 2 t + h = K half h of
//   tile t (the two tiles walk the same V blocks); the halves meet in LDS: wave h keeps row block h of the tile, hands the other
//   one over (8 KB), adds its partner's and stores 32 x 64 results.  The four K-sliced components (32 + j / 2): a 32 x 32 piece per
//   workgroup, four K steps per wave, summed through LDS as in k_w4_gemm64b.  Sums of two K halves: not bit-identical to
//   k_w4_gemm64b's single chain (same error against fp64).
// ----------------------------------------------------------------------------
struct W4KStage { float4 a[2]; w4_u32x4 b[3]; };
__global__ __launch_bounds__(256, 2) void k_w4_gemm64k(const float* __restrict__ V, const unsigned short* __restrict__ Ub, float* __restrict__ M,
                                                       const Ctrl* ctrl, W4Geom gm, unsigned long long* stamps) {
  if (ctrl != nullptr && ctrl->done) return;   // a step enqueued past the end of the interval (Ctrl::done)
  extern __shared__ __attribute__((aligned(16))) float smem[];   // 32 KB: [4 waves][2 blocks][4 r4][64 lanes][4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long* st = stamps != nullptr ? stamps + ((size_t)blockIdx.x * 4 + wave) * 16 : nullptr;
  w4_stamp(st, 0);
  const int l31 = lane & 31, hi = lane >> 5;
  const int nRB = gm.RB, G8 = gm.G8, G2 = G8 >> 1, CB = gm.C >> 5;
  const int j = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const int a_off = (((l31 >> 2) * 8) + hi * 4 + (l31 & 3)) * 4;   // lane (row = 4 s + t, k-half hi) inside a V block
  auto vblk = [&](int comp, int rb) { return reinterpret_cast<const float4*>(V + (((size_t)comp * nRB + rb) * G8) * 256 + a_off); };
  auto ublk = [&](int comp, int cb) { return reinterpret_cast<const w4_u32x4*>(Ub) + (((size_t)comp * CB + cb) * G2) * 192 + lane; };
  const size_t sstride = (size_t)(gm.C >> 5) * 36 * 128;   // floats per sample of M

  // the K-sliced component's piece of this workgroup: rows rbs (32), column block cbs (32), K steps [4 wave, 4 wave + 4)
  const int scomp = 32 + (j >> 1);
  const int rbs = 2 * (idx >> 3) + (j & 1), cbs = 2 * ((idx >> 1) & 3) + (idx & 1);
  const int SG = G2 >> 2;                        // its K steps per wave
  const float4* sa = vblk(scomp, rbs) + (size_t)(2 * wave * SG) * 64;
  const w4_u32x4* sb = ublk(scomp, cbs) + (size_t)(3 * wave * SG) * 64;
  auto snext = [&](W4KStage& s) {
    s.a[0] = sa[0]; s.a[1] = sa[64];
#pragma unroll
    for (int q = 0; q < 3; ++q) s.b[q] = sb[q * 64];
    sa += 128; sb += 192;
  };

  // --- own component: K half h of the 64 x 64 tile (rt, 2 p + t)
  const int comp = 4 * j + (idx & 3), rt = idx >> 3, t = wave >> 1, h = wave & 1;
  const int ct = 2 * ((idx >> 2) & 1) + t;
  W4KStage sring[2];
  {
    W4BPtrs p;
    p.a[0] = vblk(comp, 2 * rt); p.a[1] = vblk(comp, 2 * rt + 1);
    p.b[0] = ublk(comp, 2 * ct); p.b[1] = ublk(comp, 2 * ct + 1);
    float16_t acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[r][c][q] = 0.f;
    w4b_run<2, 2, 0>(acc, p, h * (G2 >> 1), G2 >> 1, st);
    // the K-sliced piece's first two steps are requested now: they arrive under the exchange and the stores
    snext(sring[0]);
    snext(sring[1]);
    asm volatile("" ::: "memory");
    // the halves meet: wave h hands row block 1 - h over and keeps row block h (h is wave-uniform: two straight-line copies, the
    // accumulators stay in registers)
    float* mine = smem + wave * 2048;
    const float* theirs = smem + (wave ^ 1) * 2048;
    auto give = [&](const float16_t (&g)[2]) {
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
          *reinterpret_cast<float4*>(mine + c * 1024 + (r4 * 64 + lane) * 4) = make_float4(g[c][4 * r4], g[c][4 * r4 + 1], g[c][4 * r4 + 2], g[c][4 * r4 + 3]);
    };
    if (h) give(acc[0]); else give(acc[1]);
    __syncthreads();
    float* m0 = M + ((size_t)(rt * 16 + hi) * (gm.C >> 5) + 2 * ct) * (36 * 128) + (size_t)comp * 128 + l31 + (size_t)h * 8 * sstride;
    auto keep = [&](const float16_t (&k)[2], bool first) {   // first: this wave holds K half 0 (the sum is half 0 + half 1 either way)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const float4 o = *reinterpret_cast<const float4*>(theirs + c * 1024 + (r4 * 64 + lane) * 4);
          float* o0 = m0 + (size_t)(2 * r4) * sstride + c * (36 * 128);
          st_wt(o0, first ? k[c][4 * r4] + o.x : o.x + k[c][4 * r4]);
          st_wt(o0 + 32, first ? k[c][4 * r4 + 1] + o.y : o.y + k[c][4 * r4 + 1]);
          st_wt(o0 + 64, first ? k[c][4 * r4 + 2] + o.z : o.z + k[c][4 * r4 + 2]);
          st_wt(o0 + 96, first ? k[c][4 * r4 + 3] + o.w : o.w + k[c][4 * r4 + 3]);
        }
    };
    if (h) keep(acc[1], false); else keep(acc[0], true);
    w4_stamp(st, 4);
  }
  // --- the K-sliced component's piece
  {
    float16_t acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    for (int g = 0; g < SG; g += 2) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const W4Split as = w4_split8(sring[i].a[0], sring[i].a[1]);
        w4_mac6(acc, as, sring[i].b[0], sring[i].b[1], sring[i].b[2]);
        __builtin_amdgcn_sched_barrier(0);
        if (g + 2 + i < SG) snext(sring[i]);
      }
    }
    w4_stamp(st, 5);
    __syncthreads();                 // (the exchange's reads of smem are done)
    float* red = smem + wave * 1024;
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4)
      *reinterpret_cast<float4*>(red + (r4 * 64 + lane) * 4) = make_float4(acc[4 * r4], acc[4 * r4 + 1], acc[4 * r4 + 2], acc[4 * r4 + 3]);
    __syncthreads();
    {
      const int r4 = wave;
      float4 s = *reinterpret_cast<const float4*>(smem + (r4 * 64 + lane) * 4);
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const float4 v = *reinterpret_cast<const float4*>(smem + w * 1024 + (r4 * 64 + lane) * 4);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      }
      float* mrow = M + ((size_t)(rbs * 8 + 2 * r4 + hi) * (gm.C >> 5) + cbs) * (36 * 128) + (size_t)scomp * 128 + l31;
      st_wt(mrow, s.x);
      st_wt(mrow + 32, s.y);
      st_wt(mrow + 64, s.z);
      st_wt(mrow + 96, s.w);
    }
  }
  if (st != nullptr) {
    w4_stamp(st, 6);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    w4_stamp(st, 7);
  }
}

// ---- the hook of w4_select.hip
void w4_diag_switches(W4Switches& sw) {
  sw.early = env_int("NODE_TUNE_W4_EARLY", 0);
  const char* e = getenv("NODE_TUNE_W4_STAMPS");
  sw.stamps = e != nullptr ? reinterpret_cast<unsigned long long*>(strtoull(e, nullptr, 0)) : nullptr;
}
// a batch the selector gave to k_w4_gemm64b: true when a variant took it instead (same operands: fp32 rows, filter triples)
bool launch_w4_gemm_variant(const W4Switches& sw, const float* V, const unsigned short* Ub, float* M, const Ctrl* ctrl, const W4Geom& gm,
                            hipStream_t s) {
  const int N = gm.N, C = gm.C;
  if (env_int("NODE_TUNE_W4_KSPLIT", 0) != 0 && C == 256) {   // two waves per SIMD, a tile's K range in two halves
    hipLaunchKernelGGL(k_w4_gemm64k, dim3(64 * (N / 16)), dim3(256), 8 * 1024 * sizeof(float), s, V, Ub, M, ctrl, gm, sw.stamps);
    return true;
  }
  if (env_int("NODE_TUNE_W4_LDS", 0) != 0 && C == 256 && N % 32 == 0) {      // the own component's operands through an LDS-DMA ring
    static bool attrl[MAX_DEVICES] = {};
    allow_full_lds(reinterpret_cast<const void*>(k_w4_gemm64l), attrl);
    hipLaunchKernelGGL(k_w4_gemm64l, dim3((N / 16) * (C >> 6) * 8), dim3(256), (size_t)W4L_NS * W4L_SLOT, s, V, Ub, M, ctrl, gm, sw.stamps);
    return true;
  }
  if (env_int("NODE_TUNE_W4_HALF", 0) != 0 && C == 256 && sw.sharev == 1) {    // half-height tiles, two waves per SIMD (bit-identical)
    hipLaunchKernelGGL(k_w4_gemm32b, dim3((N / 8) * 4 * 8), dim3(256), 4 * 1024 * sizeof(float), s, V, Ub, M, ctrl, gm);
    return true;
  }
  return false;
}

}  // namespace node
