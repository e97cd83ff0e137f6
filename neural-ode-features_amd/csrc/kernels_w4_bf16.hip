// Winograd F(4x4,3x3) pipeline, stage 2: the 36 component GEMMs on bf16 TRIPLES at fp32 accuracy -- k_w4_gemm64b (operands
// straight from L2) and k_w4_gemm128b (LDS-tiled, long reductions).  gfx950 (MI355X / CDNA4) only.  See wino4.h for the data
// layouts, w4_gemm.h for the split and the register ring, w4_select.hip for which batch takes which kernel.
#include "w4_gemm.h"

namespace node {

// ----------------------------------------------------------------------------
// k_w4_gemm64b: k_w4_gemm64's products on the bf16 matrix pipe at fp32 accuracy.  Every fp32 operand is split EXACTLY
// into three bf16 parts (x = h + m + l: 3 x 8 mantissa bits; U once per solve by k_w4_pack, V in registers here with
// v_cvt_pk_bf16_f32), and a K = 16 step of a 32 x 32 block is six v_mfma_f32_32x32x16_bf16 -- hh, hm, mh, mm, hl, lh,
// fp32 accumulation; the dropped products ml, lm, ll are <= 2^-24 of the result -- instead of eight
// v_mfma_f32_32x32x2_f32: 192 instead of 512 matrix-pipe cycles.  Measured against an fp64 product the error is that
// of the fp32 MFMA chain (tools/bf16x3 check in tests/test_gpu_w4.py: same 3.2e-6-of-max|y| convolution error).
// Same decomposition, layouts of V and M, and XCD placement as k_w4_gemm64; a lane's eight K values of a step are
// channels {8 g + 4 hi + e} of TWO consecutive g blocks (two of the 16-B loads the fp32 kernel issues too).
// 24.4 -> 19.6 us per launch at cfg 2.  (Measured and not kept, end of round 3: this loop's forty operand requests as inline asm
// with ONE exact wait per step -- s_waitcnt vmcnt(26), where the compiler's placement waits for up to vmcnt(20) -- as in
// k_w4_gemm128b below, where that gave 8 %: 22.5 us by events either way at cfg 2, whose 16 steps per tile are not what bounds it.)  (Measured and not kept: the same products with the operands shared through LDS
// -- 128 x 128 tiles per workgroup, three LDS buffers, fragments prefetched under the MFMAs, L2 -> CU traffic 448
// instead of 768 KB per CU -- 21.5 - 22.8 us: what bounds the launch now is its 52 MB through the fabric plus fill and
// drain, not the per-CU operand stream.)
// ----------------------------------------------------------------------------
template <int AB>
__global__ __launch_bounds__(256) void k_w4_gemm64b(const float* __restrict__ V, const unsigned short* __restrict__ Ub, float* __restrict__ M,
                                                    const Ctrl* ctrl, W4Geom gm, int mode, unsigned long long* stamps) {
  if (ctrl != nullptr && ctrl->done) return;   // a step enqueued past the end of the interval (Ctrl::done)
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [4 waves][2 blocks][4 r4][64 lanes][4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long* st = stamps != nullptr ? stamps + ((size_t)blockIdx.x * 4 + wave) * 16 : nullptr;
  w4_stamp(st, 0);
  const int l31 = lane & 31, hi = lane >> 5;
  const int nCT = gm.C >> 6, nRB = gm.RB, G8 = gm.G8, G2 = G8 >> 1, CB = gm.C >> 5;
  const int j = blockIdx.x & 7, tile = blockIdx.x >> 3;
  const int rt = tile / nCT, ct = tile - rt * nCT;
  const int a_off = (((l31 >> 2) * 8) + hi * 4 + (l31 & 3)) * 4;   // lane (row = 4 s + t, k-half hi) inside a V block
  constexpr int padv = 0, padu = 0;   // (the operand blocks keep their power-of-two spacing)
  auto vblk = [&](int comp, int rb) {
    const size_t b = (size_t)comp * nRB + rb;
    return reinterpret_cast<const float4*>(V + (b * G8) * 256 - b * padv * 256 + a_off);
  };
  auto ublk = [&](int comp, int cb) {
    const size_t b = (size_t)comp * CB + cb;
    return reinterpret_cast<const w4_u32x4*>(Ub) + (b * G2) * 192 - b * padu * 64 + lane;
  };

  // The shared component's operands (four K = 16 steps per wave at C = 256: 128 registers -- the kernel runs one wave per
  // SIMD, so the file's other half is free) are requested BEFORE the own component's loop: nothing else would cover their
  // latency behind it (the ablation of DESIGN.md 4.7: the second ring fill cost ~3 of the shared component's 4.7 us).
  constexpr int SH = 4;
  const bool early = !(AB & 1) && !(AB & 2) && !(AB & 8) && (G2 >> 2) == SH;
  // mode bit 3 (NODE_TUNE_W4_EARLY = 1): ... and BEHIND the ring's first four steps, whose operands the first MFMA waits for (the
  // texture path takes a CU's requests at 64 B per clock: 32 KB per wave in front of them is ~1 us)
  W4BStage shr[SH];
  auto request_shared = [&]() {
    const int scomp = 32 + (j >> 1), srb = 2 * rt + (j & 1);
    W4BPtrs sp;
    sp.a[0] = vblk(scomp, srb); sp.a[1] = sp.a[0];
    sp.b[0] = ublk(scomp, 2 * ct); sp.b[1] = ublk(scomp, 2 * ct + 1);
    if (early) {
#pragma unroll
      for (int i = 0; i < SH; ++i) {
        w4b_load<1>(shr[i], sp, wave * SH + i);
        __builtin_amdgcn_sched_barrier(0);
      }
      asm volatile("" ::: "memory");   // (the compiler may not sink these requests to their first use behind the loop)
    }
  };
  const bool behind = (mode & 8) != 0;
  if (!behind) request_shared();
  // --- this wave's own component: the whole 64 x 64 tile over the whole K range.
  // mode bit 1 (NODE_TUNE_W4_SHAREV, four column tiles only): the four waves of a workgroup take the SAME component and
  // row tile and one column tile each -- they walk the same V blocks in lock-step, so three of their four requests for a
  // block are served by the CU's own L1 / merged in flight -- instead of four components of one tile (nothing shared
  // inside the CU).  The workgroup's place (tile % nCT) then names the component, the wave the column tile.
  {
    const bool sharev = (mode & 2) != 0 && nCT == 4;
    // mode bit 2 (NODE_TUNE_W4_SHAREV = 2; four column tiles, row tiles a multiple of two): a workgroup takes a 128 x 128 tile of
    // one component, wave (r, c) its 64 x 64 quarter: two waves walk each V block together, two each U block
    const bool share2 = (mode & 4) != 0 && nCT == 4 && (nRB & 3) == 0;
    const int comp = 4 * j + (share2 ? (tile & 3) : sharev ? ct : wave);
    const int oct = share2 ? 2 * ((tile >> 2) & 1) + (wave & 1) : sharev ? wave : ct;
    const int ort = share2 ? 2 * (tile >> 3) + (wave >> 1) : rt;
    W4BPtrs p;
    p.a[0] = vblk(comp, 2 * ort); p.a[1] = vblk(comp, 2 * ort + 1);
    p.b[0] = ublk(comp, 2 * oct); p.b[1] = ublk(comp, 2 * oct + 1);
    float16_t acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[r][c][q] = 0.f;
    w4b_run<W4B_DEPTH, 2, AB>(acc, p, 0, G2, st, [&]() { if (behind) request_shared(); });
    const size_t sstride = (size_t)(gm.C >> 5) * 36 * 128;   // floats per sample of M
    float* m0 = M + ((size_t)(ort * 16 + hi) * (gm.C >> 5) + 2 * oct) * (36 * 128) + (size_t)comp * 128 + l31;
    if (!(AB & 4) || acc[0][0][0] == 123.456f)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      float* o = m0 + (size_t)(2 * (q >> 2)) * sstride + (q & 3) * 32;
      st_wt(o, acc[0][0][q]);
      st_wt(o + 36 * 128, acc[0][1][q]);
      st_wt(o + 8 * sstride, acc[1][0][q]);
      st_wt(o + 8 * sstride + 36 * 128, acc[1][1][q]);
    }
    w4_stamp(st, 4);
  }
  // --- half a tile of a shared component: rows [32 half, 32 half + 32), K range [wave G2/4, (wave+1) G2/4) per wave
  if (!(AB & 1)) {
    const int scomp = 32 + (j >> 1), rb = 2 * rt + (j & 1);
    const int ng = G2 >> 2, g0 = wave * ng;
    W4BPtrs p;
    p.a[0] = vblk(scomp, rb); p.a[1] = p.a[0];
    p.b[0] = ublk(scomp, 2 * ct); p.b[1] = ublk(scomp, 2 * ct + 1);
    float16_t acc[2][2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[0][c][q] = 0.f;
    if (early) {
      W4Split cs[2];
#pragma unroll
      for (int i = 0; i < SH; ++i) {
        cs[0] = w4_split8(shr[i].a[0][0], shr[i].a[0][1]);
        w4b_mac<1>(acc, cs, shr[i]);
      }
    } else if (ng % 4 == 0) w4b_run<4, 1, AB>(acc, p, g0, ng);
    else if (ng % 2 == 0) w4b_run<2, 1, AB>(acc, p, g0, ng);
    else w4b_run<1, 1, AB>(acc, p, g0, ng);
    w4_stamp(st, 5);
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
      if ((AB & 4) && s.x != 123.456f) continue;
      st_wt(mrow, s.x);
      st_wt(mrow + 32, s.y);
      st_wt(mrow + 64, s.z);
      st_wt(mrow + 96, s.w);
    }
  }
#ifdef NODE_DIAG
  if (st != nullptr) {   // (diagnostics: when this wave's stores have drained)
    w4_stamp(st, 6);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    w4_stamp(st, 7);
  }
#endif
}

// ----------------------------------------------------------------------------
// k_w4_gemm128b: k_w4_gemm64b's products for LONG reductions (C >= 512: cfg 5's 16x16 states at 1024 filters), as a
// classic LDS-tiled GEMM.  k_w4_gemm64b gives every wave a component of its own, so the four waves of a workgroup share
// nothing and an XCD works on 4.5 components at once: at C = 1024 that is 47 MB of operands against a 4 MB L2, every
// 64-row tile streams all of the filter triples in from the Infinity Cache again (3.6 GB per launch, measured 472 us =
// 0.39 of the bf16 pipe).  Here a workgroup owns a 128 x 128 tile of ONE component, its waves 64 x 64 quarters; per
// K = 16 step each wave fetches one quarter of the tile's operands (2 + 3 KB instead of 4 + 6), splits its row block
// into bf16 triples ONCE for the workgroup, and the MFMA-ready 1 KB blocks go through a two-stage LDS ring (one barrier
// per step; two workgroups per CU cover each other's barriers).  An XCD walks through its components one at a time --
// 64 concurrent workgroups = every tile of a component at cfg 5 -- so what is live in its L2 is one K slice of V and U.
// Same V / Ub / M layouts.  Needs 4 N % 128 == 0 and C % 128 == 0.
// (The first version of this kernel, round 3, was measured at cfg 2 -- C = 256, 16 steps per tile -- and lost to
// k_w4_gemm64b there, 21.5 - 22.8 against 19.6 us: fill and drain dominate so short a loop.)
// ----------------------------------------------------------------------------
// A wave's share of one K = 16 step: its row block (two g blocks of V), its column block (three parts of Ub).  The five
// requests are inline asm with HAND-PLACED waits: left to the compiler, the wait state of the loop entry merged into the
// steady state made every other step wait for all but one of the ten requests in flight -- the step's own prefetch
// (s_waitcnt vmcnt(1) where vmcnt(5) is exact).  W4C_WAIT ties the wait to the registers, so no use can move above it, and
// the registers stay allocated to the request while it is in flight.
struct W4CLoad { w4_f32x4 a0, a1; w4_u32x4 b0, b1, b2; };
#define W4C_FETCH(L, PA, PB)                                                                        \
  {                                                                                                 \
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"((L).a0) : "v"(PA) : "memory");            \
    asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"((L).a1) : "v"(PA) : "memory"); \
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"((L).b0) : "v"(PB) : "memory");            \
    asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"((L).b1) : "v"(PB) : "memory"); \
    asm volatile("global_load_dwordx4 %0, %1, off offset:2048" : "=v"((L).b2) : "v"(PB) : "memory"); \
  }
#define W4C_WAIT(N, L) \
  asm volatile("s_waitcnt vmcnt(" #N ")" : "+v"((L).a0), "+v"((L).a1), "+v"((L).b0), "+v"((L).b1), "+v"((L).b2) : : "memory")

__global__ __launch_bounds__(256, 2) void k_w4_gemm128b(const float* __restrict__ V, const unsigned short* __restrict__ Ub,
                                                        float* __restrict__ M, const Ctrl* ctrl, W4Geom gm) {
  if (ctrl != nullptr && ctrl->done) return;   // a step enqueued past the end of the interval (Ctrl::done)
  extern __shared__ __attribute__((aligned(16))) w4_u32x4 tile_lds[];   // [2 stages][A 4 row blocks x 3 parts | B 4 column blocks x 3 parts][64 lanes]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int nCT = gm.C >> 7, nRT = gm.R >> 7, nT = nRT * nCT, G8 = gm.G8, G2 = G8 >> 1, CB = gm.C >> 5, nRB = gm.RB;
  // workgroup -> (component, tile): XCD j (= blockIdx % 8) takes components 4 j .. 4 j + 3 one after the other, then half of the
  // tiles of component 32 + j / 2
  const int j = blockIdx.x & 7, i = blockIdx.x >> 3;
  int comp, tile;
  if (i < 4 * nT) { comp = 4 * j + i / nT; tile = i % nT; }
  else { comp = 32 + (j >> 1); tile = (j & 1) * (nT >> 1) + (i - 4 * nT); }
  const int RT = tile / nCT, CT = tile - RT * nCT;
  const int a_off = (((l31 >> 2) * 8) + hi * 4 + (l31 & 3)) * 4;   // lane (row = 4 s + t, k-half hi) inside a V block
  // this lane's requests of step g2: V at pa + g2 * 2 KB (+ 1 KB: the second g block), Ub at pb + g2 * 3 KB (+ 1, 2 KB: the parts)
  const char* pa = reinterpret_cast<const char*>(V + (((size_t)comp * nRB + 4 * RT + wave) * G8) * 256 + a_off);
  const char* pb = reinterpret_cast<const char*>(reinterpret_cast<const w4_u32x4*>(Ub) + (((size_t)comp * CB + 4 * CT + wave) * G2) * 192 + lane);
  // LDS block (stage, kind 0 = A / 1 = B, block 0..3, part): 64 lanes x 16 B, every access lane * 16 B -- conflict-free
  auto blk = [&](int stage, int kind, int b, int part) { return tile_lds + ((((stage * 2 + kind) * 4 + b) * 3 + part) * 64 + lane); };
#define W4C_STASH(L, STAGE)                                                                                  \
  {                                                                                                          \
    const W4Split sp_ = w4_split8(make_float4((L).a0.x, (L).a0.y, (L).a0.z, (L).a0.w),                       \
                                  make_float4((L).a1.x, (L).a1.y, (L).a1.z, (L).a1.w));                      \
    *blk(STAGE, 0, wave, 0) = __builtin_bit_cast(w4_u32x4, sp_.h);                                           \
    *blk(STAGE, 0, wave, 1) = __builtin_bit_cast(w4_u32x4, sp_.m);                                           \
    *blk(STAGE, 0, wave, 2) = __builtin_bit_cast(w4_u32x4, sp_.l);                                           \
    *blk(STAGE, 1, wave, 0) = (L).b0;                                                                        \
    *blk(STAGE, 1, wave, 1) = (L).b1;                                                                        \
    *blk(STAGE, 1, wave, 2) = (L).b2;                                                                        \
  }
  const int wr = wave >> 1, wc = wave & 1;
  float16_t acc[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[r][c][q] = 0.f;

  // Two register sets, never copied: at the top of an even step k, ldx holds step k + 1 and ldy step k + 2 (five requests
  // each, ldx's the older) -- two steps of cover.  (Reads past the reduction's end land in the buffers' slack.)
  W4CLoad ldx, ldy;
  W4C_FETCH(ldx, pa, pb)
  W4C_WAIT(0, ldx);
  W4C_STASH(ldx, 0)
  W4C_FETCH(ldx, pa + 2048, pb + 3072)
  W4C_FETCH(ldy, pa + 4096, pb + 6144)
  pa += 3 * 2048; pb += 3 * 3072;          // -> step 3
  __syncthreads();
#define W4C_STEP(ST, LD)                                                                                          \
  {                                                                                                               \
    w4_u32x4 fa[2][3], fb[2][3];                                                                                  \
    _Pragma("unroll") for (int r = 0; r < 2; ++r) _Pragma("unroll") for (int q = 0; q < 3; ++q) {                 \
      fa[r][q] = *blk(ST, 0, 2 * wr + r, q);                                                                      \
      fb[r][q] = *blk(ST, 1, 2 * wc + r, q);                                                                      \
    }                                                                                                             \
    w4c_mac(acc, fa, fb);                                                                                         \
    W4C_WAIT(5, LD); /* the older five of the ten in flight */                                                    \
    W4C_STASH(LD, (ST) ^ 1) /* the next step -> the other stage (everybody left it at the last barrier) */        \
    W4C_FETCH(LD, pa, pb)                                                                                         \
    pa += 2048; pb += 3072;                                                                                       \
    __syncthreads();                                                                                              \
  }
  for (int k = 0; k < G2; k += 2) {   // (G2 = C / 16 is even: C % 128 == 0)
    W4C_STEP(0, ldx)
    W4C_STEP(1, ldy)
  }
  W4C_WAIT(0, ldx);                   // nothing may still be landing in registers the epilogue reuses
  W4C_WAIT(0, ldy);
#undef W4C_STEP
#undef W4C_STASH
  // M is [n][C/32][36][4 t][32 c] (wino4.h): this wave's 64 x 64 quarter = 64-row tile 2 RT + wr, 64-column tile 2 CT + wc
  const int rt = 2 * RT + wr, ct = 2 * CT + wc;
  const size_t sstride = (size_t)(gm.C >> 5) * 36 * 128;   // floats per sample of M
  float* m0 = M + ((size_t)(rt * 16 + hi) * (gm.C >> 5) + 2 * ct) * (36 * 128) + (size_t)comp * 128 + l31;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    float* o = m0 + (size_t)(2 * (q >> 2)) * sstride + (q & 3) * 32;
    st_wt(o, acc[0][0][q]);
    st_wt(o + 36 * 128, acc[0][1][q]);
    st_wt(o + 8 * sstride, acc[1][0][q]);
    st_wt(o + 8 * sstride + 36 * 128, acc[1][1][q]);
  }
}

void launch_w4_gemm_bf16_64(const float* V, const unsigned short* Ub, float* M, const Ctrl* ctrl, const W4Geom& gm, int mode,
                            unsigned long long* stamps, hipStream_t s) {
  hipLaunchKernelGGL(k_w4_gemm64b<0>, dim3((gm.N / 16) * (gm.C >> 6) * 8), dim3(256), 4 * 2048 * sizeof(float), s, V, Ub, M, ctrl, gm, mode, stamps);
}
void launch_w4_gemm_bf16_128(const float* V, const unsigned short* Ub, float* M, const Ctrl* ctrl, const W4Geom& gm, hipStream_t s) {
  static bool attr[MAX_DEVICES] = {};
  const int nT = (gm.N / 32) * (gm.C >> 7);
  allow_full_lds(reinterpret_cast<const void*>(k_w4_gemm128b), attr);
  hipLaunchKernelGGL(k_w4_gemm128b, dim3(8 * (4 * nT + nT / 2)), dim3(256), 2 * 24 * 64 * 16, s, V, Ub, M, ctrl, gm);
}

}  // namespace node
