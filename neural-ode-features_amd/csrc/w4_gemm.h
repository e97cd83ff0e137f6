// Winograd F(4x4,3x3) pipeline, stage 2: what the translation units of the 36 component GEMMs share (internal to csrc/).
//   kernels_w4_pack.hip    the once-per-solve filter transform, the fp16-pair scales, the split checker
//   kernels_w4_f32.hip     fp32 MFMA:    k_w4_gemm, k_w4_gemm64, k_w4_gemm_small
//   kernels_w4_bf16.hip    bf16 triples: k_w4_gemm64b, k_w4_gemm128b
//   kernels_w4_f16.hip     fp16 pairs:   k_w4_gemm64h, k_w4_gemm128h, k_w4_gemm256h
//   kernels_w4_wgrad.hip   the weight gradients of all three families; k_w4_gemm64h_wgrad64h (weight gradient + one GEMM, one launch)
//   w4_select.hip          the NODE_TUNE_W4_* switches, which kernel runs for (N, C), launch_w4_gemm / launch_w4_gemm_f16
//   kernels_w4_diag.hip    measured-and-rejected variants: libnode_hip_diag.so only (build.py --diag)
// A kernel is launched from the file that defines it: every family exports plain host launchers (below) and w4_select.hip
// calls them.  gfx950 (MI355X / CDNA4) only.  See wino4.h for the data layouts.
#pragma once
#include "wino4.h"

namespace node {

typedef float float16_t __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void* w4_lds_ptr_t;

// Big once-written, once-read results (M, dU): stored WRITE-THROUGH (agent scope = sc1 on gfx950) so that they leave the
// XCD's L2 while the kernel still runs instead of as one write-back burst at its end (MI355X_MICROARCH.md, `boundary`:
// + B / 6 TB/s behind B dirty bytes).  NODE_WT_STORES=0 at build time: plain stores (A/B measurements).
#ifndef NODE_WT_STORES
#define NODE_WT_STORES 1
#endif
__device__ __forceinline__ void st_wt(float* p, float v) {
#if NODE_WT_STORES
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  *p = v;
#endif
}

typedef __bf16 w4_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 w4_bf16x2 __attribute__((ext_vector_type(2)));
typedef float w4_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned w4_u32x4 __attribute__((ext_vector_type(4)));
typedef float w4_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 w4_f16x8 __attribute__((ext_vector_type(8)));

// x = h + m + l EXACTLY: eight fp32 values as three bf16 parts each (every bf16 kernel, k_w4_split_check, k_w4_wgrad128b)
struct W4Split { w4_bf16x8 h, m, l; };
// (Measured and not kept, round 3: the remainders as v_dot2_f32_bf16(part, (-1, 0) | (0, -1), x) -- three instructions per pair
// and level instead of four.  No launch got faster (cfg 2 GEMM 23.2 vs 22.5 us by events, cfg 5 382 vs 383), and the compiler
// folded the (-1, 0) pair into an inline constant the instruction reads as (0, -1): wrong remainders for every even element,
// caught by tests/test_gpu_w4.py::test_w4_split_is_exact_on_the_device, which stays.)
// (the subtraction as ONE v_pk_add_f32 -- written as `x - convert(part)` the compiler emits two v_add_f32: 126 instead of 63
//  instructions per four K steps of k_w4_gemm64b, whose clock the chip holds down under load: fewer VALU instructions per MFMA is
//  what raises it, MI355X_MICROARCH.md 'DVFS give-back')
__device__ __forceinline__ w4_f32x2 w4_minus_part(const w4_f32x2& x, const w4_bf16x2& part) {
  return x + (-__builtin_convertvector(part, w4_f32x2));   // (a two-float fadd is a legal packed operation; the fsub is expanded)
}
__device__ __forceinline__ W4Split w4_split8(const float4& p, const float4& q) {
  const w4_f32x2 v[4] = {{p.x, p.y}, {p.z, p.w}, {q.x, q.y}, {q.z, q.w}};
  w4_u32x4 hh, mm, ll;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const w4_bf16x2 h = __builtin_convertvector(v[i], w4_bf16x2);
    const w4_f32x2 r = w4_minus_part(v[i], h);
    const w4_bf16x2 m = __builtin_convertvector(r, w4_bf16x2);
    const w4_f32x2 t = w4_minus_part(r, m);
    const w4_bf16x2 l = __builtin_convertvector(t, w4_bf16x2);
    hh[i] = __builtin_bit_cast(unsigned, h);
    mm[i] = __builtin_bit_cast(unsigned, m);
    ll[i] = __builtin_bit_cast(unsigned, l);
  }
  W4Split o;
  o.h = __builtin_bit_cast(w4_bf16x8, hh);
  o.m = __builtin_bit_cast(w4_bf16x8, mm);
  o.l = __builtin_bit_cast(w4_bf16x8, ll);
  return o;
}

// stamps (timing diagnostics, NODE_TUNE_W4_STAMPS): wall-clock ticks (100 MHz) of lane 0 -- [1] ring requested, [2] first step's operands
// arrived and multiplied, [3] loop done
#ifdef NODE_DIAG
__device__ __forceinline__ void w4_stamp(unsigned long long* st, int k) {
  if (st != nullptr && (threadIdx.x & 63) == 0) { st[k] = wall_clock64(); st[8 + k] = clock64(); }
}
#else
__device__ __forceinline__ void w4_stamp(unsigned long long*, int) {}   // (the product library stamps nothing)
#endif
struct W4Nothing { __device__ __forceinline__ void operator()() const {} };

// ----------------------------------------------------------------------------
// The register ring of the bf16-triple kernels that read their operands straight from L2 (k_w4_gemm64b; the variants of
// kernels_w4_diag.hip): fp32 row operand split in registers, filter operand as k_w4_pack's triples.
// ----------------------------------------------------------------------------
constexpr int W4B_DEPTH = 4;   // K = 16 steps (two g blocks each) in flight

struct W4BStage { float4 a[2][2]; w4_u32x4 b[2][3]; };   // [row block][g of the pair], [column block][part]
// (Measured and removed, round 4: the K steps of a wave's own component in a per-wave ROTATED order against L2-channel camping --
// every wave walks its streams with the same power-of-two strides.  18.2 -> 19.8 us per launch, cfg 2 24 870 -> 24 480 images/s: the
// waves that SHARE an operand block ask for it at the same time in the lock-step order and are served by one L2 fill; rotated,
// they are not.  And there is no camping to cure: pulling every block 1 - 11 KB out of the power-of-two spacing changes nothing
// (round-4 timing experiment, profiles/r04_w4_gemm_pad.txt).)
struct W4BPtrs { const float4* a[2]; const w4_u32x4* b[2]; };
template <int NRB>
__device__ __forceinline__ void w4b_load(W4BStage& s, const W4BPtrs& p, int g2) {
#pragma unroll
  for (int r = 0; r < NRB; ++r) {
    s.a[r][0] = p.a[r][(size_t)(2 * g2) * 64];
    s.a[r][1] = p.a[r][(size_t)(2 * g2 + 1) * 64];
  }
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int q = 0; q < 3; ++q) s.b[c][q] = p.b[c][(size_t)(g2 * 3 + q) * 64];
}
// the 6 * NRB * 2 MFMAs of one K = 16 step, the independent accumulators round-robin (no dependent back-to-back pair)
template <int NRB>
__device__ __forceinline__ void w4b_mac(float16_t (&acc)[2][2], const W4Split (&a)[2], const W4BStage& s) {
  w4_bf16x8 B[2][3];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int q = 0; q < 3; ++q) B[c][q] = __builtin_bit_cast(w4_bf16x8, s.b[c][q]);
#define W4B_P(AP, BQ)                                                                             \
  _Pragma("unroll") for (int r = 0; r < NRB; ++r) _Pragma("unroll") for (int c = 0; c < 2; ++c)   \
      acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[r].AP, B[c][BQ], acc[r][c], 0, 0, 0);
  W4B_P(l, 0) W4B_P(h, 2) W4B_P(m, 1) W4B_P(m, 0) W4B_P(h, 1) W4B_P(h, 0)   // smallest products first
#undef W4B_P
}
struct W4BCursor { const float4* a[2]; const w4_u32x4* b[2]; };
template <int NRB>
__device__ __forceinline__ void w4b_next(W4BStage& s, W4BCursor& cu) {   // the next K = 16 step of the streams
#pragma unroll
  for (int r = 0; r < NRB; ++r) {
    s.a[r][0] = cu.a[r][0];
    s.a[r][1] = cu.a[r][64];
    cu.a[r] += 128;
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
#pragma unroll
    for (int q = 0; q < 3; ++q) s.b[c][q] = cu.b[c][q * 64];
    cu.b[c] += 192;
  }
}
// acc += sum over K = 16 steps [g0, g0 + n) (n a multiple of D): a ring of D stages, each refilled right behind the
// MFMAs that consumed it; the refills of the last D steps read up to D steps past the range (buffer slack).  The exact
// bf16 split of the NEXT step's row operand (v_cvt_pk_bf16_f32 + subtracts: ~44 VALU instructions per row block) is
// interleaved with the CURRENT step's MFMAs -- one matrix instruction, then a few vector ones -- so that a wave that
// has its SIMD to itself keeps both pipes busy.
// after_fill: called once the ring's first D steps are requested (k_w4_gemm64b puts the shared component's requests there)
// (AB: the calling kernel's ablation parameter; only AB = 0 is instantiated)
template <int D, int NRB, int AB = 0, class F = W4Nothing>
__device__ __forceinline__ void w4b_run(float16_t (&acc)[2][2], const W4BPtrs& p, int g0, int n, unsigned long long* st = nullptr,
                                        F after_fill = F()) {
  W4BStage ring[D];
  // the operand streams as running pointers (one 64-bit add per stream and step; the loads of a step differ by immediates)
  W4BCursor cu;
#pragma unroll
  for (int r = 0; r < NRB; ++r) cu.a[r] = p.a[r] + (size_t)(2 * g0) * 64;
#pragma unroll
  for (int c = 0; c < 2; ++c) cu.b[c] = p.b[c] + (size_t)(3 * g0) * 64;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    w4b_next<NRB>(ring[i], cu);
    __builtin_amdgcn_sched_barrier(0);
  }
  after_fill();
  W4Split cur[2], nxt[2];
  w4_stamp(st, 1);
#pragma unroll
  for (int r = 0; r < NRB; ++r) cur[r] = w4_split8(ring[0].a[r][0], ring[0].a[r][1]);
  for (int g = g0; g < g0 + n; g += D) {
    if (g == g0 + D) w4_stamp(st, 2);
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const W4BStage& ns = ring[(i + 1) % D];          // the step after this one (refilled D - 1 steps ago)
#pragma unroll
      for (int r = 0; r < NRB; ++r) nxt[r] = w4_split8(ns.a[r][0], ns.a[r][1]);
      w4b_mac<NRB>(acc, cur, ring[i]);
#pragma unroll
      for (int k = 0; k < 12 * NRB; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // one MFMA ...
        __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);   // ... then up to four VALU instructions of the split
      }
      __builtin_amdgcn_sched_barrier(0);   // the refill stays behind the MFMAs that read the old contents
      w4b_next<NRB>(ring[i], cu);
#pragma unroll
      for (int r = 0; r < NRB; ++r) cur[r] = nxt[r];
    }
  }
  w4_stamp(st, 3);
}

// one K = 16 step of a 64 x 64 tile from MFMA-ready bf16 triples on both sides (k_w4_gemm128b, k_w4_wgrad128b: the LDS-tiled kernels)
__device__ __forceinline__ void w4c_mac(float16_t (&acc)[2][2], const w4_u32x4 (&a)[2][3], const w4_u32x4 (&b)[2][3]) {
  w4_bf16x8 A[2][3], B[2][3];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) { A[r][q] = __builtin_bit_cast(w4_bf16x8, a[r][q]); B[r][q] = __builtin_bit_cast(w4_bf16x8, b[r][q]); }
#define W4C_P(AP, BQ)                                                                           \
  _Pragma("unroll") for (int r = 0; r < 2; ++r) _Pragma("unroll") for (int c = 0; c < 2; ++c)   \
      acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[r][AP], B[c][BQ], acc[r][c], 0, 0, 0);
  W4C_P(2, 0) W4C_P(0, 2) W4C_P(1, 1) W4C_P(1, 0) W4C_P(0, 1) W4C_P(0, 0)   // parts 0 = h, 1 = m, 2 = l: smallest products first
#undef W4C_P
}

// ----------------------------------------------------------------------------
// The register ring of the fp16-pair kernels that read their operands straight from L2 (k_w4_gemm64h, the shared piece of
// k_w4_gemm128h, and the GEMM half of k_w4_gemm64h_wgrad64h in kernels_w4_wgrad.hip): both operands arrive as MFMA fragments.
// ----------------------------------------------------------------------------
struct W4HStage { w4_u32x4 a[2][2], b[2][2]; };    // [row block][part h, l], [column block][part]
struct W4HCursor { const w4_u32x4* a[2]; const w4_u32x4* b[2]; };
template <int NRB>
__device__ __forceinline__ void w4h_next(W4HStage& s, W4HCursor& cu) {   // the next K = 16 step of the streams (2 KB per stream and step)
#pragma unroll
  for (int r = 0; r < NRB; ++r) {
    s.a[r][0] = cu.a[r][0];
    s.a[r][1] = cu.a[r][64];
    cu.a[r] += 128;
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    s.b[c][0] = cu.b[c][0];
    s.b[c][1] = cu.b[c][64];
    cu.b[c] += 128;
  }
}
template <int NRB>
__device__ __forceinline__ void w4h_mac(float16_t (&acc)[2][2], const W4HStage& s) {
  w4_f16x8 A[2][2], B[2][2];
#pragma unroll
  for (int r = 0; r < NRB; ++r)
#pragma unroll
    for (int q = 0; q < 2; ++q) A[r][q] = __builtin_bit_cast(w4_f16x8, s.a[r][q]);
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int q = 0; q < 2; ++q) B[c][q] = __builtin_bit_cast(w4_f16x8, s.b[c][q]);
#define W4H_P(AP, BQ)                                                                             \
  _Pragma("unroll") for (int r = 0; r < NRB; ++r) _Pragma("unroll") for (int c = 0; c < 2; ++c)   \
      acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[r][AP], B[c][BQ], acc[r][c], 0, 0, 0);
  W4H_P(1, 0) W4H_P(0, 1) W4H_P(0, 0)   // smallest products first
#undef W4H_P
}
// acc += sum over K = 16 steps [g0, g0 + n) (n a multiple of D): a ring of D stages, each refilled right behind the MFMAs that
// consumed it (the refills of the last D steps read up to D steps past the range: buffer slack)
template <int D, int NRB, class F = W4Nothing>
__device__ __forceinline__ void w4h_run(float16_t (&acc)[2][2], const W4HCursor& start, int n, F after_fill = F(), unsigned long long* st = nullptr) {
  W4HStage ring[D];
  W4HCursor cu = start;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    w4h_next<NRB>(ring[i], cu);
    __builtin_amdgcn_sched_barrier(0);
  }
  after_fill();
  w4_stamp(st, 1);
  for (int g = 0; g < n; g += D) {
    if (g == D) w4_stamp(st, 2);
#pragma unroll
    for (int i = 0; i < D; ++i) {
      w4h_mac<NRB>(acc, ring[i]);
      __builtin_amdgcn_sched_barrier(0);   // the refill stays behind the MFMAs that read the old contents
      w4h_next<NRB>(ring[i], cu);
    }
  }
}

// ----------------------------------------------------------------------------
// The A/B switches that select the component-GEMM kernel (w4_select.hip). ONE reader for the packer (which filter forms a
// solve prepares) and the launchers (which kernel reads them): a process that changes a switch between solves (the tests do)
// can never pack for one kernel and launch another.  Under every setting the results stay correct: the switches choose which
// kernel family multiplies and how a component's tiles are dealt to waves (bit-identical).
//   NODE_TUNE_W4_GEMM64 = 0    k_w4_gemm (eight waves, 32 x 64 tiles) everywhere
//   NODE_TUNE_W4_BF16X3 = 0    the fp32 MFMA kernels instead of the bf16 triples
//   NODE_TUNE_W4_F16 = 0       never the fp16-pair operands (the bf16-triple kernels everywhere)
//   NODE_TUNE_W4_GEMM128 / _WGRAD128 = 0 never / 1 wherever it fits / unset (-1): long reductions (C >= 512)
//   NODE_TUNE_W4_H256 = 0 never / 1 where whole rounds of the chip are filled / 2 wherever the geometry has the tiles (tests)
//   NODE_TUNE_W4_SHAREV = 1 / 2  how k_w4_gemm64b / k_w4_gemm64h / k_w4_wgrad deal a component's tiles to the waves of a workgroup
//   NODE_TUNE_WGRAD_PAIRED = 0   an augmented evaluation's fp16-pair weight gradient and conv-1 data gradient as two launches;
//                            1   (default) as ONE launch (k_w4_gemm64h_wgrad64h) where w4_pair_fits, the weight gradient's workgroups
//                                first in the grid, 256 registers (two workgroups of either half per CU);
//                            3 / 5 / 7  measured variants: + 2 the GEMM's workgroups first, + 4 the GEMM's own register budget
// ----------------------------------------------------------------------------
struct W4Switches {
  int g64, b16, sharev, gemm128, wgrad128, f16, h256;
  int wgrad_paired;              // NODE_TUNE_WGRAD_PAIRED (below)
  // libnode_hip_diag.so only (0 / null in the product library):
  int early;                     // NODE_TUNE_W4_EARLY: k_w4_gemm64b's mode bit 3
  unsigned long long* stamps;    // NODE_TUNE_W4_STAMPS = device address of [grid * 4][16] u64 (tools/w4_stamps.py)
};
const W4Switches& w4_switches();   // as of the last w4_refresh_tuning() of this thread

// Which kernel runs for (N, C): pure functions of the switches and the geometry, each fit condition written once.
enum class W4Operands { Fp32, Pairs };   // what the caller holds: fp32 rows (launch_w4_gemm, launch_w4_wgrad) / fp16 pairs (launch_w4_*_f16)
enum class W4Gemm {
  None,          // pairs only: the geometry has no fp16-pair kernel
  Small,         // k_w4_gemm_small           (fp32 filters)
  F32Wide,       // k_w4_gemm                 (fp32 filters)
  F32_64,        // k_w4_gemm64               (fp32 filters)
  Bf16_64,       // k_w4_gemm64b              (filter triples)
  Bf16_128,      // k_w4_gemm128b             (filter triples)
  F16_64,        // k_w4_gemm64h
  F16_128,       // k_w4_gemm128h, every component
  F16_256Tail    // k_w4_gemm256h for components 0..31, k_w4_gemm128h(tail) for 32..35
};
enum class W4Wgrad { None, F32, Bf16_128, F16_64 };   // k_w4_wgrad / k_w4_wgrad128b / k_w4_wgrad64h
W4Gemm w4_select_gemm(const W4Switches& sw, int N, int C, W4Operands ops);
W4Wgrad w4_select_wgrad(const W4Switches& sw, int N, int C, bool two_layers, W4Operands ops);

// per-family launchers: geometry checked by the selector, grid and LDS size next to the kernel
void launch_w4_gemm_small(const float* V, const float* U, float* M, const Ctrl* ctrl, const W4Geom& gm, hipStream_t s);
void launch_w4_gemm_f32_wide(const float* V, const float* U, float* M, const Ctrl* ctrl, const W4Geom& gm, hipStream_t s);
void launch_w4_gemm_f32_64(const float* V, const float* U, float* M, const Ctrl* ctrl, const W4Geom& gm, hipStream_t s);
void launch_w4_gemm_bf16_64(const float* V, const unsigned short* Ub, float* M, const Ctrl* ctrl, const W4Geom& gm, int mode,
                            unsigned long long* stamps, hipStream_t s);
void launch_w4_gemm_bf16_128(const float* V, const unsigned short* Ub, float* M, const Ctrl* ctrl, const W4Geom& gm, hipStream_t s);
void launch_w4_gemm_f16_64(const unsigned* Vh, const unsigned* Uh, float* M, const Ctrl* ctrl, const W4Geom& gm, int mode, const int* v_exp,
                           const int* u_exp, unsigned long long* stamps, hipStream_t s);
// k_w4_gemm64h_wgrad64h (kernels_w4_wgrad.hip): launch_w4_gemm_f16_64 and launch_w4_wgrad_f16 (two layers) as one launch
void launch_w4_pair_f16_64(const unsigned* Vh, const unsigned* Uh, float* M, const W4Geom& gm, int mode, const int* gv_exp, const int* gu_exp,
                           const unsigned* V1, const unsigned* Z1, const unsigned* V2, const unsigned* Z2, float* dU, const Ctrl* ctrl,
                           const int* v1_exp, const int* v2_exp, const int* z_exp, int variant, hipStream_t s);
// tail: components 32..35 only (behind launch_w4_gemm_f16_256, which leaves them out)
void launch_w4_gemm_f16_128(const unsigned* Vh, const unsigned* Uh, float* M, const Ctrl* ctrl, const W4Geom& gm, const int* v_exp,
                            const int* u_exp, bool tail, hipStream_t s);
void launch_w4_gemm_f16_256(const unsigned* Vh, const unsigned* Uh, float* M, const Ctrl* ctrl, const W4Geom& gm, const int* v_exp,
                            const int* u_exp, hipStream_t s);

}  // namespace node
