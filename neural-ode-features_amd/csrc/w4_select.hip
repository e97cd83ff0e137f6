// Winograd F(4x4,3x3) pipeline, stage 2: the NODE_TUNE_W4_* switches, WHICH kernel multiplies the 36 components for a batch
// (N, C) -- one pure function per decision, asked by the packer (which filter forms a solve prepares) and by the launchers alike --
// and the public launchers of wino4.h.  The kernels live in kernels_w4_{f32,bf16,f16,wgrad}.hip (w4_gemm.h).
#include "w4_gemm.h"
#include <cstdio>
#include <cstdlib>

namespace node {

#ifdef NODE_DIAG
// The diagnostics library's ONE hook (kernels_w4_diag.hip): its own switches, and the measured-and-rejected variants that
// take a batch in k_w4_gemm64b's place.
void w4_diag_switches(W4Switches& sw);
bool launch_w4_gemm_variant(const W4Switches& sw, const float* V, const unsigned short* Ub, float* M, const Ctrl* ctrl, const W4Geom& gm,
                            hipStream_t s);
#else
static void w4_diag_switches(W4Switches&) {}
static bool launch_w4_gemm_variant(const W4Switches&, const float*, const unsigned short*, float*, const Ctrl*, const W4Geom&, hipStream_t) {
  return false;
}
#endif

static W4Switches w4_read_switches() {
  auto rd = env_int;
  W4Switches sw = {rd("NODE_TUNE_W4_GEMM64", 1), rd("NODE_TUNE_W4_BF16X3", 1), rd("NODE_TUNE_W4_SHAREV", 1), rd("NODE_TUNE_W4_GEMM128", -1),
                   rd("NODE_TUNE_W4_WGRAD128", -1), rd("NODE_TUNE_W4_F16", 1), rd("NODE_TUNE_W4_H256", 1), rd("NODE_TUNE_WGRAD_PAIRED", 1), 0, nullptr};
  w4_diag_switches(sw);
  return sw;
}
// The switches are read from the environment ONCE PER C-ABI CALL (w4_refresh_tuning at the top of every entry point that
// launches these kernels), not once per launch: a training step launches ~100 component GEMMs, and eleven getenv scans in
// front of each were a quarter of a millisecond of host time per step -- on the drop-in path, where the host is what
// bounds the step, that is throughput.  Tests that flip a switch between two calls still see it.
static thread_local W4Switches g_w4_sw;
static thread_local bool g_w4_sw_valid = false;
void w4_refresh_tuning() { g_w4_sw = w4_read_switches(); g_w4_sw_valid = true; }
const W4Switches& w4_switches() {
  if (!g_w4_sw_valid) w4_refresh_tuning();
  return g_w4_sw;
}

// ----------------------------------------------------------------------------
// The selector
// ----------------------------------------------------------------------------
// a switch of the LDS-tiled kernels: 0 never / 1 wherever the kernel fits / unset (-1): long reductions (C >= 512), where the
// kernels that give every wave a component of its own re-read their operands from the Infinity Cache
static bool w4_wants_tiled(int sw, int C) { return sw == 1 || (sw < 0 && C >= 512); }
// k_w4_gemm128b / k_w4_gemm128h: whole 128 x 128 tiles (rows = 4 N), an even number of them (components 32..35 go in half sets)
static bool w4_fits_tiles128(int N, int C) { return N % 32 == 0 && C % 128 == 0 && (((N / 32) * (C >> 7)) & 1) == 0; }
// k_w4_gemm256h: whole 256 x 256 tiles AND whole rounds of the chip (one workgroup per CU: 32 tiles-per-component workgroups, a
// multiple of 256 -- a quarter-full round is slower than k_w4_gemm128h's many small tiles); h256 = 2: wherever the tiles are whole
static bool w4_fits_tiles256(int N, int C, int h256) { return N % 64 == 0 && C % 256 == 0 && (h256 == 2 || ((N / 64) * (C >> 8)) % 8 == 0); }
static bool w4_reads_triples(W4Gemm k) { return k == W4Gemm::Bf16_64 || k == W4Gemm::Bf16_128; }

W4Gemm w4_select_gemm(const W4Switches& sw, int N, int C, W4Operands ops) {
  if (ops == W4Operands::Fp32) {
    if (N <= 16) return W4Gemm::Small;                                  // the bs = 1 census
    if (sw.g64 == 0 || N % 16 != 0) return W4Gemm::F32Wide;             // (k_w4_gemm64 and everything after it: 64-row tiles)
    if (sw.b16 == 0) return W4Gemm::F32_64;
    return w4_fits_tiles128(N, C) && w4_wants_tiled(sw.gemm128, C) ? W4Gemm::Bf16_128 : W4Gemm::Bf16_64;
  }
  // fp16 pairs: k_w4_gemm64h's 64 x 64 tiles at short reductions, the LDS-tiled kernels only at long ones (at cfg 5 k_w4_gemm64h
  // takes 371 us against k_w4_gemm128h's 262)
  if (N % 16 != 0 || C % 64 != 0) return W4Gemm::None;
  if (C < 512) return W4Gemm::F16_64;
  if (!w4_fits_tiles128(N, C)) return W4Gemm::None;
  return sw.h256 != 0 && w4_fits_tiles256(N, C, sw.h256) ? W4Gemm::F16_256Tail : W4Gemm::F16_128;
}

// k_w4_wgrad128b where the fp32 kernel is bound by the matrix pipe (long filters); the stem's one layer stays on k_w4_wgrad
W4Wgrad w4_select_wgrad(const W4Switches& sw, int N, int C, bool two_layers, W4Operands ops) {
  const bool tiles128 = N % 8 == 0 && C % 128 == 0;     // whole row blocks, whole 128 ci x 128 co tiles
  if (ops == W4Operands::Pairs) return tiles128 ? W4Wgrad::F16_64 : W4Wgrad::None;
  const bool even = (((C >> 7) * (C >> 7)) & 1) == 0;   // (k_w4_wgrad128b deals the tiles of components 32..35 in half sets)
  return two_layers && tiles128 && even && w4_wants_tiled(sw.wgrad128, C) ? W4Wgrad::Bf16_128 : W4Wgrad::F32;
}

// which filter form launch_w4_gemm will read for this batch
bool w4_uses_bf16(int N, int C) { return w4_reads_triples(w4_select_gemm(w4_switches(), N, C, W4Operands::Fp32)); }
// whether a solve prepares fp16 pairs for this batch (its first evaluations still run the triples: wino4.h)
bool w4_f16_fits(int N, int C) {
  return w4_switches().f16 != 0 && w4_uses_bf16(N, C) && w4_select_gemm(w4_switches(), N, C, W4Operands::Pairs) != W4Gemm::None;
}

// ----------------------------------------------------------------------------
// The launchers of wino4.h
// ----------------------------------------------------------------------------
// how a component's tiles are dealt to the waves of a workgroup (k_w4_gemm64b / k_w4_gemm64h mode bits 1, 2)
static int w4_sharev_mode(const W4Switches& sw) { return (sw.sharev == 1 ? 2 : 0) | (sw.sharev == 2 ? 4 : 0); }

void launch_w4_gemm(const float* V, const float* U, float* M, const Ctrl* ctrl, int N, int C, hipStream_t s, const unsigned short* Ub) {
  const W4Switches& sw = w4_switches();
  const W4Geom gm = w4_geom(N, C);
  W4Gemm k = w4_select_gemm(sw, N, C, W4Operands::Fp32);
  if (Ub == nullptr && w4_reads_triples(k)) k = W4Gemm::F32_64;     // (a caller that prepared the fp32 filters only)
  switch (k) {
    case W4Gemm::Small: launch_w4_gemm_small(V, U, M, ctrl, gm, s); return;
    case W4Gemm::F32Wide: launch_w4_gemm_f32_wide(V, U, M, ctrl, gm, s); return;
    case W4Gemm::F32_64: launch_w4_gemm_f32_64(V, U, M, ctrl, gm, s); return;
    case W4Gemm::Bf16_128: launch_w4_gemm_bf16_128(V, Ub, M, ctrl, gm, s); return;
    default: break;
  }
  if (launch_w4_gemm_variant(sw, V, Ub, M, ctrl, gm, s)) return;
  launch_w4_gemm_bf16_64(V, Ub, M, ctrl, gm, w4_sharev_mode(sw) | (sw.early ? 8 : 0), sw.stamps, s);
}

void launch_w4_gemm_f16(const unsigned* Vh, const unsigned* Uh, float* M, const Ctrl* ctrl, int N, int C, const int* v_exp, const int* u_exp,
                        hipStream_t s) {
  const W4Switches& sw = w4_switches();
  const W4Geom gm = w4_geom(N, C);
  switch (w4_select_gemm(sw, N, C, W4Operands::Pairs)) {
    case W4Gemm::F16_256Tail:
      launch_w4_gemm_f16_256(Vh, Uh, M, ctrl, gm, v_exp, u_exp, s);
      launch_w4_gemm_f16_128(Vh, Uh, M, ctrl, gm, v_exp, u_exp, true, s);
      return;
    case W4Gemm::F16_128: launch_w4_gemm_f16_128(Vh, Uh, M, ctrl, gm, v_exp, u_exp, false, s); return;
    case W4Gemm::F16_64: launch_w4_gemm_f16_64(Vh, Uh, M, ctrl, gm, w4_sharev_mode(sw), v_exp, u_exp, sw.stamps, s); return;
    default:      // w4_f16_fits said no: the caller prepared pairs for a batch that has no kernel for them
      fprintf(stderr, "launch_w4_gemm_f16: no fp16-pair kernel for N = %d, C = %d\n", N, C);
      abort();
  }
}

// The pair of an augmented evaluation -- weight gradient and conv-1 data gradient -- as one launch: where the GEMM is k_w4_gemm64h
// (C < 512) and the weight gradient k_w4_wgrad64h.  Every other batch keeps the two launches.
bool w4_pair_fits(int N, int C) {
  const W4Switches& sw = w4_switches();
  return (sw.wgrad_paired & 1) != 0 && sw.f16 != 0 && w4_select_gemm(sw, N, C, W4Operands::Pairs) == W4Gemm::F16_64 &&
         w4_select_wgrad(sw, N, C, true, W4Operands::Pairs) == W4Wgrad::F16_64;
}
void launch_w4_gemm_wgrad_f16(const unsigned* Vh, const unsigned* Uh, float* M, const int* gv_exp, const int* gu_exp, const unsigned* V1,
                              const unsigned* Z1, const unsigned* V2, const unsigned* Z2, float* dU, const Ctrl* ctrl, int N, int C,
                              const int* v1_exp, const int* v2_exp, const int* z_exp, hipStream_t s) {
  const W4Switches& sw = w4_switches();
  launch_w4_pair_f16_64(Vh, Uh, M, w4_geom(N, C), w4_sharev_mode(sw), gv_exp, gu_exp, V1, Z1, V2, Z2, dU, ctrl, v1_exp, v2_exp, z_exp,
                        sw.wgrad_paired, s);
}

}  // namespace node
