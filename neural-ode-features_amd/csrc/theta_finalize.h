// ============================================================================
// theta-segment stage derivative: reduce the split-K / per-tile partials written
// by the wgrad GEMM and the GroupNorm-backward epilogues into one vector in the
// internal theta layout, times osign (= tsign, the reverse-time negation).
// The body of k_theta_finalize (kernels_theta_finalize.hip) as a device function, so that the same workgroups can
// also ride in front of another kernel's grid (k_w4s_pass_rider, kernels_w4s.hip).
// ============================================================================
#pragma once
#include "pointwise_common.h"
#include "wino4.h"

namespace node {

// ONE launch (a kernel on this box costs >= 5 us however little it does, and this used to be three):
//   bulk of the vector (the last 2 x wb workgroups): the two conv-weight blocks, out[r] = osign * sum_sp wpart[sp][r], as
//     float4 with four slabs in flight per thread (the split-K slabs are 16 x 2.36 MB at C = 256: HBM-bound);
//   the small pieces (the first 5 x nsm workgroups; 26 C values): GroupNorm affine gradients (jobs 0..2), time-channel taps
//     and conv biases (jobs 3, 4) -- column sums of short matrices ([rows][2C] per-tile GroupNorm partials,
//     [N][9C] per-sample masked dz sums); one 64-column chunk, 64 columns x 4 row groups, per workgroup;
//   vjp_t = sum_layers sum_{tap,co} W[co][0][tap] * S[tap][co]  (d conv / d t = time-channel border map): each
//     conv-job workgroup leaves the dot product of its 64 columns in a.sred's tail, the last one to arrive
//     (agent-scope fences around a device counter) adds them in a fixed order -- deterministic.
//
// BT = threads of the calling workgroup, 256 or 128; `bx_all` of `nblk`: the workgroup's place in the grid of launch_theta_finalize
// (theta_finalize_blocks).  A 128-thread workgroup does the work of the 256-thread one it stands for with every sum in the same
// order: a thread walks the elements of the bulk that two threads walked (the bulk is per element), and carries the row-group sums
// of the two row groups rg and rg + 2 as separate accumulators, which meet in `red` exactly where four row groups' did.
// The caller has tested ctrl->done.
// (a run-time index into an array of the kernel's arguments makes the compiler keep a copy of it in scratch memory: selects instead)
template <typename T>
__device__ __forceinline__ T tf_sel2(const T (&x)[2], int i) { return i ? x[1] : x[0]; }
template <typename T>
__device__ __forceinline__ T tf_sel3(const T (&x)[3], int i) { return i == 0 ? x[0] : i == 1 ? x[1] : x[2]; }

template <int BT>
__device__ __forceinline__ void theta_finalize_body(const ThetaFinalizeArgs& a, const Dims& d, const int bx_all, const int nblk) {
  static_assert(BT == 256 || BT == 128, "a row group is one wave: four of them in one or two per thread");
  __shared__ float red[256];
  __shared__ int s_last;
  const int tid = threadIdx.x;
  const ThetaLayout L = theta_layout(d.C);
  const int C = d.C;
  // linear grid: [5 jobs x nsm column chunks of the small pieces][2 layers x wb blocks of the bulk sums] -- the small
  // jobs first, so that their arrival chain overlaps the bulk; no workgroup is launched just to exit
  const int nsm = (9 * C + 63) / 64;
  const int wb = (nblk - 5 * nsm) / 2;
  if (bx_all >= 5 * nsm) {
    const int layer = (bx_all - 5 * nsm) / wb, bx = (bx_all - 5 * nsm) - layer * wb;
    const size_t CC = (size_t)C * C;
    const size_t n4 = 9 * CC / 4;   // C % 4 == 0
    const float4* wp = reinterpret_cast<const float4*>(tf_sel2(a.wpart, layer));
    float4* out = reinterpret_cast<float4*>(a.theta_out + tf_sel2(L.wc, layer));   // 16-B aligned: every block size is a multiple of C
    const size_t stride = (size_t)wb * 256;
    if (a.dU != nullptr) {   // F(4x4,3x3)-domain gradients, every element written once by k_w4_wgrad: dW = G^T dU G
      // (measured, round 6: one (ci, co) pair per thread instead of four -- 2 x 256 instead of 2 x 64 workgroups with work -- 15.8 against
      //  13.0 us: the launch is one round of 36 loads per thread either way, and 4-byte loads are four times the requests)
      const size_t cc4 = CC / 4;
      const float4* du = reinterpret_cast<const float4*>(a.dU + (size_t)layer * W4_COMPS * CC);
      for (int h = 0; h < 256; h += BT)
      for (size_t i = (size_t)bx * 256 + h + tid; i < cc4; i += stride) {
        // (a uniform component base plus one 32-bit byte offset per thread -- C C 4 bytes < 4 GB: otherwise every one of the 45 vectors
        //  keeps a 64-bit address in vector registers of its own)
        const unsigned off = (unsigned)i * 16u;
        float4 tq[6][3];   // t[xi][kw] = sum_nu dU[xi][nu] G[nu][kw]
#pragma unroll
        for (int xi = 0; xi < 6; ++xi) {
          float4 u[6];
#pragma unroll
          for (int nu = 0; nu < 6; ++nu) u[nu] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(du + (size_t)(xi * 6 + nu) * cc4) + off);
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int nu = 0; nu < 6; ++nu) {
              const float gq = (float)W4_G[nu][kw];
              if (gq != 0.f) { s.x += gq * u[nu].x; s.y += gq * u[nu].y; s.z += gq * u[nu].z; s.w += gq * u[nu].w; }
            }
            tq[xi][kw] = s;
          }
        }
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int xi = 0; xi < 6; ++xi) {
              const float gq = (float)W4_G[xi][kh];
              if (gq != 0.f) { s.x += gq * tq[xi][kw].x; s.y += gq * tq[xi][kw].y; s.z += gq * tq[xi][kw].z; s.w += gq * tq[xi][kw].w; }
            }
            *reinterpret_cast<float4*>(reinterpret_cast<char*>(out + (size_t)(kh * 3 + kw) * cc4) + off) = make_float4(a.osign * s.x, a.osign * s.y, a.osign * s.z, a.osign * s.w);
          }
      }
      return;
    }
    for (int h = 0; h < 256; h += BT)
    for (size_t i = (size_t)bx * 256 + h + tid; i < n4; i += stride) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      int sp = 0;
      for (; sp + 4 <= d.nsplit; sp += 4) {
        const float4 v0 = wp[(size_t)sp * n4 + i], v1 = wp[(size_t)(sp + 1) * n4 + i];
        const float4 v2 = wp[(size_t)(sp + 2) * n4 + i], v3 = wp[(size_t)(sp + 3) * n4 + i];
        acc.x += (v0.x + v1.x) + (v2.x + v3.x); acc.y += (v0.y + v1.y) + (v2.y + v3.y);
        acc.z += (v0.z + v1.z) + (v2.z + v3.z); acc.w += (v0.w + v1.w) + (v2.w + v3.w);
      }
      for (; sp < d.nsplit; ++sp) {
        const float4 v = wp[(size_t)sp * n4 + i];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
      out[i] = make_float4(a.osign * acc.x, a.osign * acc.y, a.osign * acc.z, a.osign * acc.w);
    }
    return;
  }
  const int job = bx_all / nsm, bxs = bx_all - job * nsm;
  const bool gn = job < 3;
  const int layer = gn ? job : job - 3;
  const int ncol = gn ? 2 * C : 9 * C;
  if (bxs * 64 >= ncol) return;
  const int rows = gn ? tf_sel3(a.gpart_rows, layer) : (a.spart_rows > 0 ? a.spart_rows : d.N);
  const float* src = gn ? tf_sel3(a.gpart, layer) : tf_sel2(a.spart, layer);
  const int cl = tid & 63, rg = tid >> 6;
  const int col = bxs * 64 + cl;
  float vr[256 / BT];     // the sums of row groups rg (and, 128 threads, rg + 2)
#pragma unroll
  for (int g = 0; g < 256 / BT; ++g) {
    float v = 0.f;
    if (col < ncol) {
      int r = rg + g * (BT / 64);
      for (; r + 12 < rows; r += 16) {
        const float v0 = src[(size_t)r * ncol + col], v1 = src[(size_t)(r + 4) * ncol + col];
        const float v2 = src[(size_t)(r + 8) * ncol + col], v3 = src[(size_t)(r + 12) * ncol + col];
        v += (v0 + v1) + (v2 + v3);
      }
      for (; r < rows; r += 4) v += src[(size_t)r * ncol + col];
    }
    vr[g] = v;
  }
#pragma unroll
  for (int g = 0; g < 256 / BT; ++g) red[g * BT + tid] = vr[g];
  __syncthreads();
  if (rg != 0) return;          // the first wave finishes the job
  const bool on = col < ncol;
  const float v = (red[cl] + red[64 + cl]) + (red[128 + cl] + red[192 + cl]);
  if (gn) {   // columns [0, C) = dgamma, [C, 2C) = dbeta
    if (on) {
      const int which = col >= C ? 1 : 0;
      a.theta_out[(which ? tf_sel3(L.b, layer) : tf_sel3(L.g, layer)) + (col - which * C)] = a.osign * v;
    }
    return;
  }
  // column = tap * C + co
  if (on) {
    a.theta_out[tf_sel2(L.wt, layer) + col] = a.osign * (v * eval_time(a.et));  // time-channel taps: t * masked sums
    if (col >= 4 * C && col < 5 * C) a.theta_out[tf_sel2(L.cb, layer) + (col - 4 * C)] = a.osign * v;  // conv bias = centre tap
  }
  const int nb = (9 * C + 63) / 64;                    // conv-job workgroups per layer
  float* dotpart = a.sred + (size_t)2 * 9 * C;         // [2][nb] partial dot products, then the arrival counter
  unsigned* counter = reinterpret_cast<unsigned*>(dotpart + 2 * nb);
  const float part = wave_sum(on ? v * tf_sel2(a.wtime, layer)[col] : 0.f);   // wtime: [tap][co], gathered once per solve (k_wtime)
  // Hand-off without fences: an agent-scope release here would write back this XCD's whole L2, which is full of
  // the wgrad slabs' dirty lines (measured: +12 us on the launch).  The partial is an agent-scope (write-through)
  // store, acknowledged (vmcnt(0)) before the agent-scope count; the last arriver reads with agent-scope loads.
  // This leans on gfx950's memory system (agent-scope stores write through the XCD's L2; s_waitcnt vmcnt(0) waits
  // for the write acknowledgement), not on the HIP memory model -- so it is tied to the architecture at compile
  // time, and tests/test_gpu_parity.py::test_vjp_t_is_deterministic_over_repeated_launches watches it.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "k_theta_finalize's fence-free hand-off is only valid on gfx950: use release/acquire on the counter elsewhere"
#endif
  if (cl == 0) {
    __hip_atomic_store(dotpart + layer * nb + bxs, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(2 * nb - 1);
  }
  __builtin_amdgcn_wave_barrier();
  if (!s_last) return;                                  // (one wave: LDS write above is visible after the wave barrier)
  float tot = 0.f;
  for (int i = cl; i < 2 * nb; i += 64) tot += __hip_atomic_load(dotpart + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  tot = wave_sum(tot);
  if (cl == 0) {
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch (stream order)
    if (a.write_scalar) a.ctrl->ts_k[a.kidx] = a.osign * tot;
    if (a.vjp_t_out) *a.vjp_t_out = a.osign * tot;
  }
}

// the grid of the finalize: [5 jobs x nsmall column chunks][2 layers x wblocks of the bulk], whatever the workgroup's size
inline unsigned theta_finalize_blocks(const Dims& d, const ThetaFinalizeArgs& a) {
  size_t wblocks = (9 * (size_t)d.C * d.C / 4 + 255) / 256;
  if (a.dU != nullptr) wblocks = ((size_t)d.C * d.C / 4 + 255) / 256;      // F(4x4,3x3)-domain gradients: one float4 of (ci, co) pairs per thread
  if (wblocks > 1024) wblocks = 1024;
  const size_t nsmall = (9 * (size_t)d.C + 63) / 64;
  return (unsigned)(5 * nsmall + 2 * wblocks);
}

}  // namespace node
