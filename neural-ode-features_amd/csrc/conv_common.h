// What the fp32 3x3 convolution kernels (kernels_conv_{direct,wino1d,wino2d,small}.hip) share: the MFMA accumulator type, the LDS
// strides of the operand images and of the epilogue tile, the DPP wave sum, the in-kernel stamps of the NODE_STAMPS build, and the
// GroupNorm epilogue that follows every one of the throughput kernels.  conv_select.hip chooses among the kernels.
#pragma once
#include "node_internal.h"

namespace node {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int AST2 = 36;          // floats per halo slot of the A image
constexpr int BST2 = 36;          // floats per output column of the B tile
constexpr int BBUF2 = BN * BST2;  // one B piece in LDS
constexpr int CT2 = BN + 1;       // epilogue tile stride
// the two Winograd kernels: 16-channel K chunks
constexpr int KCW = 16;            // channels per K chunk
constexpr int ASTW = 20;           // floats per (slot, component) row of the A image: 16 channels + 16-B pad

// 64-lane sum on the DPP cross-lane path (8 VALU ops) instead of six LDS-crossbar shuffles:
// quad swaps, row mirrors, then the two row broadcasts; the total lands in lane 63.
__device__ inline float wave_sum_p(float v) {
#define DPP_ADD(CTRL, RM)                                                                              \
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, RM, 0xf, true))
  DPP_ADD(0xB1, 0xf);   // quad_perm [1,0,3,2]
  DPP_ADD(0x4E, 0xf);   // quad_perm [2,3,0,1]
  DPP_ADD(0x141, 0xf);  // row_half_mirror
  DPP_ADD(0x140, 0xf);  // row_mirror: every lane of a 16-lane row holds the row sum
  DPP_ADD(0x142, 0xa);  // row_bcast15 into rows 1 and 3
  DPP_ADD(0x143, 0xc);  // row_bcast31 into rows 2 and 3
#undef DPP_ADD
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ inline int slot_of_p(int p, int W, int Wp) {
  const int h = p / W;
  return (h + 1) * Wp + (p - h * W) + 1;
}

#ifdef NODE_STAMPS
#define PSTAMP(buf, slot, INS)                                                                   \
  do {                                                                                           \
    if ((buf) != nullptr && (threadIdx.x & 63) == 0) {                                           \
      unsigned long long _t;                                                                     \
      __builtin_amdgcn_sched_barrier(0);                                                         \
      asm volatile(INS " %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");                       \
      __builtin_amdgcn_sched_barrier(0);                                                         \
      (buf)[((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 16 + (slot)] = _t; \
    }                                                                                            \
  } while (0)
#define ABL(bit) (a.ablate & (bit))   /* timing-only ablations: 1 no B stream, 2 no barrier, 4 no operand reads, 8 no A stream */
#else
#define PSTAMP(buf, slot, INS) do { } while (0)
#define ABL(bit) 0
#endif

// ----------------------------------------------------------------------------
// Shared epilogue tail.  On entry the pre-normalisation tile Ct[BM][CT2] (conv output + bias + t*tmap,
// or the raw data gradient) is complete in LDS and the workgroup is synchronised.  Forward: GroupNorm
// statistics with a lane<->pixel mapping (conflict-free, no integer division in any loop, DPP wave
// reductions), normalise (+ReLU), 16-B stores of the activation and of xhat / rstd for the backward.
// Backward: ReLU mask, (dgamma, dbeta) tile partials, GroupNorm backward, 16-B stores.
// ----------------------------------------------------------------------------
template <int THREADS, int BM>
__device__ inline void conv_epilogue_tail(const ConvArgs& a, const Dims& d, float* smem, int n0, int c0, int nsamp,
                                          int ncols, int mtile) {
  constexpr int NWAVES = THREADS / 64;
  constexpr int RL = THREADS / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool fwd = a.mode != CM_BWD_RELU_GN;
  float* Ct = smem;                   // [BM][CT2]
  float* Xt = smem + BM * CT2;        // [BM][CT2]   (bwd only)
  float* st0 = smem + 2 * BM * CT2;   // [S*BN] mean / m1
  float* st1 = st0 + d.S * BN;        // [S*BN] rstd / m2
  float* cred = st1 + d.S * BN;       // [RL][64][2]
  const int GT = ncols / d.cpg;  // whole groups in this tile
  const int npairs = nsamp * GT;
  const float inv_m = 1.0f / (float)(d.HW * d.cpg);
  // thread <-> (column quad, row lane) mapping of the store passes
  const int colq = (tid & 15) * 4, rr = tid >> 4;
  const bool vec_ok = ((c0 & 3) == 0) && ((ncols & 3) == 0);
  int glq[4];
  bool okq[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    okq[i] = (colq + i) < ncols;
    glq[i] = okq[i] ? (colq + i) / d.cpg : 0;
  }

  if (fwd) {
    for (int pair = wave; pair < npairs; pair += NWAVES) {
      const int s = pair / GT, gl = pair - s * GT;
      const float* base = Ct + (s * d.HW) * CT2 + gl * d.cpg;
      float sum = 0.f;
      for (int p = lane; p < d.HW; p += 64) {
#pragma unroll 8
        for (int cc = 0; cc < d.cpg; ++cc) sum += base[p * CT2 + cc];
      }
      const float mean = wave_sum_p(sum) * inv_m;
      float s2 = 0.f;
      for (int p = lane; p < d.HW; p += 64) {
#pragma unroll 8
        for (int cc = 0; cc < d.cpg; ++cc) {
          const float dv = base[p * CT2 + cc] - mean;
          s2 += dv * dv;
        }
      }
      const float var = wave_sum_p(s2) * inv_m;
      const float rstd = 1.0f / sqrtf(var + d.eps);
      if (lane == 0) {
        st0[pair] = mean;
        st1[pair] = rstd;
        if (a.rstd_out) a.rstd_out[(size_t)(n0 + s) * d.G + c0 / d.cpg + gl] = rstd;
      }
    }
    __syncthreads();
    PSTAMP(a.stamps, 7, "s_memtime");
    float gm[4], bt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      gm[i] = okq[i] ? a.gamma[c0 + colq + i] : 0.f;
      bt[i] = okq[i] ? a.beta[c0 + colq + i] : 0.f;
    }
    const bool relu = a.mode == CM_FWD_GN_RELU;
    for (int s = 0; s < nsamp; ++s) {
      float mean[4], rstd[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { mean[i] = st0[s * GT + glq[i]]; rstd[i] = st1[s * GT + glq[i]]; }
      for (int p = rr; p < d.HW; p += RL) {
        const float* src = Ct + (s * d.HW + p) * CT2 + colq;
        float xh[4], o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          xh[i] = (src[i] - mean[i]) * rstd[i];
          float v = xh[i] * gm[i] + bt[i];
          if (relu) v = fmaxf(v, 0.f);
          o[i] = a.osign * v;
        }
        const size_t off = ((size_t)(n0 + s) * d.HW + p) * d.C + c0 + colq;
        if (vec_ok) {
          if (okq[0]) {
            *reinterpret_cast<float4*>(a.out + off) = make_float4(o[0], o[1], o[2], o[3]);
            if (a.xhat_out) *reinterpret_cast<float4*>(a.xhat_out + off) = make_float4(xh[0], xh[1], xh[2], xh[3]);
          }
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (okq[i]) {
              a.out[off + i] = o[i];
              if (a.xhat_out) a.xhat_out[off + i] = xh[i];
            }
        }
      }
    }
  } else {
    // ReLU mask, dxhat = du * gamma, column partials of (dgamma, dbeta)
    float gm[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) gm[i] = okq[i] ? a.gamma[c0 + colq + i] : 0.f;
    float dg[4] = {0.f, 0.f, 0.f, 0.f}, db[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < nsamp; ++s) {
      for (int p = rr; p < d.HW; p += RL) {
        const int row = s * d.HW + p;
        const size_t off = ((size_t)(n0 + s) * d.HW + p) * d.C + c0 + colq;
        float x[4], ac[4];
        if (vec_ok) {
          float4 xv = make_float4(0.f, 0.f, 0.f, 0.f), av = xv;
          if (okq[0]) {
            xv = *reinterpret_cast<const float4*>(a.xhat + off);
            av = *reinterpret_cast<const float4*>(a.act + off);
          }
          x[0] = xv.x; x[1] = xv.y; x[2] = xv.z; x[3] = xv.w;
          ac[0] = av.x; ac[1] = av.y; ac[2] = av.z; ac[3] = av.w;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            x[i] = okq[i] ? a.xhat[off + i] : 0.f;
            ac[i] = okq[i] ? a.act[off + i] : 0.f;
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float du = (okq[i] && ac[i] > 0.f) ? Ct[row * CT2 + colq + i] : 0.f;
          dg[i] += du * x[i];
          db[i] += du;
          Ct[row * CT2 + colq + i] = du * gm[i];
          Xt[row * CT2 + colq + i] = x[i];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      cred[(rr * 64 + colq + i) * 2] = dg[i];
      cred[(rr * 64 + colq + i) * 2 + 1] = db[i];
    }
    __syncthreads();
    if (tid < 128) {
      const int col = tid & 63, which = tid >> 6;
      if (col < ncols) {
        float v = 0.f;
#pragma unroll 8
        for (int r = 0; r < RL; ++r) v += cred[(r * 64 + col) * 2 + which];
        a.gpart[((size_t)mtile * 2 + which) * d.C + c0 + col] = v;
      }
    }
    for (int pair = wave; pair < npairs; pair += NWAVES) {
      const int s = pair / GT, gl = pair - s * GT;
      const int base = (s * d.HW) * CT2 + gl * d.cpg;
      float s1 = 0.f, s2 = 0.f;
      for (int p = lane; p < d.HW; p += 64) {
#pragma unroll 8
        for (int cc = 0; cc < d.cpg; ++cc) {
          const float dxh = Ct[base + p * CT2 + cc];
          s1 += dxh;
          s2 += dxh * Xt[base + p * CT2 + cc];
        }
      }
      s1 = wave_sum_p(s1) * inv_m;
      s2 = wave_sum_p(s2) * inv_m;
      if (lane == 0) { st0[pair] = s1; st1[pair] = s2; }
    }
    __syncthreads();
    for (int s = 0; s < nsamp; ++s) {
      float m1[4], m2[4], rs[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        m1[i] = st0[s * GT + glq[i]];
        m2[i] = st1[s * GT + glq[i]];
        rs[i] = okq[i] ? a.rstd[(size_t)(n0 + s) * d.G + c0 / d.cpg + glq[i]] : 0.f;
      }
      for (int p = rr; p < d.HW; p += RL) {
        const int row = s * d.HW + p;
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          o[i] = a.osign * (rs[i] * (Ct[row * CT2 + colq + i] - m1[i] - Xt[row * CT2 + colq + i] * m2[i]));
        const size_t off = ((size_t)(n0 + s) * d.HW + p) * d.C + c0 + colq;
        if (vec_ok) {
          if (okq[0]) *reinterpret_cast<float4*>(a.out + off) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (okq[i]) a.out[off + i] = o[i];
        }
        if (a.spart) {   // keep the finished tile for the column sums below (same thread read these four entries)
#pragma unroll
          for (int i = 0; i < 4; ++i) Ct[row * CT2 + colq + i] = okq[i] ? o[i] : 0.f;
        }
      }
    }
    if (a.spart) {
      // masked column sums of the data gradient this tile just produced (it is the next layer's dz): saves a
      // k_colsum launch and its pass over the tensor.  Xt is free now: border flags, then the reduction scratch.
      __syncthreads();
      unsigned char* flg = reinterpret_cast<unsigned char*>(Xt);
      float* red9 = Xt + 64;   // HW <= BM <= 256 bytes of flags
      for (int p = tid; p < d.HW; p += THREADS) {
        const int h = p / d.W, x = p - h * d.W;
        flg[p] = (unsigned char)((h == 0 ? 1 : 0) | (h == d.H - 1 ? 2 : 0) | (x == 0 ? 4 : 0) | (x == d.W - 1 ? 8 : 0));
      }
      __syncthreads();
      for (int s = 0; s < nsamp; ++s)
        masked_colsum_tile(Ct + (s * d.HW) * CT2, CT2, d.HW, flg, ncols, max(1, min(min(THREADS / ncols, 8), (BM * CT2 - 64) / (9 * ncols))), tid, red9,
                           a.spart + (size_t)(n0 + s) * 9 * d.C + c0, d.C);
    }
  }
}

}  // namespace node
