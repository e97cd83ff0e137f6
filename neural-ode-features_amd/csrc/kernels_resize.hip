// The transfer evaluations' test transform (the reference's evaluate.py:38-50: Resize, ToTensor, Normalize on a PIL image) as
// ONE launch per batch:
//
//   out_u8[b]     = Resize(data[index[b]])                    uint8 [B, C, OH, OW]   PIL's 8-bit bilinear resample, bit for bit
//   out_f32[b]    = Normalize(ToTensor(out_u8[b]))            fp32  [B, C, OH, OW]   k_augment's test-transform expressions
//   out_labels[b] = labels[index[b]]                          int64 [B]
//
// PIL resamples in two passes of 32-bit integer arithmetic: horizontally over every input row, rounding to bytes, then
// vertically on those bytes.  An output byte of either pass is clip(((1 << 21) + sum_k coeff[k] * pixel[xmin + k]) >> 22, 0,
// 255); the coefficients (a row sums to 2^22 up to its tap count, so the sum stays below 2^31) come from the host
// (resize_api.hip), one table per axis.  A pass whose size does not change has no table and copies.
//
// Shape: one workgroup per (image, channel) plane.  Pass 1 reads the plane from global memory -- a few KB that the
// workgroup alone touches: the taps of neighbouring outputs overlap in the cache, HBM sees each byte once -- and leaves
// the [H, OW] bytes between the passes in LDS.  Pass 2 reads columns of it and writes the outputs: consecutive lanes own
// consecutive groups of V output pixels of a row, so a wave stores contiguous runs.  V = 4 when OW is a multiple of 4 and the
// pointers are aligned to it (the reference's sizes): pass 1 writes and pass 2 reads LDS a dword at a time -- the lanes of one
// output row take consecutive dwords of one row of `mid` -- the uint8 output leaves as dwords and the fp32 output as float4,
// 1 KB per wave and store.  V = 1 is the same code on single pixels, for every other width.
// TAB: the two tables (a few KB at the reference's sizes) are copied into LDS first, one load per thread and one latency, and
// both passes read them there; a workgroup is short, and with the tables in global memory its time was two dependent global
// loads (position, then coefficient) in front of every output.  Tables that do not fit next to `mid` stay in global memory.
// An index outside [0, N) never reads the split: a black image (normalised like any other) and the label -1.
#include "node_internal.h"

namespace node {

namespace {

// PIL's clip8.  The bilinear filter has no negative weight, so acc >= 1 << 21 and the clip at 0 never acts: the shift is a
// logical one and the clip an unsigned minimum.  (Written as min(max(acc >> 22, 0), 255), hipcc of ROCm 7 packs two results
// with v_ashr_pk_u8_i32 and ORs the other bytes into a register whose upper half it takes to be zero; on gfx950 that half kept
// its previous contents, a coefficient, and the packed word was wrong.  tests/test_gpu_resize.py compares every byte.)
__device__ __forceinline__ uint32_t resize_clip8(int acc) { return min((uint32_t)acc >> RESIZE_BITS, 255u); }

template <int V, bool TAB>
__global__ __launch_bounds__(RESIZE_THREADS) void k_resize(const uint8_t* __restrict__ data, const int64_t* __restrict__ labels,
                                                           const int64_t* __restrict__ index, float* __restrict__ out_f32,
                                                           uint8_t* __restrict__ out_u8, int64_t* __restrict__ out_labels,
                                                           ResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  // one axis's table is contiguous: xmin [out], count [out], coeff [out, ksize]
  const int nh = a.horiz.coeff ? a.ow * (2 + a.horiz.ksize) : 0, nv = a.vert.coeff ? a.oh * (2 + a.vert.ksize) : 0;
  const int32_t* htab = a.horiz.xmin;
  const int32_t* vtab = a.vert.xmin;
  uint8_t* mid = lds;                                                 // [h, ow]: the horizontal pass's bytes
  if constexpr (TAB) {
    int32_t* tab = reinterpret_cast<int32_t*>(lds);
    for (int i = threadIdx.x; i < nh; i += RESIZE_THREADS) tab[i] = a.horiz.xmin[i];
    for (int i = threadIdx.x; i < nv; i += RESIZE_THREADS) tab[nh + i] = a.vert.xmin[i];
    htab = tab;
    vtab = tab + nh;
    mid = lds + 4 * (size_t)(nh + nv);
    __syncthreads();
  }
  const int32_t* hcoeff = htab + 2 * a.ow;
  const int32_t* vcoeff = vtab + 2 * a.oh;
  const int b = blockIdx.x, c = blockIdx.y, nc = gridDim.y;
  const int64_t item = index[b];
  const bool known = item >= 0 && item < a.n;
  if (c == 0 && threadIdx.x == 0) out_labels[b] = known ? labels[item] : -1;
  const int owv = a.ow / V;

  // pass 1: data[item, c] [h, w] -> mid [h, ow]
  const uint8_t* src = data + ((size_t)(known ? item : 0) * nc + c) * a.h * a.w;
  for (int e = threadIdx.x; e < a.h * owv; e += RESIZE_THREADS) {
    const int y = e / owv, x0 = (e - y * owv) * V;
    const uint8_t* row = src + (size_t)y * a.w;
    uint32_t packed = 0;
    if (known) {
      if (!a.horiz.coeff) {
        if constexpr (V == 4) {
          packed = *reinterpret_cast<const uint32_t*>(row + x0);
        } else {
          packed = row[x0];
        }
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const int xx = x0 + v;
          const int first = htab[xx], taps = htab[a.ow + xx];
          const int32_t* k = hcoeff + (size_t)xx * a.horiz.ksize;
          int acc = 1 << (RESIZE_BITS - 1);
          for (int t = 0; t < taps; ++t) acc += k[t] * (int)row[first + t];
          packed |= (uint32_t)resize_clip8(acc) << (8 * v);
        }
      }
    }
    if constexpr (V == 4) {
      *reinterpret_cast<uint32_t*>(mid + y * a.ow + x0) = packed;
    } else {
      mid[y * a.ow + x0] = (uint8_t)packed;
    }
  }
  __syncthreads();

  // pass 2: mid [h, ow] -> the outputs [oh, ow]
  const size_t plane = ((size_t)b * nc + c) * a.oh * a.ow;
  for (int e = threadIdx.x; e < a.oh * owv; e += RESIZE_THREADS) {
    const int yy = e / owv, x0 = (e - yy * owv) * V;
    uint32_t packed;
    if (!a.vert.coeff) {
      if constexpr (V == 4) {
        packed = *reinterpret_cast<const uint32_t*>(mid + yy * a.ow + x0);
      } else {
        packed = mid[yy * a.ow + x0];
      }
    } else {
      const int first = vtab[yy], taps = vtab[a.oh + yy];
      const int32_t* k = vcoeff + (size_t)yy * a.vert.ksize;
      int acc[V];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = 1 << (RESIZE_BITS - 1);
      for (int t = 0; t < taps; ++t) {
        const int kt = k[t];
        uint32_t word;
        if constexpr (V == 4) {
          word = *reinterpret_cast<const uint32_t*>(mid + (first + t) * a.ow + x0);
        } else {
          word = mid[(first + t) * a.ow + x0];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] += kt * (int)((word >> (8 * v)) & 0xffu);
      }
      packed = 0;
#pragma unroll
      for (int v = 0; v < V; ++v) packed |= (uint32_t)resize_clip8(acc[v]) << (8 * v);
    }
    const size_t at = plane + (size_t)yy * a.ow + x0;
    if (out_u8) {
      if constexpr (V == 4) {
        *reinterpret_cast<uint32_t*>(out_u8 + at) = packed;
      } else {
        out_u8[at] = (uint8_t)packed;
      }
    }
    if (out_f32) {
      float y[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const float x = (float)((packed >> (8 * v)) & 0xffu) / 255.f;          // k_augment's expressions, to the letter
        y[v] = a.normalize ? (x - a.mean[c]) / a.std[c] : x;
      }
      if constexpr (V == 4) {
        *reinterpret_cast<float4*>(out_f32 + at) = make_float4(y[0], y[1], y[2], y[3]);
      } else {
        out_f32[at] = y[0];
      }
    }
  }
}

}  // namespace

void launch_resize(const ResizeArgs& a, int c, const uint8_t* data, const int64_t* labels, const int64_t* index, int batch,
                   float* out_f32, uint8_t* out_u8, int64_t* out_labels, hipStream_t s) {
  const dim3 grid((unsigned)batch, (unsigned)c);
  const size_t mid = ((size_t)a.h * a.ow + 3) & ~(size_t)3;
  const size_t tables = 4 * ((a.horiz.coeff ? (size_t)a.ow * (2 + a.horiz.ksize) : 0) + (a.vert.coeff ? (size_t)a.oh * (2 + a.vert.ksize) : 0));
  const bool tab = mid + tables <= (size_t)RESIZE_LDS_BYTES;
  const size_t lds = mid + (tab ? tables : 0);
  // dword / float4 accesses: every row and plane starts on a multiple of 4 pixels, and so must the tensors
  const bool wide = a.ow % 4 == 0 && (uintptr_t)data % 4 == 0 && (uintptr_t)out_u8 % 4 == 0 &&
                    (uintptr_t)out_f32 % 16 == 0;
  auto* kernel = wide ? (tab ? k_resize<4, true> : k_resize<4, false>) : (tab ? k_resize<1, true> : k_resize<1, false>);
  hipLaunchKernelGGL(kernel, grid, dim3(RESIZE_THREADS), lds, s, data, labels, index, out_f32, out_u8, out_labels, a);
}

}  // namespace node
