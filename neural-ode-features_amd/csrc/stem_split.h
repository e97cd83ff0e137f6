// The exact three-way bf16 split of eight consecutive fp32 channels (stem.h: "triples"), shared by the kernel files that write
// triples: kernels_stem.hip and kernels_stem_banded.hip.
#pragma once
#include "stem.h"

namespace node {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// eight consecutive channels -> three 16-B vectors (v_cvt_pk_bf16_f32 pairs)
__device__ __forceinline__ void split8(const float4& p, const float4& q, u32x4& hh, u32x4& mm, u32x4& ll) {
  const f32x2 v[4] = {{p.x, p.y}, {p.z, p.w}, {q.x, q.y}, {q.z, q.w}};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bf16x2 h = __builtin_convertvector(v[i], bf16x2);
    const f32x2 r = v[i] - __builtin_convertvector(h, f32x2);
    const bf16x2 m = __builtin_convertvector(r, bf16x2);
    const f32x2 r2 = r - __builtin_convertvector(m, f32x2);
    const bf16x2 l = __builtin_convertvector(r2, bf16x2);
    hh[i] = __builtin_bit_cast(unsigned, h);
    mm[i] = __builtin_bit_cast(unsigned, m);
    ll[i] = __builtin_bit_cast(unsigned, l);
  }
}

}  // namespace node
