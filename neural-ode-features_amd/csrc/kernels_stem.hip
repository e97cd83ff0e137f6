// The residual stem in front of the ODE block as hand-written gfx950 kernels (stem.h has the data formats):
//   reference: model.py:167-178 (ResDownsample), model.py:284-310 (ResBlock), model.py:255-265 (conv3x3 / conv1x1),
//   model.py:268-271 (GroupNorm(min(32, C), C)).
// Round 3 ran these seven convolutions through MIOpen: 1.3 ms of the 5.5 ms cfg-2 step, a third of it layout transposes
// and PyTorch reductions around the library's kernels.  Here the stem is NHWC from its first kernel to its last:
//   k_stem_conv      forward convolutions and data gradients of the 64 ... 4096-channel layers (the stems, the trunks, the 4x4
//                    hand-off convolutions; reductions of more than 4096 products in segments: the SEG instance): a gather GEMM over
//                    (tap, input channel) on the bf16 matrix pipe at fp32 accuracy -- both operands arrive as exact bf16
//                    triples, staged global -> LDS by plain 16-B copies (LDS-DMA through a ring of stages), six
//                    v_mfma_f32_32x32x16_bf16 per fp32 product block
//   k_stem_wgrad     weight gradients on the same pipe and triples: the reduction runs over pixels, so the [pixel][channel]
//                    rows go through the same LDS ring as they lie in memory and come out transposed
//                    (ds_read_b64_tr_b16); split-K slabs
//   k_stem_conv0_*   the first layer (K = 9 in_ch <= 27) on the NCHW input
//   k_stem_gn_*      GroupNorm + ReLU forward (writes the triples the next convolution reads) and backward
//   k_stem_prep / k_stem_from_nchw / k_stem_to_nchw / k_stem_reduce   filter splits, boundary layouts, slab sums
#include "stem.h"
#include "stem_split.h"
#include <type_traits>

namespace node {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// x = h + m + l exactly (3 x 8 significant bits; round-to-nearest-even at each level)
__device__ __forceinline__ void split3(float x, bf16_t& h, bf16_t& m, bf16_t& l) {
  const __bf16 bh = (__bf16)x;
  const float r = x - (float)bh;
  const __bf16 bm = (__bf16)r;
  const float r2 = r - (float)bm;
  const __bf16 bl = (__bf16)r2;
  h = __builtin_bit_cast(bf16_t, bh);
  m = __builtin_bit_cast(bf16_t, bm);
  l = __builtin_bit_cast(bf16_t, bl);
}
// (split8, eight consecutive channels -> three 16-B vectors: stem_split.h)
__device__ __forceinline__ float bf16_f(bf16_t v) { return __builtin_bit_cast(float, (unsigned)v << 16); }

// ============================================================================
// LDS images of the two MFMA kernels below: [row][KC channels] bf16, one image per bf16 part, filled by LDS-DMA
// (global_load_lds_dwordx4: one wave instruction = 1 KB = 64 / PP whole rows of PP 16-B pieces; the destination is
// lane-linear, so the XOR swizzle sits on the per-lane SOURCE address).  128-B rows (KC = 64): piece p of row r lives at
// slot p ^ ((r >> 1) & 7); 64-B rows (KC = 32): at slot p ^ ((r >> 2) & 3).  Both the row reads (ds_read_b128, forward /
// data gradient) and the transposed reads (ds_read_b64_tr_b16, weight gradient) of a 16-lane group then touch every bank once.
//
// Operand ring (both kernels): NST = D + 1 stages, D of them in flight.  The DMA pieces are inline asm: the compiler
// neither knows of them nor drains them in front of an LDS read; the only ordering is, per K step q,
//     s_waitcnt vmcnt(pieces of the stages issued behind stage q)   this wave's pieces of stage q have landed
//     s_waitcnt lgkmcnt(0)                                          this wave's reads of stage q - 1 are in registers
//     s_barrier                                                     ... and so have every other wave's
//     issue stage q + D  into the slot of stage q - 1;  read and multiply stage q
// (a stage is read one barrier behind the wait that retires it, and refilled one barrier behind its last read).
// D = 1 is the double-buffered one-step schedule (vmcnt(0) + barrier per step); NODE_TUNE_STEM_RING=0 selects it per call.
// ============================================================================
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef short s16x4 __attribute__((ext_vector_type(4)));
constexpr int STEM_RING_D = 3;
template <int KC>
__device__ __forceinline__ int img_off(int row, int piece) {
  constexpr int PP = KC / 8, SH = KC == 64 ? 1 : 2;
  return row * (2 * KC) + ((piece ^ ((row >> SH) & (PP - 1))) << 4);
}
// 64 / PP rows of one image: lane L brings its 16 bytes to lds_dst + 16 L (M0 is restored inside the statement)
__device__ __forceinline__ void glds16(const bf16_t* src, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(lds_dst) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// all but the pieces of the `ahead` (<= K) youngest stages have landed; NP pieces per stage and wave
template <int NP, int K>
__device__ __forceinline__ void wait_stages(int ahead) {
  if constexpr (K == 0) {
    wait_vm<0>();
  } else {
    if (ahead >= K) wait_vm<K * NP>();
    else wait_stages<NP, K - 1>(ahead);
  }
}
// the six part products of one fp32 product block, smallest first; `between` runs behind every pair (the LDS-DMA pieces of the
// stage being refilled go there: a piece issued between MFMAs costs the wave its issue slot only, nine pieces in a row in
// front of the MFMAs stall it for longer than the MFMAs take)
template <class F>
__device__ __forceinline__ void six_products(f32x16& acc, const bf16x8 (&x)[3], const bf16x8 (&y)[3], F&& between) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[2], y[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[0], y[2], acc, 0, 0, 0);
  between();
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[1], y[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[1], y[0], acc, 0, 0, 0);
  between();
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[0], y[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[0], y[0], acc, 0, 0, 0);
  between();
}
// top of K step q of nq: stage q is complete and the slot of stage q - 1 is free when this returns
template <int NP, int D>
__device__ __forceinline__ void ring_step(int q, int nq) {
  wait_stages<NP, D - 1>(min(q + D - 1, nq - 1) - q);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// ============================================================================
// k_stem_conv<KC, D, SEG>: out[row][co] = sum_{tap, ci} in[row @ tap][ci] * w[tap][co][ci]
//   tile: 128 rows x 64 columns, four waves, wave w = rows 32 w .. 32 w + 31 x both 32-column blocks
//   K chunk: one tap x KC input channels = KC / 16 MFMA K steps of six part products; both operands through the ring above
//   (KC = 32: four stages of 36 KB, three in flight; KC = 64: two of 72 KB), one barrier per chunk
//   a lane stages the same A rows for every chunk (row -> pixel decode once, source rows once per tap); a tap outside the
//   image reads the zero row
//   SEG (long reductions: launch_stem_conv): the accumulators take one segment of STEM_SEG_K products per output, then join a
//   running total and start from zero.  One fp32 accumulator rounds once per MFMA: over the 9216 products of a 3x3 filter on 1024
//   channels that chain came to 8 - 9 x the error of an fp32 CPU convolution (measured: tests/test_gpu_stem_geometry.py), growing
//   with the square root of K; in segments it stays where K = 2048 has it.  SEG = false is the kernel without a total.
// ============================================================================
constexpr int STEM_SEG_K = 2048;
template <int KC, int D, bool SEG>
__global__ __launch_bounds__(256) void k_stem_conv(const SConvArgs a) {
  constexpr int BM = 128, BN = 64, NST = D + 1, KS = KC / 16;
  constexpr int ROWB = 2 * KC, PP = KC / 8, RPI = 64 / PP, SH = KC == 64 ? 1 : 2;
  constexpr int A_PLANE = BM * ROWB, B_PLANE = BN * ROWB, A_BYTES = 3 * A_PLANE, BUF = A_BYTES + 3 * B_PLANE;
  constexpr int NJA = 32 / RPI, NJB = 16 / RPI, NP = 3 * (NJA + NJB);   // DMA pieces per wave: 32 A rows, 16 B rows, three parts
  extern __shared__ __align__(16) unsigned char smem[];
  int* out_off = reinterpret_cast<int*>(smem + NST * BUF);
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int ntn = a.Cout / BN;
  int b = blockIdx.x;
  const int nblk = gridDim.x;
  if ((nblk & 7) == 0) b = (b & 7) * (nblk >> 3) + (b >> 3);   // blocks b, b + 8, .. share an XCD: neighbouring tiles (the same A rows)
  const int ntn_all = (a.mode == 0 && a.w2 != nullptr) ? 2 * ntn : ntn;
  const int tile_m = b / ntn_all;
  int tile_n = b - tile_m * ntn_all;
  const bool shortcut_tile = tile_n >= ntn;        // forward: the shortcut's column tiles
  if (shortcut_tile) tile_n -= ntn;
  // class of this tile (static indices only: a dynamically indexed kernel-argument array would be copied to scratch)
  int tile0 = 0, ch = a.cls_h[0], cw = a.cls_w[0], cpy = a.cls_py[0], cpx = a.cls_px[0], ntap = a.cls_ntap[0];
  unsigned long long taps = a.cls_taps[0];
#pragma unroll
  for (int c = 1; c < 4; ++c)
    if (c < a.nclass && tile_m >= a.cls_tile0[c]) {
      tile0 = a.cls_tile0[c]; ch = a.cls_h[c]; cw = a.cls_w[c]; cpy = a.cls_py[c]; cpx = a.cls_px[c]; ntap = a.cls_ntap[c];
      taps = a.cls_taps[c];
    }
  if (shortcut_tile) { ntap = 1; taps = (unsigned long long)((a.KH >> 1) * a.KW + (a.KW >> 1)); }   // the centre tap
  const bf16_t* wsel = shortcut_tile ? a.w2 : a.w;
  const size_t wsel_plane = shortcut_tile ? a.w2_plane : a.w_plane;
  const int wtaps_one = shortcut_tile ? 1 : 0;     // the shortcut's filter has ONE tap block
  // data gradient: the shortcut's K segment, for the (even, even) class
  const bool extra_k = a.mode == 1 && a.in2 != nullptr && cpy == 0 && cpx == 0 && a.step == 2;
  const int row0 = (tile_m - tile0) * BM;
  const int Mc = a.N * ch * cw;
  // the NJA A rows this lane stages: 32 wave + RPI j + lane / PP
  const int lrow = lane / PP, lslot = lane & (PP - 1);
  int rn[NJA], roy[NJA], rox[NJA];
  bool rval[NJA];
#pragma unroll
  for (int j = 0; j < NJA; ++j) {
    const int rl = 32 * wave + RPI * j + lrow, r = row0 + rl;
    rval[j] = r < Mc;
    rn[j] = roy[j] = rox[j] = 0;
    if (rval[j]) {
      rn[j] = r / (ch * cw);
      const int rem = r - rn[j] * ch * cw;
      const int cy = rem / cw;
      roy[j] = cy * a.step + cpy;
      rox[j] = (rem - cy * cw) * a.step + cpx;
    }
    if (lslot == 0) out_off[rl] = rval[j] ? (rn[j] * a.OH + roy[j]) * a.OW + rox[j] : -1;
  }
  const int ncc = a.Cin / KC;
  const int nseg = ntap + (extra_k ? 1 : 0);       // K segments: the class' taps, then the shortcut's of a data gradient
  const int nchunk = nseg * ncc;

  // the chunk the next issue() brings: (segment i_seg, channel chunk i_cc); per segment, the lane's sources at channel 0
  int i_seg = 0, i_cc = 0;
  const bf16_t* asrc[NJA];
  const bf16_t* bsrc[NJB];
  size_t a_pl = 0, b_pl = 0;
  auto set_segment = [&]() {
    const bool xk = i_seg >= ntap;                   // the shortcut's segment of a data gradient
    const int tap = xk ? 0 : (int)((taps >> (4 * i_seg)) & 15);
    const int ky = tap / a.KW, kx = tap - ky * a.KW;
    const int pad = xk ? 0 : a.pad;
    const bf16_t* in = xk ? a.in2 : a.in;
    const bf16_t* wq = xk ? a.w2 : wsel;
    const int wtap = (xk || wtaps_one) ? 0 : tap;
    a_pl = a.in_plane;
    b_pl = xk ? a.w2_plane : wsel_plane;
#pragma unroll
    for (int j = 0; j < NJA; ++j) {
      int iy, ix;
      bool ok = rval[j];
      if (a.mode == 0) {
        iy = (roy[j] << a.sshift) + ky - pad;
        ix = (rox[j] << a.sshift) + kx - pad;
      } else {
        const int ty = roy[j] + pad - ky, tx = rox[j] + pad - kx;   // divisible by the stride: the class' tap list guarantees it
        ok = ok && ty >= 0 && tx >= 0;
        iy = ty >> a.sshift;
        ix = tx >> a.sshift;
      }
      ok = ok && (unsigned)iy < (unsigned)a.IH && (unsigned)ix < (unsigned)a.IW;
      const int irow = ok ? (rn[j] * a.IH + iy) * a.IW + ix : a.zero_row;
      const int rl = 32 * wave + RPI * j + lrow;
      asrc[j] = in + (size_t)irow * a.Cin + ((lslot ^ ((rl >> SH) & (PP - 1))) << 3);
    }
#pragma unroll
    for (int j = 0; j < NJB; ++j) {
      const int col = 16 * wave + RPI * j + lrow;
      bsrc[j] = wq + ((size_t)wtap * a.Cout + tile_n * BN + col) * a.Cin + ((lslot ^ ((col >> SH) & (PP - 1))) << 3);
    }
  };
  const unsigned lds0 = (unsigned)(size_t)(lds_ptr_t)smem;
  // piece k of NP of the chunk (i_seg, i_cc) into ring slot `stage`: A rows first (row group j, part p), then B
  auto piece = [&](int k, int stage) {
    const bool isb = k >= 3 * NJA;
    const int kk = isb ? k - 3 * NJA : k, j = kk / 3, p = kk - 3 * j;
    const int c0 = i_cc * KC;
    if (!isb) glds16(asrc[j] + p * a_pl + c0, lds0 + stage * BUF + 32 * wave * ROWB + p * A_PLANE + j * RPI * ROWB);
    else glds16(bsrc[j] + p * b_pl + c0, lds0 + stage * BUF + A_BYTES + 16 * wave * ROWB + p * B_PLANE + j * RPI * ROWB);
  };
  auto next_chunk = [&]() {
    if (++i_cc == ncc) {
      i_cc = 0;
      if (++i_seg < nseg) set_segment();
    }
  };

  f32x16 acc[2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[c][i] = 0.f;

  set_segment();
#pragma unroll
  for (int q = 0; q < D; ++q)
    if (q < nchunk) {
#pragma unroll
      for (int k = 0; k < NP; ++k) piece(k, q);
      next_chunk();
    }
  const int li = lane & 31, lg = lane >> 5;
  const int arow = 32 * wave + li;
  int st_read = 0, st_fill = D;                      // ring slots of stage q and of stage q + D
  // one K step; FILL: stage q + D is requested, two MFMAs between its pieces
  auto step = [&](int q, auto fill) {
    constexpr bool FILL = decltype(fill)::value;
    ring_step<NP, D>(q, nchunk);
    const unsigned char* A = smem + st_read * BUF;
    const unsigned char* B = A + A_BYTES;
    // the fragments of K step ks + 1 are requested before the products of step ks issue
    bf16x8 fa[2][3], fb[2][2][3];
    auto fetch = [&](int ks, int s) {
#pragma unroll
      for (int p = 0; p < 3; ++p)
        fa[s][p] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(A + p * A_PLANE + img_off<KC>(arow, 2 * ks + lg)));
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int p = 0; p < 3; ++p)
          fb[s][c][p] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(B + p * B_PLANE + img_off<KC>(32 * c + li, 2 * ks + lg)));
    };
    int pk = 0;
    auto between = [&]() {
      if constexpr (FILL) {
        if (pk < NP) piece(pk, st_fill);
        ++pk;
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    fetch(0, 0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int s = ks & 1;
      if (ks + 1 < KS) fetch(ks + 1, s ^ 1);
      if constexpr (FILL) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < 2; ++c) six_products(acc[c], fa[s], fb[s][c], between);
    }
    static_assert(NP <= 6 * KS, "a chunk's pieces go between its MFMA pairs");
    if constexpr (FILL) next_chunk();
    st_read = st_read + 1 == NST ? 0 : st_read + 1;
    st_fill = st_fill + 1 == NST ? 0 : st_fill + 1;
  };
  int q = 0;
  if constexpr (SEG) {
    constexpr int QSEG = STEM_SEG_K / KC;              // chunks per segment: the same K boundaries at every KC
    f32x16 tot[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int i = 0; i < 16; ++i) tot[c][i] = 0.f;
    auto join = [&]() {
      if ((q + 1) % QSEG == 0 && q + 1 < nchunk) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int i = 0; i < 16; ++i) { tot[c][i] += acc[c][i]; acc[c][i] = 0.f; }
      }
    };
    for (; q + D < nchunk; ++q) { step(q, std::true_type()); join(); }
    for (; q < nchunk; ++q) { step(q, std::false_type()); join(); }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[c][i] = tot[c][i] + acc[c][i];
  } else {
    for (; q + D < nchunk; ++q) step(q, std::true_type());
    for (; q < nchunk; ++q) step(q, std::false_type());
  }

  // epilogue: register r of a 32 x 32 block = row 8 (r / 4) + 4 (lane / 32) + r % 4, column lane % 32: 128-B row stores.
  // The conditions are decided once; every load of a lane is requested before the first is used (a row past the end reads
  // row 0 and stores nothing); the additions keep their order: acc + bias, + res, + out.
  int off[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) off[i] = out_off[32 * wave + 8 * (i >> 2) + 4 * lg + (i & 3)];
  const int col0 = tile_n * BN + li;
  if (shortcut_tile) {
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (off[i] >= 0) a.out2[(size_t)off[i] * a.Cout + col0 + 32 * c] = acc[c][i];
    return;
  }
  const float bv[2] = {a.bias ? a.bias[col0] : 0.f, a.bias ? a.bias[col0 + 32] : 0.f};
  auto finish = [&](auto has_res, auto has_out) {
    constexpr bool RES = decltype(has_res)::value, OUT = decltype(has_out)::value;
    float r[2][16], o[2][16];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const size_t e = (size_t)max(off[i], 0) * a.Cout + col0 + 32 * c;
        if constexpr (RES) r[c][i] = a.res[e];
        if constexpr (OUT) o[c][i] = a.out[e];
      }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float v = acc[c][i] + bv[c];
        if constexpr (RES) v += r[c][i];
        if constexpr (OUT) v += o[c][i];
        if (off[i] >= 0) a.out[(size_t)off[i] * a.Cout + col0 + 32 * c] = v;
      }
  };
  typedef std::true_type yes;
  typedef std::false_type no;
  if (a.res) {
    if (a.accumulate) finish(yes(), yes());
    else finish(yes(), no());
  } else {
    if (a.accumulate) finish(no(), yes());
    else finish(no(), no());
  }
}

// ============================================================================
// k_stem_wgrad<TG, EXTRA, D>: dW[tap][co][ci] = sum_pixels dy[pixel][co] * in[pixel @ tap][ci] on the bf16 matrix pipe at fp32
//   accuracy.  Both operands are triples that already exist (the data gradient reads dy, the forward conv read `in`).
//   The reduction runs over PIXELS, so an MFMA operand is eight consecutive pixels of one channel: the [pixel][channel]
//   LDS images above, read with ds_read_b64_tr_b16 (a 4-row x 16-column block delivered column-major: the transpose is free).
//   workgroup = (64 co x 64 ci tile, one kernel row ky = TG taps of a TG x TG filter, one share of the pixels; TG = 1, 3
//   or 4: 1x1, 3x3 and the 4x4 stride-2 filters); wave w = the 32 x 32 block
//   (w / 2, w % 2) for the TG taps; K chunk = 16 pixels = ONE MFMA K step: a dy image (6 KB) + TG gathered input images,
//   through the ring above (D + 1 stages, D in flight).  Every workgroup writes its TG blocks of one slab; k_stem_reduce
//   sums the slabs.
//   EXTRA (ky == 1 only): the shortcut's 1x1 stride-s filter reads the pixel the centre tap reads -- one more accumulator,
//   fed by the centre tap's input image and a second dy image.
//   The body is compiled per wave (W) and per kind of workgroup (EX): which (image, part, half) pieces a wave brings, and how
//   many, are constants -- no role branches in the loop, and the counted waits are immediates.
// ============================================================================
template <int TG, bool EX, int D, int W>
__device__ __forceinline__ void stem_wgrad_wave(const SWgradArgs& a, unsigned char* smem) {
  constexpr int NST = D + 1;
  constexpr int IMG = 3 * 16 * 128;                 // one image: three parts x 16 pixels x 128 B
  constexpr int NIMG = 1 + TG + (EX ? 1 : 0);       // dy, TG inputs, dy2
  constexpr int BUF = NIMG * IMG;
  constexpr int NINST = NIMG * 6;                   // pieces of a stage: (image, part, half), dealt to the waves in turn:
  constexpr int NP = (NINST - W + 3) / 4;           // wave W brings pieces W, W + 4, ... -- all of the half W & 1
  constexpr int H = W & 1;
  const int lane = threadIdx.x & 63;
  const int nct = a.Cin >> 6, npair = nct * (a.Cout >> 6);
  const int ngrp = TG;                               // kernel rows: one workgroup each
  int bb = blockIdx.x;
  const int pair = bb % npair; bb /= npair;
  const int ky = bb % ngrp;
  const int split = bb / ngrp;
  const int cot = pair / nct, cit = pair - cot * nct;
  const int rows = a.N * a.OH * a.OW;
  const int rbeg = split * a.rows_per_split;
  const int rend = min(rbeg + a.rows_per_split, rows);
  const int nchunk = rbeg < rend ? (rend - rbeg + 15) >> 4 : 0;

  // staging: one piece = 8 pixel rows of one part of one image; lane -> pixel row 8 H + lane / 8 of the chunk, 16-B piece
  // (lane & 7) ^ swizzle.  The lane's pixel (py, px), its source row at tap (ky, 0) and its dy row advance by 16 pixels per
  // chunk: 16 = an OH OW + ay OW + ax with at most one carry per digit, so the step is a handful of adds and selects.
  const int rl = 8 * H + (lane >> 3);
  const int sw = ((lane & 7) ^ ((rl >> 1) & 7)) << 3;
  const int ohw = a.OH * a.OW;
  const int an = 16 / ohw, ay = (16 - an * ohw) / a.OW, ax = 16 - an * ohw - ay * a.OW;
  const int d_irow = (an * a.IH + ay * a.stride) * a.IW + ax * a.stride;
  const int cx_irow = (a.IW - a.OW) * a.stride, cy_irow = (a.IH - a.OH * a.stride) * a.IW;
  int r = rbeg + rl;                                 // the dy row
  int py, px, irow;
  {
    const int pn = r / ohw, rem = r - pn * ohw;
    py = rem / a.OW;
    px = rem - py * a.OW;
    irow = (pn * a.IH + py * a.stride - a.pad + ky) * a.IW + px * a.stride - a.pad;
  }
  const bf16_t* dyb = a.dy3 + cot * 64 + sw;
  const bf16_t* dy2b = EX ? a.dy23 + cot * 64 + sw : nullptr;
  const bf16_t* inb = a.in + cit * 64 + sw;
  const unsigned lds0 = (unsigned)(size_t)(lds_ptr_t)smem;
  // source offsets of the chunk the lane's pixel stands at, then the pixel's step to the next chunk
  size_t dyo, ino[TG];
  auto sources = [&]() {
    const bool valid = r < rend;
    const int iy = py * a.stride - a.pad + ky, ix0 = px * a.stride - a.pad;
    const bool oky = valid && (unsigned)iy < (unsigned)a.IH;
    dyo = (size_t)(valid ? r : a.dy_zero_row) * a.Cout;
#pragma unroll
    for (int kx = 0; kx < TG; ++kx) {
      const bool ok = oky && (unsigned)(ix0 + kx) < (unsigned)a.IW;
      ino[kx] = (size_t)(ok ? irow + kx : a.zero_row) * a.Cin;
    }
    r += 16;
    px += ax; py += ay; irow += d_irow;
    if (px >= a.OW) { px -= a.OW; py += 1; irow += cx_irow; }
    if (py >= a.OH) { py -= a.OH; irow += cy_irow; }
  };
  // piece ii of NP of that chunk into ring slot `stage`
  auto piece = [&](int ii, int stage) {
    const int inst = W + 4 * ii, im = inst / 6, part = (inst % 6) >> 1;      // constants after unrolling
    const int kx = im >= 1 && im <= TG ? im - 1 : 0;
    const bf16_t* src = im == 0 ? dyb + part * a.dy_plane + dyo
                      : im > TG ? dy2b + part * a.dy_plane + dyo
                                : inb + part * a.in_plane + ino[kx];
    glds16(src, lds0 + stage * BUF + im * IMG + part * 2048 + H * 1024);
  };

  constexpr int NA = TG + (EX ? 1 : 0);
  f32x16 acc[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;

  // transposed fragment reads: lane l -> channel column (l & 31) of the wave's block, pixels 8 (l >> 5) .. + 7
  constexpr int cob = W >> 1, cib = W & 1;
  const int kg = lane >> 5, g16 = (lane >> 4) & 1, m = lane & 15, tq = m >> 2, tp = m & 3;
  auto frag = [&](const unsigned char* img, int part, int cb0) -> bf16x8 {
    const int piece = ((cb0 + 16 * g16) >> 3) + (tp >> 1), inb8 = (tp & 1) << 3;
    const int r0 = 8 * kg + tq, r1 = r0 + 4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(img + part * 2048 + img_off<64>(r0, piece) + inb8));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(img + part * 2048 + img_off<64>(r1, piece) + inb8));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  };

#pragma unroll
  for (int q = 0; q < D; ++q)
    if (q < nchunk) {
      sources();
#pragma unroll
      for (int ii = 0; ii < NP; ++ii) piece(ii, q);
    }
  int st_read = 0, st_fill = D;                      // ring slots of stage q and of stage q + D
  // one K step; FILL: stage q + D is requested, two MFMAs between its pieces
  auto step = [&](int q, auto fill) {
    constexpr bool FILL = decltype(fill)::value;
    ring_step<NP, D>(q, nchunk);
    if constexpr (FILL) sources();
    const unsigned char* base = smem + st_read * BUF;
    // every fragment of the step is requested before its first product issues
    bf16x8 fa[3], fb[TG][3], f2[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) fa[p] = frag(base, p, 32 * cob);
#pragma unroll
    for (int j = 0; j < TG; ++j)
#pragma unroll
      for (int p = 0; p < 3; ++p) fb[j][p] = frag(base + (1 + j) * IMG, p, 32 * cib);
    if constexpr (EX) {
#pragma unroll
      for (int p = 0; p < 3; ++p) f2[p] = frag(base + (NIMG - 1) * IMG, p, 32 * cob);
    }
    int pk = 0;
    auto between = [&]() {
      if constexpr (FILL) {
        if (pk < NP) piece(pk, st_fill);
        ++pk;
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    if constexpr (FILL) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < TG; ++j) {
      six_products(acc[j], fa, fb[j], between);
      if constexpr (EX) {
        if (j == 1) six_products(acc[TG], f2, fb[j], between);     // the centre tap's input image once more, against the shortcut's dy
      }
    }
    static_assert(NP <= 3 * NA, "a chunk's pieces go between its MFMA pairs");
    st_read = st_read + 1 == NST ? 0 : st_read + 1;
    st_fill = st_fill + 1 == NST ? 0 : st_fill + 1;
  };
  int q = 0;
  for (; q + D < nchunk; ++q) step(q, std::true_type());
  for (; q < nchunk; ++q) step(q, std::false_type());
  const int li = lane & 31, hh = lane >> 5;
  const int taps_total = TG * TG;
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    float* dst = j < TG ? a.slab + ((size_t)split * taps_total + ky * TG + j) * a.Cout * a.Cin
                        : a.slab2 + (size_t)split * a.Cout * a.Cin;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int co = cot * 64 + 32 * cob + 8 * (i >> 2) + 4 * hh + (i & 3);
      dst[(size_t)co * a.Cin + cit * 64 + 32 * cib + li] = acc[j][i];
    }
  }
}

template <int TG, bool EX, int D>
__device__ __forceinline__ void stem_wgrad_waves(const SWgradArgs& a, unsigned char* smem, int wave) {
  if (wave == 0) stem_wgrad_wave<TG, EX, D, 0>(a, smem);
  else if (wave == 1) stem_wgrad_wave<TG, EX, D, 1>(a, smem);
  else if (wave == 2) stem_wgrad_wave<TG, EX, D, 2>(a, smem);
  else stem_wgrad_wave<TG, EX, D, 3>(a, smem);
}

template <int TG, bool EXTRA, int D>
__global__ __launch_bounds__(256) void k_stem_wgrad(const SWgradArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if constexpr (EXTRA) {
    const int npair = (a.Cin >> 6) * (a.Cout >> 6);
    if ((blockIdx.x / npair) % 3 == 1) {               // the ky == 1 workgroups carry the shortcut's accumulator
      stem_wgrad_waves<TG, true, D>(a, smem, wave);
      return;
    }
  }
  stem_wgrad_waves<TG, false, D>(a, smem, wave);
}

// ============================================================================
// first layer: nn.Conv2d(in_ch, 64, 3, 1), no padding, bias; x is NCHW.  K = 9 in_ch (<= 27, padded to 28 by zero filter rows)
// ============================================================================
__global__ __launch_bounds__(256) void k_stem_conv0_fwd(const float* __restrict__ x, const float* __restrict__ w0t,
                                                        const float* __restrict__ bias, float* __restrict__ h0, int N, int Cin, int H,
                                                        int W) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, hh = lane >> 5;
  const int OH = H - 2, OW = W - 2, rows = N * OH * OW, K = 9 * Cin;
  const int row0 = (blockIdx.x * 4 + wave) * 32;
  if (row0 >= rows) return;
  const int r = row0 + li;
  const bool valid = r < rows;
  int base = 0;
  if (valid) {
    const int n = r / (OH * OW), rem = r - n * OH * OW, oy = rem / OW, ox = rem - oy * OW;
    base = (n * Cin * H + oy) * W + ox;
  }
  f32x16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
  const int steps = (K + 1) >> 1;
  for (int s = 0; s < steps; ++s) {
    const int k = 2 * s + hh, kk = min(k, K - 1);
    const int ci = kk / 9, rem = kk - 9 * ci, ky = rem / 3, kx = rem - 3 * ky;
    const float av = valid ? x[base + (ci * H + ky) * W + kx] : 0.f;     // (k >= K meets a zero filter row)
    const float b0 = w0t[k * 64 + li], b1 = w0t[k * 64 + 32 + li];
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc1, 0, 0, 0);
  }
  const float bv0 = bias[li], bv1 = bias[32 + li];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int rr = row0 + 8 * (i >> 2) + 4 * hh + (i & 3);
    if (rr >= rows) continue;
    h0[(size_t)rr * 64 + li] = acc0[i] + bv0;
    h0[(size_t)rr * 64 + 32 + li] = acc1[i] + bv1;
  }
}

// dW0[co][k] = sum_rows dh0[row][co] * patch(row)[k]; column K carries the bias gradient (a constant-one operand)
__global__ __launch_bounds__(256) void k_stem_conv0_wgrad(const float* __restrict__ x, const float* __restrict__ dh0,
                                                          float* __restrict__ slab, int N, int Cin, int H, int W, int rows_per_split) {
  __shared__ float red[2 * 16 * 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, hh = lane >> 5;
  const int OH = H - 2, OW = W - 2, rows = N * OH * OW, K = 9 * Cin;
  const int per_wave = rows_per_split >> 2;
  const int rbeg = blockIdx.x * rows_per_split + wave * per_wave;
  const int rend = min(rbeg + per_wave, rows);
  int koff = 0;
  if (li < K) {
    const int ci = li / 9, rem = li - 9 * ci, ky = rem / 3;
    koff = (ci * H + ky) * W + (rem - 3 * ky);
  }
  int r = rbeg + hh;
  int n = 0, oy = 0, ox = 0;
  if (r < rows) {
    n = r / (OH * OW);
    const int rem = r - n * OH * OW;
    oy = rem / OW;
    ox = rem - oy * OW;
  }
  f32x16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
  for (; r - hh < rend; r += 2) {
    const bool valid = r < rend;
    const float a0 = valid ? dh0[(size_t)r * 64 + li] : 0.f;
    const float a1 = valid ? dh0[(size_t)r * 64 + 32 + li] : 0.f;
    float bv = 0.f;
    if (valid) bv = li < K ? x[(n * Cin * H + oy) * W + ox + koff] : (li == K ? 1.f : 0.f);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc1, 0, 0, 0);
    ox += 2;
    if (ox >= OW) {
      ox -= OW;
      oy += 1;
      if (oy >= OH) { oy = 0; n += 1; }
    }
  }
  for (int w = 1; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int i = 0; i < 16; ++i) { red[i * 64 + lane] = acc0[i]; red[(16 + i) * 64 + lane] = acc1[i]; }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int i = 0; i < 16; ++i) { acc0[i] += red[i * 64 + lane]; acc1[i] += red[(16 + i) * 64 + lane]; }
    }
    __syncthreads();
  }
  if (wave != 0) return;
  float* dst = slab + (size_t)blockIdx.x * 64 * 32;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int co = 8 * (i >> 2) + 4 * hh + (i & 3);
    dst[co * 32 + li] = acc0[i];
    dst[(32 + co) * 32 + li] = acc1[i];
  }
}

// d_x[n][ci][y][x] = sum_co sum_ky,kx dh0[n][y - ky][x - kx][co] * w0[co][ci][ky][kx]: the transposed first layer, 64 -> Cin <= 3
// channels.  One workgroup per (sample, DG_TH x DG_TW tile of IMAGE pixels):
//   1. P[pixel][k] = sum_co dh0[pixel][co] * w0[co][k] for the (DG_TH + 2) x (DG_TW + 2) pixels of dh0 that reach the tile, on the
//      fp32 matrix instruction (32 pixels x 28 columns per wave tile, K = 64 channels: lane half hh owns channels 32 hh .. 32 hh + 31 of
//      its pixel, eight float4 loads of one NHWC row), the tile in LDS; a pixel outside dh0 is a zero row, so
//   2. every image pixel gathers nine entries of P in one fixed order (border pixels: the taps that fall outside are those zero rows).
// fp32 throughout, no atomics: the same bits on every run.
constexpr int DG_TH = 8, DG_TW = 32, DG_PH = DG_TH + 2, DG_PW = DG_TW + 2, DG_NP = DG_PH * DG_PW, DG_NT = (DG_NP + 31) / 32, DG_PS = 29;
__global__ __launch_bounds__(256) void k_stem_conv0_dgrad(const float* __restrict__ dh0, const float* __restrict__ w0,
                                                          float* __restrict__ dx, int Cin, int H, int W, int tiles_x, int tiles_y) {
  __shared__ float P[DG_NT * 32 * DG_PS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, hh = lane >> 5;
  const int OH = H - 2, OW = W - 2, K = 9 * Cin;
  const int n = blockIdx.x / (tiles_x * tiles_y), rem = blockIdx.x - n * tiles_x * tiles_y, ty = rem / tiles_x, tx = rem - ty * tiles_x;
  const int y0 = ty * DG_TH, x0 = tx * DG_TW;
  float b[32];                     // w0[32 hh + s][li]: the filter as [64][K], column li (columns >= K are zero)
#pragma unroll
  for (int s = 0; s < 32; ++s) b[s] = li < K ? w0[(32 * hh + s) * K + li] : 0.f;
  for (int tile = wave; tile < DG_NT; tile += 4) {
    const int pix = tile * 32 + li, py = pix / DG_PW, px = pix - py * DG_PW;
    const int oy = y0 - 2 + py, ox = x0 - 2 + px;
    const bool valid = pix < DG_NP && oy >= 0 && oy < OH && ox >= 0 && ox < OW;
    float4 av[8];
    if (valid) {
      const float4* src = reinterpret_cast<const float4*>(dh0 + ((size_t)(n * OH + oy) * OW + ox) * 64 + 32 * hh);
#pragma unroll
      for (int q = 0; q < 8; ++q) av[q] = src[q];
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) av[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].x, b[4 * q], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].y, b[4 * q + 1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].z, b[4 * q + 2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].w, b[4 * q + 3], acc, 0, 0, 0);
    }
    if (li < 28) {
#pragma unroll
      for (int i = 0; i < 16; ++i) P[(tile * 32 + 8 * (i >> 2) + 4 * hh + (i & 3)) * DG_PS + li] = acc[i];
    }
  }
  __syncthreads();
  for (int idx = t; idx < Cin * DG_TH * DG_TW; idx += 256) {
    const int xx = idx % DG_TW, yy = (idx / DG_TW) % DG_TH, ci = idx / (DG_TW * DG_TH);
    const int y = y0 + yy, x = x0 + xx;
    if (y >= H || x >= W) continue;
    float s = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) s += P[((yy + 2 - ky) * DG_PW + xx + 2 - kx) * DG_PS + ci * 9 + ky * 3 + kx];
    dx[((size_t)(n * Cin + ci) * H + y) * W + x] = s;
  }
}

// ============================================================================
// GroupNorm + ReLU.  One workgroup per (sample, CB channels); the block [HW][CB] lives in LDS.
//   thread -> channel t % CB (fixed), pixels t / CB, t / CB + 256 / CB, ...; group sums through LDS
// ============================================================================
__device__ __forceinline__ void group_sums(float v, float* red, float* grp, int CB, int cpg, int t) {
  // red[256] <- v; grp[g] <- sum of the threads whose channel lies in group g.  Two barriers.
  red[t] = v;
  __syncthreads();
  const int ngrp = CB / cpg;
  if (t < ngrp) {
    float s = 0.f;
    for (int j = 0; j < 256 / CB; ++j)
      for (int k = 0; k < cpg; ++k) s += red[j * CB + t * cpg + k];
    grp[t] = s;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void k_stem_gn_fwd(const SGnArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int t = threadIdx.x;
  const int CB = a.CB, HW = a.HW, C = a.C;
  // (no static __shared__ next to a dynamic region that may need the whole LDS: hipFuncSetAttribute refuses their sum)
  float* tile = reinterpret_cast<float*>(smem);
  float* red = tile + (size_t)HW * CB;      // [256]
  float* gmean = red + 256;                 // [128]
  float* grstd = gmean + 128;               // [128]
  const int nblk = C / CB;
  const int n = blockIdx.x / nblk, c0 = (blockIdx.x - n * nblk) * CB;
  const int q4 = CB >> 2;
  const float* src = a.h + ((size_t)n * HW) * C + c0;
  for (int idx = t; idx < HW * q4; idx += 256) {
    const int px = idx / q4, q = idx - px * q4;
    *reinterpret_cast<float4*>(tile + px * CB + 4 * q) = *reinterpret_cast<const float4*>(src + (size_t)px * C + 4 * q);
  }
  __syncthreads();
  const int c = t & (CB - 1), pg = t / CB, PG = 256 / CB;
  const float inv_m = 1.f / (float)(a.cpg * HW);
  float s = 0.f;
  for (int px = pg; px < HW; px += PG) s += tile[px * CB + c];
  group_sums(s, red, gmean, CB, a.cpg, t);
  const float mean = gmean[c / a.cpg] * inv_m;
  float s2 = 0.f;
  for (int px = pg; px < HW; px += PG) {
    const float d = tile[px * CB + c] - mean;
    s2 = __builtin_fmaf(d, d, s2);      // (what `s2 += d * d` compiled to here; written out because k_stem_gn_fwd_fl must round the same way)
  }
  group_sums(s2, red, grstd, CB, a.cpg, t);
  const int ngrp = CB / a.cpg;
  if (t < ngrp) {
    const float m = gmean[t] * inv_m, rs = rsqrtf(grstd[t] * inv_m + a.eps);
    float* st = a.stats + ((size_t)n * (C / a.cpg) + c0 / a.cpg + t) * 2;
    st[0] = m;
    st[1] = rs;
  }
  __syncthreads();
  if (t < ngrp) {     // (second barrier of group_sums is behind every read of grstd above)
    const float m = gmean[t] * inv_m, rs = rsqrtf(grstd[t] * inv_m + a.eps);
    gmean[t] = m;
    grstd[t] = rs;
  }
  __syncthreads();
  const int q8 = CB >> 3;
  for (int idx = t; idx < HW * q8; idx += 256) {
    const int px = idx / q8, q = idx - px * q8;
    const float4 p0 = *reinterpret_cast<const float4*>(tile + px * CB + 8 * q);
    const float4 p1 = *reinterpret_cast<const float4*>(tile + px * CB + 8 * q + 4);
    float v[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int cc = 8 * q + k, g = cc / a.cpg;
      const float y = (v[k] - gmean[g]) * grstd[g] * a.gamma[c0 + cc] + a.beta[c0 + cc];
      v[k] = fmaxf(y, 0.f);
    }
    u32x4 hh, mm, ll;
    split8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), hh, mm, ll);
    bf16_t* dst = a.a3 + ((size_t)n * HW + px) * C + c0 + 8 * q;
    *reinterpret_cast<u32x4*>(dst) = hh;
    *reinterpret_cast<u32x4*>(dst + a.a_plane) = mm;
    *reinterpret_cast<u32x4*>(dst + 2 * a.a_plane) = ll;
  }
}

// backward: da = dL/d relu(GN(h)).  dy = da where the activation is positive; dgamma_c = sum dy xhat, dbeta_c = sum dy;
// dh = rstd (dy gamma - (s1 + xhat s2) / m) with s1 = sum_group gamma dbeta, s2 = sum_group gamma dgamma
// SKIP (the residual trunk's block boundary, trunk_api.hip): h also feeds the block's identity shortcut, so its gradient is
// dh + skip, skip = dL/d(block output); the sum is the next block's output gradient and leaves as fp32 and / or triples.
template <bool SKIP>
__global__ __launch_bounds__(256) void k_stem_gn_bwd(const SGnArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int CB = a.CB, HW = a.HW, C = a.C;
  float* txh = reinterpret_cast<float*>(smem);          // h, then xhat
  float* tdy = txh + (size_t)HW * CB;                     // da, then dy
  float* redA = tdy + (size_t)HW * CB;                    // [256]
  float* redB = redA + 256;                               // [256]
  float* gmean = redB + 256;                              // [128] each
  float* grstd = gmean + 128;
  float* gs1 = grstd + 128;
  float* gs2 = gs1 + 128;
  const int t = threadIdx.x;
  const int nblk = C / CB;
  const int n = blockIdx.x / nblk, c0 = (blockIdx.x - n * nblk) * CB;
  const int q4 = CB >> 2;
  const float* sh = a.h + ((size_t)n * HW) * C + c0;
  const float* sd = a.da + ((size_t)n * HW) * C + c0;
  for (int idx = t; idx < HW * q4; idx += 256) {
    const int px = idx / q4, q = idx - px * q4;
    *reinterpret_cast<float4*>(txh + px * CB + 4 * q) = *reinterpret_cast<const float4*>(sh + (size_t)px * C + 4 * q);
    *reinterpret_cast<float4*>(tdy + px * CB + 4 * q) = *reinterpret_cast<const float4*>(sd + (size_t)px * C + 4 * q);
  }
  const int ngrp = CB / a.cpg;
  if (t < ngrp) {
    const float* st = a.stats + ((size_t)n * (C / a.cpg) + c0 / a.cpg + t) * 2;
    gmean[t] = st[0];
    grstd[t] = st[1];
  }
  __syncthreads();
  const int c = t & (CB - 1), pg = t / CB, PG = 256 / CB;
  const float mean = gmean[c / a.cpg], rstd = grstd[c / a.cpg], gam = a.gamma[c0 + c], bet = a.beta[c0 + c];
  float sA = 0.f, sB = 0.f;
  for (int px = pg; px < HW; px += PG) {
    const float xh = (txh[px * CB + c] - mean) * rstd;
    const float y = xh * gam + bet;
    const float dy = y > 0.f ? tdy[px * CB + c] : 0.f;
    txh[px * CB + c] = xh;
    tdy[px * CB + c] = dy;
    sA += dy;
    sB += dy * xh;
  }
  redA[t] = sA;
  redB[t] = sB;
  __syncthreads();
  if (t < CB) {
    float A = 0.f, B = 0.f;
    for (int j = 0; j < PG; ++j) { A += redA[j * CB + t]; B += redB[j * CB + t]; }
    a.gpart[((size_t)n * 2 + 0) * C + c0 + t] = B;      // dgamma
    a.gpart[((size_t)n * 2 + 1) * C + c0 + t] = A;      // dbeta
    redA[t] = A * gam;      // (t < CB: c == t)
    redB[t] = B * gam;
  }
  __syncthreads();
  if (t < ngrp) {
    float s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < a.cpg; ++k) { s1 += redA[t * a.cpg + k]; s2 += redB[t * a.cpg + k]; }
    gs1[t] = s1;
    gs2[t] = s2;
  }
  __syncthreads();
  const float inv_m = 1.f / (float)(a.cpg * HW);
  const int q8 = CB >> 3;
  for (int idx = t; idx < HW * q8; idx += 256) {
    const int px = idx / q8, q = idx - px * q8;
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int cc = 8 * q + k, g = cc / a.cpg;
      const float xh = txh[px * CB + cc], dy = tdy[px * CB + cc];
      v[k] = grstd[g] * (dy * a.gamma[c0 + cc] - (gs1[g] + xh * gs2[g]) * inv_m);
    }
    const size_t o = ((size_t)n * HW + px) * C + c0 + 8 * q;
    if constexpr (SKIP) {
      const float4 k0 = *reinterpret_cast<const float4*>(a.skip + o), k1 = *reinterpret_cast<const float4*>(a.skip + o + 4);
      v[0] += k0.x; v[1] += k0.y; v[2] += k0.z; v[3] += k0.w;
      v[4] += k1.x; v[5] += k1.y; v[6] += k1.z; v[7] += k1.w;
    }
    const float4 p0 = make_float4(v[0], v[1], v[2], v[3]), p1 = make_float4(v[4], v[5], v[6], v[7]);
    if (a.dh) {
      *reinterpret_cast<float4*>(a.dh + o) = p0;
      *reinterpret_cast<float4*>(a.dh + o + 4) = p1;
    }
    if (a.dh3) {
      u32x4 hh, mm, ll;
      split8(p0, p1, hh, mm, ll);
      *reinterpret_cast<u32x4*>(a.dh3 + o) = hh;
      *reinterpret_cast<u32x4*>(a.dh3 + o + a.dh_plane) = mm;
      *reinterpret_cast<u32x4*>(a.dh3 + o + 2 * a.dh_plane) = ll;
    }
  }
}

// ----------------------------------------------------------------------------
// The same two passes with their requests kept in flight (the default; NODE_TUNE_STEM_GN=0 launches the kernels above).
// Every sum is the chain of additions it is above, so the results are the same bits:
//   * block, grid and the thread -> (channel, pixels pg, pg + PG, ...) assignment of the statistics are the ones above; which
//     (sample, block) a workgroup takes is not (gn_block_id);
//   * the fill issues GN_NB independent 16-byte loads per thread before the first LDS write (the last, partial batch re-reads
//     the block's last request instead of branching around loads, and drops the copies into `dump`: 16 bytes of the sums'
//     scratch, which nothing reads before the barrier behind the fill);
//   * the serial sums read their LDS operands eight at a time ahead of the additions, which stay in order;
//   * the store loop holds its eight channels' gamma / beta / statistics in registers (a thread's channels never change:
//     256 % (CB / 8) == 0).
// CB and cpg are powers of two here (stem_gn_cb refuses every other shape).
// Measured and not kept (profiles/stem_gn_ab.txt): narrower channel blocks under the same summation stride, i.e. more and smaller
// workgroups per CU.  With a sample's blocks in one L2 (gn_block_id) blocks half as wide took 1.3 us off each 15 x 15 backward
// (15.4 -> 14.1) and nothing off the other four launches; 8-channel blocks made the 30 x 30 launches 20 - 25 % slower.
// ----------------------------------------------------------------------------
constexpr int GN_NB = 8;
__device__ __forceinline__ int gn_log2(int v) { return 31 - __clz(v); }
// Workgroups b and b + 8 share an XCD and its L2.  A block of 16 channels is 64 bytes of every 128-byte line of its sample's rows
// (32 of the triples' lines): dealt out in launch order, the C / CB blocks of a sample sit on different XCDs, each line is fetched
// by several L2s and leaves them in pieces.  This id gives every XCD a contiguous run of (sample, block) pairs instead, so a
// sample's blocks meet in one L2.  A bijection for every grid size; which block a workgroup takes changes no result: on a part
// or partition mode that deals workgroups out differently (another XCD count, no round-robin) only the locality is lost.
__device__ __forceinline__ int gn_block_id() {
  const int b = blockIdx.x, q = gridDim.x >> 3, r = gridDim.x & 7, x = b & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}

template <int NS>
__device__ __forceinline__ void gn_fill(float* tile0, const float* __restrict__ src0, float* tile1, const float* __restrict__ src1,
                                        float* dump, int C, int lq4, int total, int t) {
  const int qm = (1 << lq4) - 1;
  int idx = t;
  for (; idx + (GN_NB - 1) * 256 < total; idx += GN_NB * 256) {
    float4 r0[GN_NB], r1[GN_NB];
#pragma unroll
    for (int u = 0; u < GN_NB; ++u) {
      const int i = idx + 256 * u;
      const size_t o = (size_t)(i >> lq4) * C + 4 * (i & qm);
      r0[u] = *reinterpret_cast<const float4*>(src0 + o);
      if constexpr (NS == 2) r1[u] = *reinterpret_cast<const float4*>(src1 + o);
    }
#pragma unroll
    for (int u = 0; u < GN_NB; ++u) {
      *reinterpret_cast<float4*>(tile0 + 4 * (idx + 256 * u)) = r0[u];      // (pixel * CB + 4 q = 4 i)
      if constexpr (NS == 2) *reinterpret_cast<float4*>(tile1 + 4 * (idx + 256 * u)) = r1[u];
    }
  }
  if (idx < total) {
    float4 r0[GN_NB], r1[GN_NB];
#pragma unroll
    for (int u = 0; u < GN_NB; ++u) {
      const int i = min(idx + 256 * u, total - 1);
      const size_t o = (size_t)(i >> lq4) * C + 4 * (i & qm);
      r0[u] = *reinterpret_cast<const float4*>(src0 + o);
      if constexpr (NS == 2) r1[u] = *reinterpret_cast<const float4*>(src1 + o);
    }
#pragma unroll
    for (int u = 0; u < GN_NB; ++u) {       // (an `if` around the write would take its load along: one request per branch)
      const bool real = idx + 256 * u < total;
      *reinterpret_cast<float4*>(real ? tile0 + 4 * (idx + 256 * u) : dump) = r0[u];
      if constexpr (NS == 2) *reinterpret_cast<float4*>(real ? tile1 + 4 * (idx + 256 * u) : dump) = r1[u];
    }
  }
}

// group_sums with the operands of each chain read eight ahead: grp[g] = ((red[g cpg] + red[g cpg + 1]) + ... ) over
// (j, k), j < PG outer, k < cpg inner -- the order above
__device__ __forceinline__ void group_sums_ahead(float v, float* red, float* grp, int CB, int lcpg, int PG, int t) {
  red[t] = v;
  __syncthreads();
  if (t < (CB >> lcpg)) {
    const float* r0 = red + (t << lcpg);
    const int n = PG << lcpg, km = (1 << lcpg) - 1;
    float s = 0.f;
    for (int i = 0; i < n; i += 8) {
      float x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int ii = min(i + u, n - 1);
        x[u] = r0[(ii >> lcpg) * CB + (ii & km)];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (i + u < n) s += x[u];
    }
    grp[t] = s;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void k_stem_gn_fwd_fl(const SGnArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int t = threadIdx.x;
  const int CB = a.CB, HW = a.HW, C = a.C;
  float* tile = reinterpret_cast<float*>(smem);
  float* red = tile + (size_t)HW * CB;      // [256]
  float* gmean = red + 256;                 // [128]
  float* grstd = gmean + 128;               // [128]
  const int nblk = C / CB, bid = gn_block_id();
  const int n = bid / nblk, c0 = (bid - n * nblk) * CB;
  const int lcb = gn_log2(CB), lcpg = gn_log2(a.cpg);
  gn_fill<1>(tile, a.h + ((size_t)n * HW) * C + c0, nullptr, nullptr, red, C, lcb - 2, HW << (lcb - 2), t);
  __syncthreads();
  const int c = t & (CB - 1), pg = t >> lcb, PG = 256 >> lcb;
  const float inv_m = 1.f / (float)(a.cpg * HW);
  float s = 0.f;
#pragma unroll 4
  for (int px = pg; px < HW; px += PG) s += tile[px * CB + c];
  group_sums_ahead(s, red, gmean, CB, lcpg, PG, t);
  const float mean = gmean[c >> lcpg] * inv_m;
  float s2 = 0.f;
#pragma unroll 4
  for (int px = pg; px < HW; px += PG) {
    const float d = tile[px * CB + c] - mean;
    s2 = __builtin_fmaf(d, d, s2);      // (as above; left to contraction, the unrolled loop multiplies in pairs and adds: two roundings)
  }
  group_sums_ahead(s2, red, grstd, CB, lcpg, PG, t);
  const int ngrp = CB >> lcpg;
  if (t < ngrp) {
    const float m = gmean[t] * inv_m, rs = rsqrtf(grstd[t] * inv_m + a.eps);
    float* st = a.stats + ((size_t)n * (C >> lcpg) + (c0 >> lcpg) + t) * 2;
    st[0] = m;
    st[1] = rs;
  }
  __syncthreads();
  if (t < ngrp) {
    const float m = gmean[t] * inv_m, rs = rsqrtf(grstd[t] * inv_m + a.eps);
    gmean[t] = m;
    grstd[t] = rs;
  }
  __syncthreads();
  const int lq8 = lcb - 3, q = t & ((1 << lq8) - 1), pstep = 256 >> lq8;
  float gm[8], gr[8], ga[8], be[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int cc = 8 * q + k, g = cc >> lcpg;
    gm[k] = gmean[g];
    gr[k] = grstd[g];
    ga[k] = a.gamma[c0 + cc];
    be[k] = a.beta[c0 + cc];
  }
#pragma unroll 2
  for (int px = t >> lq8; px < HW; px += pstep) {
    const float4 p0 = *reinterpret_cast<const float4*>(tile + px * CB + 8 * q);
    const float4 p1 = *reinterpret_cast<const float4*>(tile + px * CB + 8 * q + 4);
    float v[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float y = (v[k] - gm[k]) * gr[k] * ga[k] + be[k];
      v[k] = fmaxf(y, 0.f);
    }
    u32x4 hh, mm, ll;
    split8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), hh, mm, ll);
    bf16_t* dst = a.a3 + ((size_t)n * HW + px) * C + c0 + 8 * q;
    *reinterpret_cast<u32x4*>(dst) = hh;
    *reinterpret_cast<u32x4*>(dst + a.a_plane) = mm;
    *reinterpret_cast<u32x4*>(dst + 2 * a.a_plane) = ll;
  }
}

template <bool SKIP>
__global__ __launch_bounds__(256) void k_stem_gn_bwd_fl(const SGnArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int CB = a.CB, HW = a.HW, C = a.C;
  float* txh = reinterpret_cast<float*>(smem);          // h, then xhat
  float* tdy = txh + (size_t)HW * CB;                     // da, then dy
  float* redA = tdy + (size_t)HW * CB;                    // [256]
  float* redB = redA + 256;                               // [256]
  float* gmean = redB + 256;                              // [128] each
  float* grstd = gmean + 128;
  float* gs1 = grstd + 128;
  float* gs2 = gs1 + 128;
  const int t = threadIdx.x;
  const int nblk = C / CB, bid = gn_block_id();
  const int n = bid / nblk, c0 = (bid - n * nblk) * CB;
  const int lcb = gn_log2(CB), lcpg = gn_log2(a.cpg);
  gn_fill<2>(txh, a.h + ((size_t)n * HW) * C + c0, tdy, a.da + ((size_t)n * HW) * C + c0, redA, C, lcb - 2, HW << (lcb - 2), t);
  const int ngrp = CB >> lcpg;
  if (t < ngrp) {
    const float* st = a.stats + ((size_t)n * (C >> lcpg) + (c0 >> lcpg) + t) * 2;
    gmean[t] = st[0];
    grstd[t] = st[1];
  }
  __syncthreads();
  const int c = t & (CB - 1), pg = t >> lcb, PG = 256 >> lcb;
  const float mean = gmean[c >> lcpg], rstd = grstd[c >> lcpg], gam = a.gamma[c0 + c], bet = a.beta[c0 + c];
  float sA = 0.f, sB = 0.f;
#pragma unroll 4
  for (int px = pg; px < HW; px += PG) {
    const float xh = (txh[px * CB + c] - mean) * rstd;
    const float y = xh * gam + bet;
    const float dy = y > 0.f ? tdy[px * CB + c] : 0.f;
    txh[px * CB + c] = xh;
    tdy[px * CB + c] = dy;
    sA += dy;
    sB += dy * xh;
  }
  redA[t] = sA;
  redB[t] = sB;
  __syncthreads();
  if (t < CB) {
    float A = 0.f, B = 0.f;
    for (int j0 = 0; j0 < PG; j0 += 8) {
      float xa[8], xb[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int j = min(j0 + u, PG - 1);
        xa[u] = redA[j * CB + t];
        xb[u] = redB[j * CB + t];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (j0 + u < PG) { A += xa[u]; B += xb[u]; }
    }
    a.gpart[((size_t)n * 2 + 0) * C + c0 + t] = B;      // dgamma
    a.gpart[((size_t)n * 2 + 1) * C + c0 + t] = A;      // dbeta
    redA[t] = A * gam;      // (t < CB: c == t)
    redB[t] = B * gam;
  }
  __syncthreads();
  if (t < ngrp) {
    float s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < a.cpg; ++k) { s1 += redA[t * a.cpg + k]; s2 += redB[t * a.cpg + k]; }
    gs1[t] = s1;
    gs2[t] = s2;
  }
  __syncthreads();
  const float inv_m = 1.f / (float)(a.cpg * HW);
  const int lq8 = lcb - 3, q = t & ((1 << lq8) - 1), pstep = 256 >> lq8;
  float gr[8], ga[8], g1[8], g2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int cc = 8 * q + k, g = cc >> lcpg;
    gr[k] = grstd[g];
    ga[k] = a.gamma[c0 + cc];
    g1[k] = gs1[g];
    g2[k] = gs2[g];
  }
  // (SKIP: one pixel per trip -- over two, the compiler waited for each of the four `skip` loads on its own)
  constexpr int PX_PER_TRIP = SKIP ? 1 : 2;
#pragma unroll PX_PER_TRIP
  for (int px = t >> lq8; px < HW; px += pstep) {
    const size_t o = ((size_t)n * HW + px) * C + c0 + 8 * q;
    float4 k0, k1;
    if constexpr (SKIP) {
      k0 = *reinterpret_cast<const float4*>(a.skip + o);
      k1 = *reinterpret_cast<const float4*>(a.skip + o + 4);
    }
    const float4 x0 = *reinterpret_cast<const float4*>(txh + px * CB + 8 * q), x1 = *reinterpret_cast<const float4*>(txh + px * CB + 8 * q + 4);
    const float4 d0 = *reinterpret_cast<const float4*>(tdy + px * CB + 8 * q), d1 = *reinterpret_cast<const float4*>(tdy + px * CB + 8 * q + 4);
    const float xs[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w}, ds[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float xh = xs[k], dy = ds[k];
      v[k] = gr[k] * (dy * ga[k] - (g1[k] + xh * g2[k]) * inv_m);
    }
    if constexpr (SKIP) {
      v[0] += k0.x; v[1] += k0.y; v[2] += k0.z; v[3] += k0.w;
      v[4] += k1.x; v[5] += k1.y; v[6] += k1.z; v[7] += k1.w;
    }
    const float4 p0 = make_float4(v[0], v[1], v[2], v[3]), p1 = make_float4(v[4], v[5], v[6], v[7]);
    if (a.dh) {
      *reinterpret_cast<float4*>(a.dh + o) = p0;
      *reinterpret_cast<float4*>(a.dh + o + 4) = p1;
    }
    if (a.dh3) {
      u32x4 hh, mm, ll;
      split8(p0, p1, hh, mm, ll);
      *reinterpret_cast<u32x4*>(a.dh3 + o) = hh;
      *reinterpret_cast<u32x4*>(a.dh3 + o + a.dh_plane) = mm;
      *reinterpret_cast<u32x4*>(a.dh3 + o + 2 * a.dh_plane) = ll;
    }
  }
}

// ============================================================================
// boundary layouts: NCHW fp32 <-> NHWC (fp32 and / or triples); 64 channels x 64 pixels per workgroup through LDS
// ============================================================================
// bpart (nullable) [N * ceil(HW / 64)][C]: per-channel sums of the workgroup's 64 pixels, taken in pixel order -- the partial sums of
// a bias gradient when src is a convolution's output gradient (k_stem_reduce kind 3 adds them up)
__global__ __launch_bounds__(256) void k_stem_from_nchw(const float* __restrict__ src, float* __restrict__ dst, bf16_t* __restrict__ dst3,
                                                        size_t plane, int C, int HW, float* __restrict__ bpart) {
  __shared__ float tile[64][65];
  const int t = threadIdx.x;
  const int npb = (HW + 63) / 64, ncb = C / 64;
  const int n = blockIdx.x / (npb * ncb), rem = blockIdx.x - n * npb * ncb, cb = rem / npb, pb = rem - cb * npb;
  const int c0 = cb * 64, p0 = pb * 64;
  for (int idx = t; idx < 64 * 64; idx += 256) {
    const int cc = idx >> 6, pp = idx & 63;
    tile[cc][pp] = p0 + pp < HW ? src[((size_t)n * C + c0 + cc) * HW + p0 + pp] : 0.f;
  }
  __syncthreads();
  if (bpart != nullptr && t < 64) {       // (pixels past the image are zeros in the tile)
    float s = 0.f;
#pragma unroll 8
    for (int pp = 0; pp < 64; ++pp) s += tile[t][pp];
    bpart[((size_t)n * npb + pb) * C + c0 + t] = s;
  }
  for (int idx = t; idx < 64 * 8; idx += 256) {
    const int pp = idx >> 3, q = idx & 7;
    if (p0 + pp >= HW) continue;
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = tile[8 * q + k][pp];
    const size_t o = ((size_t)n * HW + p0 + pp) * C + c0 + 8 * q;
    const float4 a0 = make_float4(v[0], v[1], v[2], v[3]), a1 = make_float4(v[4], v[5], v[6], v[7]);
    if (dst) {
      *reinterpret_cast<float4*>(dst + o) = a0;
      *reinterpret_cast<float4*>(dst + o + 4) = a1;
    }
    if (dst3) {
      u32x4 hh, mm, ll;
      split8(a0, a1, hh, mm, ll);
      *reinterpret_cast<u32x4*>(dst3 + o) = hh;
      *reinterpret_cast<u32x4*>(dst3 + o + plane) = mm;
      *reinterpret_cast<u32x4*>(dst3 + o + 2 * plane) = ll;
    }
  }
}

// part[b][c] = sum of src[row][c] over the rows b * rows_per_blk .. + rows_per_blk - 1 of an fp32 NHWC tensor [rows][C]: the partial
// sums of the bias gradient of a convolution whose output gradient a GroupNorm backward wrote (k_stem_reduce kind 3 adds them up).
// thread = (channel t % 64 of the workgroup's 64, every fourth row); the four row classes meet in LDS in a fixed order.
__global__ __launch_bounds__(256) void k_stem_colsum(const float* __restrict__ src, float* __restrict__ part, int rows, int C, int rows_per_blk) {
  __shared__ float red[4][64];
  const int t = threadIdx.x, cl = t & 63, sub = t >> 6;
  const int nct = C >> 6;
  const int blk = blockIdx.x / nct, c = (blockIdx.x - blk * nct) * 64 + cl;
  const int r0 = blk * rows_per_blk, r1 = min(r0 + rows_per_blk, rows);
  float s0 = 0.f, s1 = 0.f;
  int r = r0 + sub;
  for (; r + 4 < r1; r += 8) {
    s0 += src[(size_t)r * C + c];
    s1 += src[(size_t)(r + 4) * C + c];
  }
  if (r < r1) s0 += src[(size_t)r * C + c];
  red[sub][cl] = s0 + s1;
  __syncthreads();
  if (sub == 0) part[(size_t)blk * C + c] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

// fp32 -> triples, element for element (n % 8 == 0)
__global__ __launch_bounds__(256) void k_stem_split(const float* __restrict__ src, bf16_t* __restrict__ dst3, size_t plane, size_t n8) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const float4 a0 = reinterpret_cast<const float4*>(src)[2 * i], a1 = reinterpret_cast<const float4*>(src)[2 * i + 1];
  u32x4 hh, mm, ll;
  split8(a0, a1, hh, mm, ll);
  *reinterpret_cast<u32x4*>(dst3 + 8 * i) = hh;
  *reinterpret_cast<u32x4*>(dst3 + 8 * i + plane) = mm;
  *reinterpret_cast<u32x4*>(dst3 + 8 * i + 2 * plane) = ll;
}

__global__ __launch_bounds__(256) void k_stem_to_nchw(const float* __restrict__ src, float* __restrict__ dst, int C, int HW) {
  __shared__ float tile[64][65];
  const int t = threadIdx.x;
  const int npb = (HW + 63) / 64, ncb = C / 64;
  const int n = blockIdx.x / (npb * ncb), rem = blockIdx.x - n * npb * ncb, cb = rem / npb, pb = rem - cb * npb;
  const int c0 = cb * 64, p0 = pb * 64;
  for (int idx = t; idx < 64 * 64; idx += 256) {
    const int pp = idx >> 6, cc = idx & 63;
    tile[cc][pp] = p0 + pp < HW ? src[((size_t)n * HW + p0 + pp) * C + c0 + cc] : 0.f;
  }
  __syncthreads();
  for (int idx = t; idx < 64 * 64; idx += 256) {
    const int cc = idx >> 6, pp = idx & 63;
    if (p0 + pp < HW) dst[((size_t)n * C + c0 + cc) * HW + p0 + pp] = tile[cc][pp];
  }
}

// ============================================================================
// preparation (once per forward): filters -> triples in both operand layouts, conv0's filter transposed, zero rows
// ============================================================================
__global__ __launch_bounds__(256) void k_stem_prep(const SPrepArgs a) {
  // a flat grid, every job its own run of workgroups (as [largest job] x [jobs] 18 k of the 19 k workgroups at cfg 2 came to leave at once)
  int seg = 0;                       // 0..5: the filter jobs (those past njobs are empty), 6: conv0's filter, 7: the zero rows
  while (seg < 7 && blockIdx.x >= a.blk0[seg + 1]) ++seg;
  const size_t idx = (size_t)(blockIdx.x - a.blk0[seg]) * 256 + threadIdx.x;
  const int job = seg < 6 ? seg : a.njobs + (seg - 6);
  if (job < a.njobs) {
    const SPrepJob& j = a.job[job];
    const size_t total = (size_t)j.taps * j.Cout * j.Cin;
    if (idx >= total) return;
    const int ci = (int)(idx % j.Cin);
    const size_t r = idx / j.Cin;
    const int co = (int)(r % j.Cout), tap = (int)(r / j.Cout);
    const float v = j.w[((size_t)co * j.Cin + ci) * j.taps + tap];
    bf16_t h, m, l;
    split3(v, h, m, l);
    const size_t of = ((size_t)tap * j.Cout + co) * j.Cin + ci, od = ((size_t)tap * j.Cin + ci) * j.Cout + co;
    j.wf[of] = h; j.wf[of + total] = m; j.wf[of + 2 * total] = l;
    j.wd[od] = h; j.wd[od + total] = m; j.wd[od + 2 * total] = l;
    return;
  }
  if (job == a.njobs) {        // conv0: [64][k0] -> [28][64], zero rows behind k0
    if (a.w0t == nullptr || idx >= 28 * 64) return;
    const int k = (int)(idx / 64), co = (int)(idx % 64);
    a.w0t[idx] = k < a.k0 ? a.w0[co * a.k0 + k] : 0.f;
    return;
  }
  // zero rows of the triples tensors
  const int which = (int)(idx / 4096), e = (int)(idx % 4096);
  if (which >= a.nzero * 3) return;
  const int ten = which / 3, p = which - 3 * ten;
  if (e < a.zero_c[ten]) a.zero[ten][p * a.zero_plane[ten] + e] = 0;
}

// ============================================================================
// slab / partial sums into the caller's gradient tensors.  kind 0: one workgroup per (output channel co, tap): thread =
// (ci % 64, quarter of the splits); the slabs are read in their own order (runs of 64 floats), the four quarters meet in
// LDS, and the sums go to PyTorch's [co][ci][tap] order.  (A first version gave every thread ALL splits of nine taps: chains
// of 500+ dependent loads, 120 us for 50 MB.)
// ============================================================================
__global__ __launch_bounds__(256) void k_stem_reduce(const SReduceArgs a) {
  __shared__ float part[4][64];
  // a flat grid, every job its own run of workgroups (as [largest job] x [jobs] two thirds of the 16 k workgroups at cfg 2 came to leave at once)
  int ji = 0;
  while (ji + 1 < a.njobs && blockIdx.x >= a.blk0[ji + 1]) ++ji;
  const SReduceJob& j = a.job[ji];
  const unsigned bx = blockIdx.x - a.blk0[ji];
  const int t = threadIdx.x;
  if (j.kind == 0) {
    const int co = bx / j.taps, tap = bx - co * j.taps;
    if (co >= j.Co) return;
    const size_t total = (size_t)j.taps * j.Co * j.Ci;
    const int cl = t & 63, sub = t >> 6;
    for (int c0 = 0; c0 < j.Ci; c0 += 64) {
      const float* src = j.slab + ((size_t)tap * j.Co + co) * j.Ci + c0 + cl;
      float s0 = 0.f, s1 = 0.f;
      int k = sub;
      // (eight slabs in flight per thread instead of two; the additions keep their order, so the sums are the same bits)
      for (; k + 28 < j.ns; k += 32) {
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = src[(size_t)(k + 4 * q) * total];
#pragma unroll
        for (int q = 0; q < 8; q += 2) { s0 += v[q]; s1 += v[q + 1]; }
      }
      for (; k + 4 < j.ns; k += 8) {
        s0 += src[(size_t)k * total];
        s1 += src[(size_t)(k + 4) * total];
      }
      if (k < j.ns) s0 += src[(size_t)k * total];
      part[sub][cl] = s0 + s1;
      __syncthreads();
      if (sub == 0) j.out[((size_t)co * j.Ci + c0 + cl) * j.taps + tap] = (part[0][cl] + part[1][cl]) + (part[2][cl] + part[3][cl]);
      __syncthreads();
    }
  } else {
    // kinds 1 (conv0: 64 x 32 words per slab, 450 slabs at cfg 2), 2 (per-sample partials, 2 Co words) and 3 (bias partials, Co words): a workgroup sums 32 outputs, its
    // eight 32-lane groups every eighth slab with eight loads in flight, the groups meet in LDS in a fixed order.  (One thread per output
    // and all slabs, four in flight: 113 dependent rounds at cfg 2 -- the 48 us this launch took.)
    const size_t nout = j.kind == 1 ? (size_t)64 * 32 : j.kind == 2 ? (size_t)2 * j.Co : (size_t)j.Co;
    const int o = t & 31, g = t >> 5;
    const size_t idx = (size_t)bx * 32 + o;
    if ((size_t)bx * 32 >= nout) return;
    const bool on = idx < nout;
    const float* src = j.slab + (on ? idx : 0);
    float acc = 0.f;
    int k = g;
    for (; k + 56 < j.ns; k += 64) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = src[(size_t)(k + 8 * q) * nout];
      acc += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    for (; k < j.ns; k += 8) acc += src[(size_t)k * nout];
    part[g >> 1][(g & 1) * 32 + o] = acc;
    __syncthreads();
    if (g != 0 || !on) return;
    const float sum = ((part[0][o] + part[0][32 + o]) + (part[1][o] + part[1][32 + o])) + ((part[2][o] + part[2][32 + o]) + (part[3][o] + part[3][32 + o]));
    if (j.kind == 1) {
      const int co = (int)(idx >> 5), kk = (int)(idx & 31);
      if (kk < j.Ci) j.out[co * j.Ci + kk] = sum;
      else if (kk == j.Ci) j.out2[co] = sum;
    } else {
      if (idx < (size_t)j.Co) j.out[idx] = sum;
      else j.out2[idx - j.Co] = sum;
    }
  }
}

}  // namespace

// ============================================================================
// launchers
// ============================================================================
// NODE_TUNE_STEM_RING=0 (read per call): the one-step, double-buffered schedule of both matrix kernels (A/B runs, tests);
// the results are the same bits at every depth -- the products enter each accumulator in one order
static bool stem_ring() { return env_int("NODE_TUNE_STEM_RING", 1) != 0; }

void launch_stem_conv(const SConvArgs& a, hipStream_t s) {
  const int mt = a.cls_tile0[a.nclass];
  const int ntn = (a.Cout / 64) * ((a.mode == 0 && a.w2 != nullptr) ? 2 : 1);
#define STEM_CONV(KC, D, SEG)                                                             \
  {                                                                                       \
    static bool attr[MAX_DEVICES] = {};                                                   \
    allow_full_lds(reinterpret_cast<const void*>(k_stem_conv<KC, D, SEG>), attr);         \
    const size_t lds = (size_t)(D + 1) * (3 * 128 + 3 * 64) * 2 * KC + 512;               \
    hipLaunchKernelGGL((k_stem_conv<KC, D, SEG>), dim3(mt * ntn), dim3(256), lds, s, a);   \
  }
  // reductions of more than two segments' length (3x3 on 512 channels and more, 4x4 on 512 and more) are summed in segments; every
  // shorter one -- 3x3 on up to 256 channels: K <= 2304 -- runs the kernel without a total, the bits it always had
  const bool seg = (size_t)a.KH * a.KW * a.Cin > 2 * STEM_SEG_K;
  if (stem_ring()) {
    if (seg) STEM_CONV(32, STEM_RING_D, true)
    else STEM_CONV(32, STEM_RING_D, false)
  } else {
    if (seg) STEM_CONV(64, 1, true)
    else STEM_CONV(64, 1, false)
  }
#undef STEM_CONV
}

void launch_stem_wgrad(const SWgradArgs& a, hipStream_t s) {
  const int taps = a.KH * a.KW;
  const int krows = stem_wgrad_rows(taps);
  const int grid = (a.Cin / 64) * (a.Cout / 64) * krows * a.nsplit;
  const int nimg = 1 + krows + (a.dy23 ? 1 : 0);
#define STEM_WG(T, EX, D)                                                                \
  {                                                                                       \
    static bool attr[MAX_DEVICES] = {};                                                   \
    allow_full_lds(reinterpret_cast<const void*>(k_stem_wgrad<T, EX, D>), attr);          \
    const size_t lds = (size_t)(D + 1) * nimg * 3 * 16 * 128;                             \
    hipLaunchKernelGGL((k_stem_wgrad<T, EX, D>), dim3(grid), dim3(256), lds, s, a);        \
  }
  if (stem_ring()) {
    if (taps == 9 && a.dy23) STEM_WG(3, true, STEM_RING_D)
    else if (taps == 9) STEM_WG(3, false, STEM_RING_D)
    else if (taps == 16) STEM_WG(4, false, STEM_RING_D)
    else STEM_WG(1, false, STEM_RING_D)
  } else {
    if (taps == 9 && a.dy23) STEM_WG(3, true, 1)
    else if (taps == 9) STEM_WG(3, false, 1)
    else if (taps == 16) STEM_WG(4, false, 1)
    else STEM_WG(1, false, 1)
  }
#undef STEM_WG
}

void launch_stem_conv0_fwd(const float* x, const float* w0t, const float* bias, float* h0, int N, int Cin, int H, int W, hipStream_t s) {
  const int rows = N * (H - 2) * (W - 2);
  hipLaunchKernelGGL(k_stem_conv0_fwd, dim3((rows + 127) / 128), dim3(256), 0, s, x, w0t, bias, h0, N, Cin, H, W);
}
void launch_stem_conv0_wgrad(const float* x, const float* dh0, float* slab, int N, int Cin, int H, int W, int nsplit, int rows_per_split,
                             hipStream_t s) {
  hipLaunchKernelGGL(k_stem_conv0_wgrad, dim3(nsplit), dim3(256), 0, s, x, dh0, slab, N, Cin, H, W, rows_per_split);
}
void launch_stem_conv0_dgrad(const float* dh0, const float* w0, float* dx, int N, int Cin, int H, int W, hipStream_t s) {
  const int tx = (W + DG_TW - 1) / DG_TW, ty = (H + DG_TH - 1) / DG_TH;
  hipLaunchKernelGGL(k_stem_conv0_dgrad, dim3((unsigned)(N * tx * ty)), dim3(256), 0, s, dh0, w0, dx, Cin, H, W, tx, ty);
}

// channels per workgroup of the GroupNorm passes: a power of two in [max(8, cpg), 128] whose [HW][CB] block fits the LDS
// twice (the backward holds xhat and dy); 0 if even the smallest does not
int stem_gn_cb(int HW, int C, int cpg) {
  const size_t budget = 150 * 1024;
  int cb = 8;
  while (cb < cpg) cb *= 2;
  if (cb > C || cb > 128 || (size_t)HW * cb * 2 * sizeof(float) > budget) return 0;
  while (cb * 2 <= C && cb * 2 <= 128 && (size_t)HW * cb * 4 * sizeof(float) <= budget) cb *= 2;
  static const int cap = env_int("NODE_TUNE_STEM_GNCB", -1);      // upper limit of the channel block (A/B measurements)
  while (cap > 0 && cb > cap && cb / 2 >= cpg && cb / 2 >= 8) cb /= 2;
  // the kernels index channels with `t & (CB - 1)`, run C / CB blocks per sample and CB / cpg whole groups per block:
  // a block that does not divide C leaves channels unwritten, a group that straddles blocks gets wrong statistics
  // (filters = 192, 384, ...: cpg = 6, 12).  Such shapes are refused (check_stem_shape) and run the module sequence.
  if (C % cb != 0 || cb % cpg != 0) return 0;
  return cb;
}
// NODE_TUNE_STEM_GN=0 (read per call): the GroupNorm passes as k_stem_gn_fwd / k_stem_gn_bwd (A/B runs, tests).  Default:
// k_stem_gn_*_fl -- same block, same grid, same LDS, the same bits.
static bool stem_gn_fl() { return env_int("NODE_TUNE_STEM_GN", 1) != 0; }
void launch_stem_gn_fwd(const SGnArgs& a, hipStream_t s) {
  if (stem_gn_fl()) {
    static bool attr[MAX_DEVICES] = {};
    allow_full_lds(reinterpret_cast<const void*>(k_stem_gn_fwd_fl), attr);
    hipLaunchKernelGGL(k_stem_gn_fwd_fl, dim3(a.N * (a.C / a.CB)), dim3(256), ((size_t)a.HW * a.CB + 512) * sizeof(float), s, a);
    return;
  }
  static bool attr[MAX_DEVICES] = {};
  allow_full_lds(reinterpret_cast<const void*>(k_stem_gn_fwd), attr);
  hipLaunchKernelGGL(k_stem_gn_fwd, dim3(a.N * (a.C / a.CB)), dim3(256), ((size_t)a.HW * a.CB + 512) * sizeof(float), s, a);
}
void launch_stem_gn_bwd(const SGnArgs& a, hipStream_t s) {
  const dim3 grid(a.N * (a.C / a.CB));
  const size_t lds = ((size_t)2 * a.HW * a.CB + 1024) * sizeof(float);
  if (stem_gn_fl()) {
    if (a.skip) {
      static bool attr[MAX_DEVICES] = {};
      allow_full_lds(reinterpret_cast<const void*>(k_stem_gn_bwd_fl<true>), attr);
      hipLaunchKernelGGL(k_stem_gn_bwd_fl<true>, grid, dim3(256), lds, s, a);
    } else {
      static bool attr[MAX_DEVICES] = {};
      allow_full_lds(reinterpret_cast<const void*>(k_stem_gn_bwd_fl<false>), attr);
      hipLaunchKernelGGL(k_stem_gn_bwd_fl<false>, grid, dim3(256), lds, s, a);
    }
    return;
  }
  if (a.skip) {
    static bool attr[MAX_DEVICES] = {};
    allow_full_lds(reinterpret_cast<const void*>(k_stem_gn_bwd<true>), attr);
    hipLaunchKernelGGL(k_stem_gn_bwd<true>, grid, dim3(256), lds, s, a);
  } else {
    static bool attr[MAX_DEVICES] = {};
    allow_full_lds(reinterpret_cast<const void*>(k_stem_gn_bwd<false>), attr);
    hipLaunchKernelGGL(k_stem_gn_bwd<false>, grid, dim3(256), lds, s, a);
  }
}

void launch_stem_prep(const SPrepArgs& a0, hipStream_t s) {
  SPrepArgs a = a0;
  unsigned at = 0;
  for (int i = 0; i < 6; ++i) {
    a.blk0[i] = at;
    if (i < a.njobs) at += (unsigned)(((size_t)a.job[i].taps * a.job[i].Cout * a.job[i].Cin + 255) / 256);
  }
  a.blk0[6] = at; at += (28 * 64 + 255) / 256;                              // conv0's filter
  a.blk0[7] = at; at += (unsigned)(((size_t)a.nzero * 3 * 4096 + 255) / 256);    // zero rows
  a.blk0[8] = at;
  hipLaunchKernelGGL(k_stem_prep, dim3(at), dim3(256), 0, s, a);
}
void launch_stem_from_nchw(const float* src, float* dst_nhwc, bf16_t* dst3, size_t plane, int N, int C, int HW, hipStream_t s, float* bpart) {
  hipLaunchKernelGGL(k_stem_from_nchw, dim3(N * (C / 64) * ((HW + 63) / 64)), dim3(256), 0, s, src, dst_nhwc, dst3, plane, C, HW, bpart);
}
void launch_stem_colsum(const float* src, float* part, int rows, int C, int rows_per_blk, hipStream_t s) {
  const int nblk = (rows + rows_per_blk - 1) / rows_per_blk;
  hipLaunchKernelGGL(k_stem_colsum, dim3(nblk * (C / 64)), dim3(256), 0, s, src, part, rows, C, rows_per_blk);
}
void launch_stem_split(const float* src, bf16_t* dst3, size_t plane, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_stem_split, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, s, src, dst3, plane, n / 8);
}
void launch_stem_to_nchw(const float* src_nhwc, float* dst, int N, int C, int HW, hipStream_t s) {
  hipLaunchKernelGGL(k_stem_to_nchw, dim3(N * (C / 64) * ((HW + 63) / 64)), dim3(256), 0, s, src_nhwc, dst, C, HW);
}
void launch_stem_reduce(const SReduceArgs& a0, hipStream_t s) {
  SReduceArgs a = a0;
  unsigned at = 0;
  for (int i = 0; i < a.njobs; ++i) {
    const SReduceJob& j = a.job[i];
    a.blk0[i] = at;
    at += (unsigned)(j.kind == 0 ? j.Co * j.taps : j.kind == 1 ? 64 : j.kind == 2 ? (2 * j.Co + 31) / 32 : (j.Co + 31) / 32);
  }
  a.blk0[a.njobs] = at;
  if (at == 0) return;
  hipLaunchKernelGGL(k_stem_reduce, dim3(at), dim3(256), 0, s, a);
}

}  // namespace node
