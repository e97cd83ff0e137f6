// Input pipeline of the training loop (the reference's transform chains, utils.py:81-196) as ONE launch per batch:
//
//   out[b]        = Normalize(ToTensor(Flip(Jitter(Crop(Pad(data[index[b]]))))))      fp32  [B, C, H, W]
//   out_labels[b] = labels[index[b]]                                                  int64 [B]
//
// `data` is the whole split as uint8 [N, C, H, W] in device memory; every stage is switched by a flag bit, so the same kernel
// serves the test transform (no flag: gather, / 255; the norm bit: + Normalize).
//
//   Crop    RandomCrop(size, padding = P), zero fill: output pixel (i, j) reads source pixel (i + dy - P, j + dx - P), dy and dx
//           uniform on {0 .. 2 P}, or 0 outside the image.
//   Jitter  ColorJitter(saturation = s, hue = h) with torchvision's TENSOR formulas in fp32 on [0, 1] (adjust_saturation's blend
//           with the grey image, adjust_hue's _rgb2hsv / _hsv2rgb), no 8-bit requantisation between the two; the order bit is
//           torchvision's randperm restricted to the two active transforms.  Black stays black under both, so the padding
//           needs no jitter and Crop and Jitter commute.
//   Flip    RandomHorizontalFlip: output column j reads column W - 1 - j of the cropped image.
//
// Random numbers: Philox4x32-10, key = the 64-bit seed (lo, hi), counter = (dataset index, epoch, call, 0).  What an image
// looks like therefore depends on (seed, epoch, dataset index) alone -- not on the batch, the position in it or the rank.
//   call 0: dy = (w0 (2P+1)) >> 32, dx = (w1 (2P+1)) >> 32, flip = w2 >> 31, hue first = w3 >> 31
//   call 1: u(w) = (w >> 8) 2^-24; fs = (1 - s) + 2 s u(w0); fh = -h + 2 h u(w1)
// The draws depend on blockIdx alone, so the compiler keeps them on the scalar unit: one Philox per wave, not per lane.
//
// Shape: grid (B, ceil(H W / 256)); a thread owns ONE pixel in all C channels (jitter couples them); consecutive lanes own
// consecutive output pixels, so each channel's store is a contiguous 256 B per wave; the uint8 reads of a wave touch at most
// two source rows per channel.  No LDS, no workspace.  An index outside [0, N) never reads the split: it yields a black image
// (normalised like any other) and the label -1.
#include "node_internal.h"

namespace node {

namespace {

struct Philox4 { uint32_t w0, w1, w2, w3; };

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return {c0, c1, c2, c3};
}

__device__ __forceinline__ float unit24(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// torchvision adjust_saturation: _blend(img, rgb_to_grayscale(img), fs)
__device__ __forceinline__ void jitter_saturation(float& r, float& g, float& b, float fs) {
  const float gray = 0.2989f * r + 0.587f * g + 0.114f * b;
  r = clamp01(fs * r + (1.f - fs) * gray);
  g = clamp01(fs * g + (1.f - fs) * gray);
  b = clamp01(fs * b + (1.f - fs) * gray);
}

// torchvision adjust_hue: _rgb2hsv, h <- (h + fh) mod 1, _hsv2rgb
__device__ __forceinline__ void jitter_hue(float& r, float& g, float& b, float fh) {
  const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
  const bool eq = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eq ? 1.f : maxc);
  const float crd = eq ? 1.f : cr;
  const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
  const bool is_r = maxc == r, is_g = maxc == g;
  const float hr = is_r ? bc - gc : 0.f;
  const float hg = (is_g && !is_r) ? 2.f + rc - bc : 0.f;
  const float hb = (!is_g && !is_r) ? 4.f + gc - rc : 0.f;
  float h = fmodf((hr + hg + hb) / 6.f + 1.f, 1.f);
  h += fh;
  h -= floorf(h);
  const float v = maxc;
  const float h6 = h * 6.f, fl = floorf(h6), f = h6 - fl;
  const int sector = (int)fl % 6;
  const float p = clamp01(v * (1.f - s));
  const float q = clamp01(v * (1.f - s * f));
  const float t = clamp01(v * (1.f - s * (1.f - f)));
  switch (sector) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

template <int C>
__global__ __launch_bounds__(AUG_THREADS) void k_augment(const uint8_t* __restrict__ data, const int64_t* __restrict__ labels,
                                                         const int64_t* __restrict__ index, float* __restrict__ out,
                                                         int64_t* __restrict__ out_labels, AugmentArgs a) {
  const int b = blockIdx.x;
  const int hw = a.h * a.w;
  const int pix = blockIdx.y * AUG_THREADS + threadIdx.x;
  const int64_t item = index[b];
  const bool known = item >= 0 && item < a.n;
  if (pix == 0) out_labels[b] = known ? labels[item] : -1;
  if (pix >= hw) return;
  const int i = pix / a.w, j = pix - i * a.w;

  // the draws of this image
  int dy = 0, dx = 0;
  bool flip = false, hue_first = false;
  if (a.flags & (AUG_CROP | AUG_FLIP | AUG_JITTER)) {
    const Philox4 d = philox4x32_10((uint32_t)item, a.epoch, 0u, 0u, a.seed_lo, a.seed_hi);
    if (a.flags & AUG_CROP) {
      const uint32_t span = 2u * (uint32_t)a.pad + 1u;
      dy = (int)__umulhi(d.w0, span) - a.pad;
      dx = (int)__umulhi(d.w1, span) - a.pad;
    }
    flip = (a.flags & AUG_FLIP) && (d.w2 >> 31);
    hue_first = d.w3 >> 31;
  }
  const int si = i + dy, sj = (flip ? a.w - 1 - j : j) + dx;
  const bool inside = known && si >= 0 && si < a.h && sj >= 0 && sj < a.w;

  float x[C];
#pragma unroll
  for (int c = 0; c < C; ++c) x[c] = 0.f;
  if (inside) {
    const uint8_t* src = data + ((size_t)item * C * a.h + si) * a.w + sj;
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = (float)src[(size_t)c * hw] / 255.f;
    if constexpr (C == 3) {
      if (a.flags & AUG_JITTER) {
        const Philox4 u = philox4x32_10((uint32_t)item, a.epoch, 1u, 0u, a.seed_lo, a.seed_hi);
        const float fs = (1.f - a.saturation) + 2.f * a.saturation * unit24(u.w0);
        const float fh = -a.hue + 2.f * a.hue * unit24(u.w1);
        if (hue_first) {
          jitter_hue(x[0], x[1], x[2], fh);
          jitter_saturation(x[0], x[1], x[2], fs);
        } else {
          jitter_saturation(x[0], x[1], x[2], fs);
          jitter_hue(x[0], x[1], x[2], fh);
        }
      }
    }
  }
  float* dst = out + (size_t)b * C * hw + pix;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float y = (a.flags & AUG_NORM) ? (x[c] - a.mean[c]) / a.std[c] : x[c];
    dst[(size_t)c * hw] = y;
  }
}

}  // namespace

void launch_augment(const AugmentArgs& a, int c, const uint8_t* data, const int64_t* labels, const int64_t* index, int batch,
                    float* out, int64_t* out_labels, hipStream_t s) {
  const dim3 grid((unsigned)batch, (unsigned)((a.h * a.w + AUG_THREADS - 1) / AUG_THREADS));
  if (c == 3)
    hipLaunchKernelGGL(k_augment<3>, grid, dim3(AUG_THREADS), 0, s, data, labels, index, out, out_labels, a);
  else
    hipLaunchKernelGGL(k_augment<1>, grid, dim3(AUG_THREADS), 0, s, data, labels, index, out, out_labels, a);
}

}  // namespace node
