// C ABI of the input pipeline (include/node_hip.h: node_augment_batch): argument checks and the launch of kernels_augment.hip.
// Reference: utils.py:81-196.  Every refusal happens before the first HIP call.
#include "host_common.h"

using namespace node;

static_assert(NODE_AUG_CROP == AUG_CROP && NODE_AUG_JITTER == AUG_JITTER && NODE_AUG_FLIP == AUG_FLIP && NODE_AUG_NORM == AUG_NORM,
              "the stage bits of the header and of the kernel");

extern "C" {

int node_augment_batch(const node_augment* aug, const uint8_t* data, const int64_t* labels, const int64_t* index, int batch,
                       uint64_t seed, uint32_t epoch, float* out, int64_t* out_labels, void* stream) {
  if (!aug || !data || !labels || !index || !out || !out_labels) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if (aug->n < 1 || aug->h < 1 || aug->w < 1 || batch < 1)
    return fail(NODE_ERR_SHAPE, "augment shape n=%d h=%d w=%d batch=%d: every size must be >= 1", aug->n, aug->h, aug->w, batch);
  if (aug->c != 1 && aug->c != 3) return fail(NODE_ERR_UNSUPPORTED, "augment c=%d: images have 1 or 3 channels", aug->c);
  if ((int64_t)aug->h * aug->w > (int64_t)65535 * AUG_THREADS)
    return fail(NODE_ERR_UNSUPPORTED, "augment image of %d x %d pixels: at most %d pixels are supported", aug->h, aug->w,
                65535 * AUG_THREADS);
  const uint32_t known = NODE_AUG_CROP | NODE_AUG_JITTER | NODE_AUG_FLIP | NODE_AUG_NORM;
  if (aug->flags & ~known) return fail(NODE_ERR_ARG, "augment flags=0x%x: unknown stage bits", aug->flags);
  if ((aug->flags & NODE_AUG_JITTER) && aug->c != 3)
    return fail(NODE_ERR_UNSUPPORTED, "augment jitter with c=%d: colour jitter needs 3 channels", aug->c);
  if (aug->flags & NODE_AUG_CROP) {
    if (aug->padding < 0 || 2 * (int64_t)aug->padding + 1 > 65536)
      return fail(NODE_ERR_ARG, "augment padding=%d: 2 padding + 1 must lie in [1, 65536]", aug->padding);
  }
  if (aug->flags & NODE_AUG_JITTER) {
    if (!(aug->saturation >= 0.f && aug->saturation <= 1.f) || !(aug->hue >= 0.f && aug->hue <= 0.5f))
      return fail(NODE_ERR_ARG, "augment saturation=%g hue=%g: saturation must lie in [0, 1], hue in [0, 0.5]", (double)aug->saturation,
                  (double)aug->hue);
  }
  if (aug->flags & NODE_AUG_NORM) {
    for (int ch = 0; ch < aug->c; ++ch)
      if (!(aug->std[ch] > 0.f) || !(aug->mean[ch] == aug->mean[ch]))
        return fail(NODE_ERR_ARG, "augment mean[%d]=%g std[%d]=%g: std must be > 0", ch, (double)aug->mean[ch], ch, (double)aug->std[ch]);
  }
  AugmentArgs a;
  a.n = aug->n;
  a.h = aug->h;
  a.w = aug->w;
  a.pad = (aug->flags & NODE_AUG_CROP) ? aug->padding : 0;
  a.flags = aug->flags;
  a.epoch = epoch;
  a.seed_lo = (uint32_t)seed;
  a.seed_hi = (uint32_t)(seed >> 32);
  a.saturation = aug->saturation;
  a.hue = aug->hue;
  for (int ch = 0; ch < 3; ++ch) {
    a.mean[ch] = aug->mean[ch];
    a.std[ch] = aug->std[ch];
  }
  launch_augment(a, aug->c, data, labels, index, batch, out, out_labels, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch of k_augment failed: %s", hipGetErrorString(e));
  return NODE_OK;
}

}  // extern "C"
