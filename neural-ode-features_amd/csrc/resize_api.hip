// C ABI of the transfer evaluations' test transform (include/node_hip.h: node_resize_batch, node_resize_table): PIL's
// coefficient tables, built on the host in double, their per-device copies, the argument checks and the launch of
// kernels_resize.hip.  Reference: evaluate.py:38-50.  Every refusal happens before the first HIP call.
#include "host_common.h"

#include <cmath>
#include <map>
#include <tuple>

using namespace node;

namespace {

constexpr int64_t TABLE_MAX = (int64_t)1 << 24;      // coefficients of one axis

struct HostTable {
  int ksize = 0;
  std::vector<int32_t> xmin, count, coeff;           // [out], [out], [out, ksize]
};

// taps of one output position: 2 ceil(support) + 1 (what PIL allocates per row); in, out >= 1
int64_t table_ksize(int in, int out) {
  const double scale = (double)in / (double)out;
  return (int64_t)std::ceil(scale < 1.0 ? 1.0 : scale) * 2 + 1;
}

// PIL's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter on the whole axis.  Every operation is one IEEE
// double operation in the order written: a contracted multiply-add moves a weight by an ulp, and an ulp flips a coefficient.
HostTable build_table(int in, int out) {
#pragma clang fp contract(off)
  HostTable t;
  const double scale = (double)in / (double)out;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = filterscale;
  t.ksize = (int)table_ksize(in, out);
  t.xmin.resize(out);
  t.count.resize(out);
  t.coeff.assign((size_t)out * t.ksize, 0);
  std::vector<double> w(t.ksize);
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    const int taps = xmax - xmin;
    double sum = 0.0;
    for (int x = 0; x < taps; ++x) {
      double d = (x + xmin - center + 0.5) / filterscale;
      if (d < 0.0) d = -d;
      w[x] = d < 1.0 ? 1.0 - d : 0.0;
      sum += w[x];
    }
    int32_t* k = t.coeff.data() + (size_t)xx * t.ksize;
    for (int x = 0; x < taps; ++x) {
      const double v = sum != 0.0 ? w[x] / sum : w[x];
      k[x] = (int32_t)(v * (double)(1 << RESIZE_BITS) + 0.5);
    }
    t.xmin[xx] = xmin;
    t.count[xx] = taps;
  }
  return t;
}

std::mutex g_mu;
std::map<std::pair<int, int>, HostTable> g_host;                     // (in, out)
std::map<std::tuple<int, int, int>, ResizeAxis> g_device;            // (device, in, out); lives as long as the process

const HostTable& host_table(int in, int out) {                       // g_mu held
  auto it = g_host.find({in, out});
  if (it == g_host.end()) it = g_host.emplace(std::make_pair(in, out), build_table(in, out)).first;
  return it->second;
}

// the axis's table on the current device; in == out: the pass is skipped, no table
int device_table(int in, int out, ResizeAxis* axis) {
  *axis = ResizeAxis{nullptr, nullptr, nullptr, 0};
  if (in == out) return NODE_OK;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_device.find({dev, in, out});
  if (it == g_device.end()) {
    const HostTable& t = host_table(in, out);
    const size_t head = 2 * (size_t)out, all = head + t.coeff.size();
    std::vector<int32_t> flat(all);
    std::copy(t.xmin.begin(), t.xmin.end(), flat.begin());
    std::copy(t.count.begin(), t.count.end(), flat.begin() + out);
    std::copy(t.coeff.begin(), t.coeff.end(), flat.begin() + head);
    int32_t* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, all * sizeof(int32_t)));
    hipError_t e = hipMemcpy(d, flat.data(), all * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return fail(NODE_ERR_HIP, "copy of the %d -> %d resize table failed: %s", in, out, hipGetErrorString(e));
    }
    it = g_device.emplace(std::make_tuple(dev, in, out), ResizeAxis{d, d + out, d + head, t.ksize}).first;
  }
  *axis = it->second;
  return NODE_OK;
}

int check_axis(const char* name, int in, int out) {
  if (table_ksize(in, out) * out > TABLE_MAX)
    return fail(NODE_ERR_UNSUPPORTED, "resize %s %d -> %d: %lld coefficients, at most %lld are supported", name, in, out,
                (long long)(table_ksize(in, out) * out), (long long)TABLE_MAX);
  return NODE_OK;
}

}  // namespace

extern "C" {

int node_resize_table(int in, int out, int32_t* xmin, int32_t* count, int32_t* coeff, int capacity) {
  if (in < 1 || out < 1) return fail(NODE_ERR_SHAPE, "resize table in=%d out=%d: every size must be >= 1", in, out);
  TRY(check_axis("axis", in, out));
  const int need = (int)(table_ksize(in, out) * out);
  if (capacity < need) return need;
  if (!xmin || !count || !coeff) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  std::lock_guard<std::mutex> lk(g_mu);
  const HostTable& t = host_table(in, out);
  std::copy(t.xmin.begin(), t.xmin.end(), xmin);
  std::copy(t.count.begin(), t.count.end(), count);
  std::copy(t.coeff.begin(), t.coeff.end(), coeff);
  return need;
}

int node_resize_batch(const node_resize* rs, const uint8_t* data, const int64_t* labels, const int64_t* index, int batch,
                      float* out_f32, uint8_t* out_u8, int64_t* out_labels, void* stream) {
  if (!rs || !data || !labels || !index || !out_labels) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if (!out_f32 && !out_u8) return fail(NODE_ERR_NULL, "out_f32 and out_u8 are both NULL: one of the two outputs is required");
  if (rs->n < 1 || rs->h < 1 || rs->w < 1 || rs->out_h < 1 || rs->out_w < 1 || batch < 1)
    return fail(NODE_ERR_SHAPE, "resize shape n=%d h=%d w=%d out_h=%d out_w=%d batch=%d: every size must be >= 1", rs->n, rs->h,
                rs->w, rs->out_h, rs->out_w, batch);
  if (rs->c != 1 && rs->c != 3) return fail(NODE_ERR_UNSUPPORTED, "resize c=%d: images have 1 or 3 channels", rs->c);
  if ((int64_t)rs->h * rs->out_w > RESIZE_LDS_BYTES)
    return fail(NODE_ERR_UNSUPPORTED, "resize h=%d out_w=%d: the %lld bytes between the two passes stay on chip, at most %d are supported",
                rs->h, rs->out_w, (long long)((int64_t)rs->h * rs->out_w), RESIZE_LDS_BYTES);
  const int64_t lim = (int64_t)1 << 31;
  // (h out_w <= 2^16 and w, out_h < 2^31: the products below stay far inside int64)
  if ((int64_t)rs->n * rs->c * rs->h >= lim || (int64_t)rs->n * rs->c * rs->h * rs->w >= lim ||
      (int64_t)batch * rs->c * rs->out_h >= lim || (int64_t)batch * rs->c * rs->out_h * rs->out_w >= lim)
    return fail(NODE_ERR_UNSUPPORTED, "resize of [%d, %d, %d, %d] to [%d, %d, %d, %d]: tensors of 2^31 elements or more are not supported",
                rs->n, rs->c, rs->h, rs->w, batch, rs->c, rs->out_h, rs->out_w);
  TRY(check_axis("width", rs->w, rs->out_w));
  TRY(check_axis("height", rs->h, rs->out_h));
  if (rs->normalize) {
    for (int ch = 0; ch < rs->c; ++ch)
      if (!(rs->std[ch] > 0.f) || !(rs->mean[ch] == rs->mean[ch]))
        return fail(NODE_ERR_ARG, "resize mean[%d]=%g std[%d]=%g: std must be > 0", ch, (double)rs->mean[ch], ch, (double)rs->std[ch]);
  }
  ResizeArgs a;
  a.n = rs->n;
  a.h = rs->h;
  a.w = rs->w;
  a.oh = rs->out_h;
  a.ow = rs->out_w;
  a.normalize = rs->normalize != 0;
  for (int ch = 0; ch < 3; ++ch) {
    a.mean[ch] = rs->mean[ch];
    a.std[ch] = rs->std[ch];
  }
  TRY(device_table(rs->w, rs->out_w, &a.horiz));
  TRY(device_table(rs->h, rs->out_h, &a.vert));
  launch_resize(a, rs->c, data, labels, index, batch, out_f32, out_u8, out_labels, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch of k_resize failed: %s", hipGetErrorString(e));
  return NODE_OK;
}

}  // extern "C"
