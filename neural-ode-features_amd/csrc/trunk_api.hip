// C ABI of the ResNet baseline's residual trunk (include/node_hip.h: node_trunk_fwd / node_trunk_bwd): `blocks` x
// ResBlock(C, C), stride 1, identity shortcut -- model.py:79 (`features`), model.py:284-310 -- as a host-side plan of the
// stem's kernels (kernels_stem.hip): gather-GEMM convolutions on bf16 triples, GroupNorm + ReLU passes that write the
// triples the next convolution reads, split-K weight gradients.  NHWC inside the workspace, NCHW at the boundary.
//
// forward:   NCHW -> NHWC | filters -> triples (6 per launch) | per block: GN1+ReLU | conv1 | GN2+ReLU | conv2 (+ x in the
//            epilogue) [| NHWC -> NCHW into taps[i]] | NHWC -> NCHW
// backward:  NCHW -> NHWC (fp32 + triples) | per block, last first: wgrad conv2 | dgrad conv2 | GN2 backward (-> triples) |
//            wgrad conv1 | dgrad conv1 | GN1 backward + the shortcut's gradient (fp32 + triples: the next block's dy) |
//            one reduction launch per three blocks (12 jobs: 6 slab sets, 6 GroupNorm partials) | NHWC -> NCHW into d_x
// Nothing is accumulated with atomics: every sum runs in a fixed order.
#include "host_common.h"
#include "stem.h"
#include "stem_plan.h"
#include <cstring>
#include <vector>

using namespace node;

namespace {

constexpr int GROUP = 3;          // blocks per filter-preparation / reduction launch (SPrepArgs: 6 filters, SReduceArgs: 12 jobs)

struct TrunkBlock {               // what one block keeps for its backward (keep = 0: every block uses set 0)
  Trip a1, a2;
  float* h;
  float *stats1, *stats2;
};
struct TrunkPlan {
  int N, C, H, W, B, R;
  float eps;
  bool keep;
  std::vector<Filt> c1, c2;
  std::vector<float*> xs;         // keep: B + 1 block inputs / outputs; otherwise two, used in turn
  std::vector<TrunkBlock> blk;
  // backward
  float* gf[2];
  Trip gt[2], dht;
  float* da;
  std::vector<float*> gp1, gp2;
  Wg w1[GROUP], w2[GROUP];
  size_t bytes;
};

TrunkPlan make_trunk_plan(const node_trunk_shape* sh, bool keep, void* base) {
  TrunkPlan p;
  p.N = sh->n; p.C = sh->channels; p.H = sh->h; p.W = sh->w; p.B = sh->blocks; p.eps = sh->eps; p.keep = keep;
  p.R = p.N * p.H * p.W;
  const int C = p.C, B = p.B, G = C < 32 ? C : 32;
  const size_t RC = (size_t)p.R * C;
  Bump b(base);
  p.c1.resize(B); p.c2.resize(B);
  for (int i = 0; i < B; ++i) {
    p.c1[i] = take_filt(b, C, C, 9);
    p.c2[i] = take_filt(b, C, C, 9);
  }
  p.xs.resize(keep ? B + 1 : 2);
  for (float*& x : p.xs) x = b.take<float>(RC);
  p.blk.resize(keep ? B : 1);
  for (TrunkBlock& k : p.blk) {
    k.a1 = take_trip(b, p.R, C);
    k.h = b.take<float>(RC);
    k.a2 = take_trip(b, p.R, C);
    k.stats1 = b.take<float>((size_t)p.N * G * 2);
    k.stats2 = b.take<float>((size_t)p.N * G * 2);
  }
  if (keep) {
    for (int i = 0; i < 2; ++i) {
      p.gf[i] = b.take<float>(RC);
      p.gt[i] = take_trip(b, p.R, C);
    }
    p.dht = take_trip(b, p.R, C);
    p.da = b.take<float>(RC);
    p.gp1.resize(B); p.gp2.resize(B);
    for (int i = 0; i < B; ++i) {
      p.gp1[i] = b.take<float>((size_t)p.N * 2 * C);
      p.gp2[i] = b.take<float>((size_t)p.N * 2 * C);
    }
    for (int i = 0; i < GROUP && i < B; ++i) {
      p.w1[i] = take_wg(b, p.R, C, C, 9, false);
      p.w2[i] = take_wg(b, p.R, C, C, 9, false);
    }
  }
  p.bytes = b.off + 256;
  return p;
}

int check_trunk_shape(const node_trunk_shape* sh) {
  if (!sh) return fail(NODE_ERR_NULL, "shape is NULL");
  if (sh->n <= 0 || sh->h <= 0 || sh->w <= 0 || sh->channels <= 0) return fail(NODE_ERR_SHAPE, "bad trunk shape");
  if (sh->blocks < 1) return fail(NODE_ERR_UNSUPPORTED, "the trunk takes blocks >= 1 (got %d)", sh->blocks);
  const int C = sh->channels;
  if (C < 64 || (C & (C - 1)) != 0 || C > 4096)
    return fail(NODE_ERR_UNSUPPORTED, "the trunk's kernels take channels a power of two in [64, 4096]: 64-column GEMM tiles, whole "
                 "GroupNorm groups per power-of-two channel block (got %d)", C);
  const size_t elems = (size_t)sh->n * sh->h * sh->w * C;
  if (elems + C >= ((size_t)1 << 31)) return fail(NODE_ERR_UNSUPPORTED, "trunk tensors must stay under 2^31 elements");
  if (stem_gn_cb(sh->h * sh->w, C, C / 32) == 0)
    return fail(NODE_ERR_UNSUPPORTED, "the GroupNorm passes hold a (sample, channel block) in LDS: %d x %d pixels of %d channels "
                 "per group do not fit", sh->h, sh->w, C / 32);
  return NODE_OK;
}

// filters of blocks [i0, i1) -> triples, and the zero rows of `nz` triples tensors
int prep_group(const TrunkPlan& p, const node_trunk_block* blocks, int i0, int i1, const Trip* const* tz, int nz, hipStream_t st) {
  SPrepArgs pa;
  memset(&pa, 0, sizeof(pa));
  int nj = 0;
  for (int i = i0; i < i1; ++i) {
    pa.job[nj++] = {blocks[i].c1_w, p.c1[i].wf, p.c1[i].wd, p.C, p.C, 9};
    pa.job[nj++] = {blocks[i].c2_w, p.c2[i].wf, p.c2[i].wd, p.C, p.C, 9};
  }
  pa.njobs = nj;
  for (int i = 0; i < nz; ++i) {
    pa.zero[i] = tz[i]->p + (size_t)tz[i]->rows * tz[i]->C;
    pa.zero_plane[i] = tz[i]->plane;
    pa.zero_c[i] = tz[i]->C;
  }
  pa.nzero = nz;
  launch_stem_prep(pa, st);
  return launch_ok("stem_prep");
}

int check_blocks(const node_trunk_block* blocks, int B) {
  if (!blocks) return fail(NODE_ERR_NULL, "blocks is NULL");
  for (int i = 0; i < B; ++i) {
    const float* const* pp = reinterpret_cast<const float* const*>(&blocks[i]);
    for (int k = 0; k < 6; ++k)
      if (!pp[k]) return fail(NODE_ERR_NULL, "trunk parameter %d of block %d is NULL", k, i);
  }
  return NODE_OK;
}

}  // namespace

extern "C" {

size_t node_trunk_workspace_bytes(const node_trunk_shape* shape, int keep_for_backward) {
  if (check_trunk_shape(shape) != NODE_OK) return 0;
  return make_trunk_plan(shape, keep_for_backward != 0, nullptr).bytes;
}

int node_trunk_describe(const node_trunk_shape* shape, node_stem_gn_info* out) {
  if (!out) return fail(NODE_ERR_NULL, "out is NULL");
  memset(out, 0, sizeof(*out));
  const int rc = check_trunk_shape(shape);
  if (rc != NODE_OK) return rc;
  *out = gn_info(shape->n, shape->h * shape->w, shape->channels);      // the gn_args of node_trunk_fwd / node_trunk_bwd
  return NODE_OK;
}

int node_trunk_fwd(const node_trunk_shape* shape, const node_trunk_block* blocks, const float* x, float* out, float* taps,
                   int keep_for_backward, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_trunk_shape(shape);
  if (rc != NODE_OK) return rc;
  if (!x || !out || !ws) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if ((rc = check_blocks(blocks, shape->blocks)) != NODE_OK) return rc;
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const TrunkPlan p = make_trunk_plan(shape, keep_for_backward != 0, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "trunk workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int N = p.N, C = p.C, H = p.H, W = p.W, B = p.B, HW = H * W;

  for (int i0 = 0; i0 < B; i0 += GROUP) {
    const int i1 = i0 + GROUP < B ? i0 + GROUP : B;
    const Trip* tz[10];
    int nz = 0;
    if (p.keep) {
      for (int i = i0; i < i1; ++i) { tz[nz++] = &p.blk[i].a1; tz[nz++] = &p.blk[i].a2; }
    } else if (i0 == 0) {
      tz[nz++] = &p.blk[0].a1; tz[nz++] = &p.blk[0].a2;
    }
    if (p.keep && i0 == 0) { tz[nz++] = &p.gt[0]; tz[nz++] = &p.gt[1]; tz[nz++] = &p.dht; }
    if ((rc = prep_group(p, blocks, i0, i1, tz, nz, st)) != NODE_OK) return rc;
  }
  launch_stem_from_nchw(x, p.xs[0], nullptr, 0, N, C, HW, st);
  if ((rc = launch_ok("stem_from_nchw")) != NODE_OK) return rc;
  const float* last = p.xs[0];
  for (int i = 0; i < B; ++i) {
    const TrunkBlock& k = p.blk[p.keep ? i : 0];
    const float* xin = p.keep ? p.xs[i] : p.xs[i & 1];
    float* xout = p.keep ? p.xs[i + 1] : p.xs[(i + 1) & 1];
    {   // a1 = relu(norm1(x))
      SGnArgs g = gn_args(xin, blocks[i].n1_w, blocks[i].n1_b, k.stats1, N, HW, C, p.eps);
      g.a3 = k.a1.p; g.a_plane = k.a1.plane;
      launch_stem_gn_fwd(g, st);
      if ((rc = launch_ok("stem_gn_fwd")) != NODE_OK) return rc;
    }
    launch_stem_conv(conv_fwd_args(k.a1, p.c1[i], k.h, N, H, W, H, W, 3, 1, 1), st);
    if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
    {   // a2 = relu(norm2(h))
      SGnArgs g = gn_args(k.h, blocks[i].n2_w, blocks[i].n2_b, k.stats2, N, HW, C, p.eps);
      g.a3 = k.a2.p; g.a_plane = k.a2.plane;
      launch_stem_gn_fwd(g, st);
      if ((rc = launch_ok("stem_gn_fwd")) != NODE_OK) return rc;
    }
    {   // y = conv2(a2) + x
      SConvArgs c = conv_fwd_args(k.a2, p.c2[i], xout, N, H, W, H, W, 3, 1, 1);
      c.res = xin;
      launch_stem_conv(c, st);
      if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
    }
    if (taps) {
      launch_stem_to_nchw(xout, taps + (size_t)i * p.R * C, N, C, HW, st);
      if ((rc = launch_ok("stem_to_nchw")) != NODE_OK) return rc;
    }
    last = xout;
  }
  launch_stem_to_nchw(last, out, N, C, HW, st);
  return launch_ok("node_trunk_fwd");
}

int node_trunk_bwd(const node_trunk_shape* shape, const node_trunk_block* blocks, const float* grad_out,
                   const node_trunk_block_grads* grads, float* d_x, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_trunk_shape(shape);
  if (rc != NODE_OK) return rc;
  if (!grad_out || !grads || !d_x || !ws) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if ((rc = check_blocks(blocks, shape->blocks)) != NODE_OK) return rc;
  if ((rc = check_blocks(reinterpret_cast<const node_trunk_block*>(grads), shape->blocks)) != NODE_OK) return rc;
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const TrunkPlan p = make_trunk_plan(shape, true, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "trunk workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int N = p.N, C = p.C, H = p.H, W = p.W, B = p.B, HW = H * W;

  // dL/d out: the last block's output gradient, as fp32 (its shortcut) and as triples (its conv2)
  int cur = 0;
  launch_stem_from_nchw(grad_out, p.gf[0], p.gt[0].p, p.gt[0].plane, N, C, HW, st);
  if ((rc = launch_ok("stem_from_nchw")) != NODE_OK) return rc;
  SReduceArgs ra;
  memset(&ra, 0, sizeof(ra));
  int nj = 0, slot = 0;
  for (int i = B - 1; i >= 0; --i) {
    const TrunkBlock& k = p.blk[i];
    const Wg &w1 = p.w1[slot], &w2 = p.w2[slot];
    const Trip& g = p.gt[cur];
    // conv2: weight gradient, data gradient -> da
    launch_stem_wgrad(wgrad_args(g, nullptr, k.a2, w2, N, H, W, H, W, C, C, 3, 1, 1), st);
    if ((rc = launch_ok("stem_wgrad")) != NODE_OK) return rc;
    launch_stem_conv(conv_dgrad_args(g, p.c2[i], p.da, N, H, W, H, W, 3, 1, 1), st);
    if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
    {
      SGnArgs a = gn_args(k.h, blocks[i].n2_w, blocks[i].n2_b, k.stats2, N, HW, C, p.eps);
      a.da = p.da; a.dh = nullptr; a.dh3 = p.dht.p; a.dh_plane = p.dht.plane; a.gpart = p.gp2[i];
      launch_stem_gn_bwd(a, st);
      if ((rc = launch_ok("stem_gn_bwd")) != NODE_OK) return rc;
    }
    // conv1
    launch_stem_wgrad(wgrad_args(p.dht, nullptr, k.a1, w1, N, H, W, H, W, C, C, 3, 1, 1), st);
    if ((rc = launch_ok("stem_wgrad")) != NODE_OK) return rc;
    launch_stem_conv(conv_dgrad_args(p.dht, p.c1[i], p.da, N, H, W, H, W, 3, 1, 1), st);
    if ((rc = launch_ok("stem_conv")) != NODE_OK) return rc;
    {   // dx = GN1'(da) + dy: the gradient of the block's input, which is the output gradient of block i - 1
      SGnArgs a = gn_args(p.xs[i], blocks[i].n1_w, blocks[i].n1_b, k.stats1, N, HW, C, p.eps);
      a.da = p.da; a.skip = p.gf[cur]; a.dh = p.gf[cur ^ 1]; a.gpart = p.gp1[i];
      if (i > 0) { a.dh3 = p.gt[cur ^ 1].p; a.dh_plane = p.gt[cur ^ 1].plane; }
      launch_stem_gn_bwd(a, st);
      if ((rc = launch_ok("stem_gn_bwd")) != NODE_OK) return rc;
      cur ^= 1;
    }
    ra.job[nj++] = {w2.slab, grads[i].c2_w, nullptr, 0, w2.nsplit, C, C, 9};
    ra.job[nj++] = {w1.slab, grads[i].c1_w, nullptr, 0, w1.nsplit, C, C, 9};
    ra.job[nj++] = {p.gp2[i], grads[i].n2_w, grads[i].n2_b, 2, N, C, 0, 0};
    ra.job[nj++] = {p.gp1[i], grads[i].n1_w, grads[i].n1_b, 2, N, C, 0, 0};
    if (++slot == GROUP || i == 0) {     // the slab sets are free again behind this launch
      ra.njobs = nj;
      launch_stem_reduce(ra, st);
      if ((rc = launch_ok("stem_reduce")) != NODE_OK) return rc;
      memset(&ra, 0, sizeof(ra));
      nj = 0; slot = 0;
    }
  }
  launch_stem_to_nchw(p.gf[cur], d_x, N, C, HW, st);
  return launch_ok("node_trunk_bwd");
}

}  // extern "C"
