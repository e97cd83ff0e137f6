// C ABI of the ResNet baseline's residual trunk with norm = 'batch' (include/node_hip.h: node_bntrunk_fwd / node_bntrunk_bwd):
// `blocks` x ResBlock(C, C, norm='batch'), stride 1, identity shortcut -- model.py:79 (`features`), model.py:284-310 with
// model.py:274 (nn.BatchNorm2d(C, track_running_stats=False)) -- as a host-side plan.  It is trunk_api.hip with the other
// norm: the BatchNorm passes of kernels_batchnorm.hip (two-stage statistics, Chan's formula, fp64 backward partials; T = nullptr,
// there is no time channel here) around the stem's gather-GEMM convolutions, data gradients and split-K weight gradients
// (kernels_stem.hip, used as they are).  NHWC inside the workspace, NCHW at the boundary.
//
// forward:   filters -> triples (6 per launch), zero rows | NCHW -> NHWC | per block: stats, apply (norm1 + ReLU -> triples) |
//            conv1 | stats, apply (norm2 + ReLU -> triples) | conv2 (+ x in the epilogue) [| NHWC -> NCHW into taps[i]] |
//            NHWC -> NCHW
// backward:  NCHW -> NHWC (fp32 + triples) | per block, last first: wgrad conv2 | dgrad conv2 | norm2': sums, dx (-> triples) |
//            wgrad conv1 | dgrad conv1 | norm1': sums, dx + the shortcut's gradient (k_bn_bwd_dx's SKIP variant; fp32 + triples:
//            the next block's dy) | one reduction launch per three blocks (6 slab sets) | NHWC -> NCHW into d_x
// dgamma / dbeta leave the dx passes directly (their chunk-0 workgroups), as in bnfunc_api.hip.
// Nothing is accumulated with atomics: every sum runs in a fixed order.
#include "bnfunc.h"
#include <cstring>
#include <vector>

using namespace node;

namespace {

constexpr int GROUP = 3;          // blocks per filter-preparation / reduction launch (SPrepArgs: 6 filters)

struct BnTrunkBlock {             // what one block keeps for its backward (keep = 0: every block uses set 0)
  Trip a1, a2;
  float* h;
  float *stats1, *stats2;
};
struct BnTrunkPlan {
  int N, C, H, W, B, R, cr, nchunk;
  float eps;
  bool keep;
  std::vector<Filt> c1, c2;
  std::vector<float*> xs;         // keep: B + 1 block inputs / outputs; otherwise two, used in turn
  std::vector<BnTrunkBlock> blk;
  float* part;                    // forward partials of the pass in flight
  // backward
  float* gf[2];
  Trip gt[2], dht;
  float* da;
  double* gpart;
  Wg w1[GROUP], w2[GROUP];
  size_t bytes;
};

BnTrunkPlan make_plan(const node_trunk_shape* sh, bool keep, void* base) {
  BnTrunkPlan p;
  p.N = sh->n; p.C = sh->channels; p.H = sh->h; p.W = sh->w; p.B = sh->blocks; p.eps = sh->eps; p.keep = keep;
  p.R = p.N * p.H * p.W;
  p.cr = bn_chunk_rows(p.R, p.C);
  p.nchunk = (p.R + p.cr - 1) / p.cr;
  const int C = p.C, B = p.B;
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
  for (BnTrunkBlock& k : p.blk) {
    k.a1 = take_trip(b, p.R, C);
    k.h = b.take<float>(RC);
    k.a2 = take_trip(b, p.R, C);
    k.stats1 = b.take<float>((size_t)2 * C);
    k.stats2 = b.take<float>((size_t)2 * C);
  }
  p.part = b.take<float>((size_t)p.nchunk * 2 * C);
  if (keep) {
    for (int i = 0; i < 2; ++i) {
      p.gf[i] = b.take<float>(RC);
      p.gt[i] = take_trip(b, p.R, C);
    }
    p.dht = take_trip(b, p.R, C);
    p.da = b.take<float>(RC);
    p.gpart = b.take<double>((size_t)p.nchunk * 2 * C);
    for (int i = 0; i < GROUP && i < B; ++i) {
      p.w1[i] = take_wg(b, p.R, C, C, 9, false);
      p.w2[i] = take_wg(b, p.R, C, C, 9, false);
    }
  }
  p.bytes = b.off + 256;
  return p;
}

int check_shape(const node_trunk_shape* sh) {
  if (!sh) return fail(NODE_ERR_NULL, "shape is NULL");
  if (sh->n <= 0 || sh->h <= 0 || sh->w <= 0 || sh->channels <= 0) return fail(NODE_ERR_SHAPE, "bad trunk shape");
  if (sh->blocks < 1) return fail(NODE_ERR_UNSUPPORTED, "the trunk takes blocks >= 1 (got %d)", sh->blocks);
  const int C = sh->channels;
  if (C < 64 || C % 64 != 0 || C > 4096)
    return fail(NODE_ERR_UNSUPPORTED, "the batch-norm trunk takes channels a multiple of 64 in [64, 4096]: 64-column GEMM tiles, "
                 "64-channel BatchNorm blocks (got %d)", C);
  const size_t elems = (size_t)sh->n * sh->h * sh->w * C;
  if (elems + C >= ((size_t)1 << 31)) return fail(NODE_ERR_UNSUPPORTED, "trunk tensors must stay under 2^31 elements");
  return NODE_OK;
}

// filters of blocks [i0, i1) -> triples, and the zero rows of `nz` triples tensors
int prep_group(const BnTrunkPlan& p, const node_trunk_block* blocks, int i0, int i1, const Trip* const* tz, int nz, hipStream_t st) {
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

int check_blocks(const void* blocks, int B, const char* what) {
  if (!blocks) return fail(NODE_ERR_NULL, "%s is NULL", what);
  for (int i = 0; i < B; ++i) {
    const void* const* pp = reinterpret_cast<const void* const*>(static_cast<const node_trunk_block*>(blocks) + i);
    for (int k = 0; k < 6; ++k) {
      if (!pp[k]) return fail(NODE_ERR_NULL, "tensor %d of block %d of %s is NULL", k, i, what);
      if (((uintptr_t)pp[k]) & 15) return fail(NODE_ERR_ARG, "tensor %d of block %d of %s must be 16-byte aligned", k, i, what);
    }
  }
  return NODE_OK;
}

int check_ptr(const void* p, const char* what, bool required) {
  if (!p) return required ? fail(NODE_ERR_NULL, "%s is NULL", what) : NODE_OK;
  if (((uintptr_t)p) & 15) return fail(NODE_ERR_ARG, "%s must be 16-byte aligned", what);
  return NODE_OK;
}

SBnArgs bn_args(const BnTrunkPlan& p, const float* h, const float* gamma, const float* beta, float* stats) {
  SBnArgs a;
  memset(&a, 0, sizeof(a));
  a.h = h; a.gamma = gamma; a.beta = beta; a.stats = stats;
  a.rows = p.R; a.C = p.C; a.H = p.H; a.W = p.W; a.chunk_rows = p.cr; a.nchunk = p.nchunk; a.relu = 1; a.eps = p.eps;
  a.out_scale = 1.0f; a.da_scale = 1.0f;
  return a;
}

#define LAUNCHED(what)                                  \
  do {                                                  \
    if ((rc = launch_ok(what)) != NODE_OK) return rc;   \
  } while (0)

// a3 = relu(norm(h)) as triples; leaves the batch statistics in `stats`
int norm_relu(const BnTrunkPlan& p, const float* h, const float* gamma, const float* beta, float* stats, const Trip& a3, hipStream_t st) {
  int rc;
  SBnArgs a = bn_args(p, h, gamma, beta, stats);
  a.part = p.part;
  launch_bn_stats(a, st);
  LAUNCHED("bn_stats");
  a.a3 = a3.p; a.a_plane = a3.plane;
  launch_bn_apply(a, st);
  LAUNCHED("bn_apply");
  return NODE_OK;
}

}  // namespace

extern "C" {

size_t node_bntrunk_workspace_bytes(const node_trunk_shape* shape, int keep_for_backward) {
  if (check_shape(shape) != NODE_OK) return 0;
  return make_plan(shape, keep_for_backward != 0, nullptr).bytes;
}

int node_bntrunk_describe(const node_trunk_shape* shape, node_bnfunc_info* out) {
  if (!out) return fail(NODE_ERR_NULL, "out is NULL");
  memset(out, 0, sizeof(*out));
  const int rc = check_shape(shape);
  if (rc != NODE_OK) return rc;
  const BnTrunkPlan p = make_plan(shape, true, nullptr);
  out->rows = p.R; out->chunk_rows = p.cr; out->nchunk = p.nchunk;
  out->last_chunk_rows = p.R - (p.nchunk - 1) * p.cr;
  out->column_tiles = p.C >> 6;
  out->wgrad_nsplit = p.w1[0].nsplit; out->wgrad_rows_per_split = p.w1[0].rps;      // (every slab set is taken with the same arguments)
  return NODE_OK;
}

int node_bntrunk_fwd(const node_trunk_shape* shape, const node_trunk_block* blocks, const float* x, float* out, float* taps,
                     int keep_for_backward, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_shape(shape);
  if (rc != NODE_OK) return rc;
  if ((rc = check_ptr(x, "x", true)) != NODE_OK || (rc = check_ptr(out, "out", true)) != NODE_OK ||
      (rc = check_ptr(taps, "taps", false)) != NODE_OK)
    return rc;
  if ((rc = check_blocks(blocks, shape->blocks, "blocks")) != NODE_OK) return rc;
  if (!ws) return fail(NODE_ERR_NULL, "workspace is NULL");
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const BnTrunkPlan p = make_plan(shape, keep_for_backward != 0, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "bntrunk workspace too small: %zu < %zu", ws_bytes, p.bytes);
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
  LAUNCHED("stem_from_nchw");
  const float* last = p.xs[0];
  for (int i = 0; i < B; ++i) {
    const BnTrunkBlock& k = p.blk[p.keep ? i : 0];
    const float* xin = p.keep ? p.xs[i] : p.xs[i & 1];
    float* xout = p.keep ? p.xs[i + 1] : p.xs[(i + 1) & 1];
    if ((rc = norm_relu(p, xin, blocks[i].n1_w, blocks[i].n1_b, k.stats1, k.a1, st)) != NODE_OK) return rc;
    launch_stem_conv(conv_fwd_args(k.a1, p.c1[i], k.h, N, H, W, H, W, 3, 1, 1), st);
    LAUNCHED("stem_conv");
    if ((rc = norm_relu(p, k.h, blocks[i].n2_w, blocks[i].n2_b, k.stats2, k.a2, st)) != NODE_OK) return rc;
    {   // y = conv2(a2) + x
      SConvArgs c = conv_fwd_args(k.a2, p.c2[i], xout, N, H, W, H, W, 3, 1, 1);
      c.res = xin;
      launch_stem_conv(c, st);
      LAUNCHED("stem_conv");
    }
    if (taps) {
      launch_stem_to_nchw(xout, taps + (size_t)i * p.R * C, N, C, HW, st);
      LAUNCHED("stem_to_nchw");
    }
    last = xout;
  }
  launch_stem_to_nchw(last, out, N, C, HW, st);
  return launch_ok("node_bntrunk_fwd");
}

int node_bntrunk_bwd(const node_trunk_shape* shape, const node_trunk_block* blocks, const float* grad_out,
                     const node_trunk_block_grads* grads, float* d_x, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_shape(shape);
  if (rc != NODE_OK) return rc;
  if ((rc = check_ptr(grad_out, "grad_out", true)) != NODE_OK || (rc = check_ptr(d_x, "d_x", true)) != NODE_OK) return rc;
  if ((rc = check_blocks(blocks, shape->blocks, "blocks")) != NODE_OK) return rc;
  if ((rc = check_blocks(grads, shape->blocks, "grads")) != NODE_OK) return rc;
  if (!ws) return fail(NODE_ERR_NULL, "workspace is NULL");
  if (((uintptr_t)ws) & 255) return fail(NODE_ERR_ARG, "workspace must be 256-byte aligned");
  const BnTrunkPlan p = make_plan(shape, true, ws);
  if (ws_bytes < p.bytes) return fail(NODE_ERR_WORKSPACE, "bntrunk workspace too small: %zu < %zu", ws_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int N = p.N, C = p.C, H = p.H, W = p.W, B = p.B, HW = H * W;

  // dL/d out: the last block's output gradient, as fp32 (its shortcut) and as triples (its conv2)
  int cur = 0;
  launch_stem_from_nchw(grad_out, p.gf[0], p.gt[0].p, p.gt[0].plane, N, C, HW, st);
  LAUNCHED("stem_from_nchw");
  SReduceArgs ra;
  memset(&ra, 0, sizeof(ra));
  int nj = 0, slot = 0;
  for (int i = B - 1; i >= 0; --i) {
    const BnTrunkBlock& k = p.blk[i];
    const Wg &w1 = p.w1[slot], &w2 = p.w2[slot];
    const Trip& g = p.gt[cur];
    // conv2: weight gradient, data gradient -> da
    launch_stem_wgrad(wgrad_args(g, nullptr, k.a2, w2, N, H, W, H, W, C, C, 3, 1, 1), st);
    LAUNCHED("stem_wgrad");
    launch_stem_conv(conv_dgrad_args(g, p.c2[i], p.da, N, H, W, H, W, 3, 1, 1), st);
    LAUNCHED("stem_conv");
    {   // norm2 + ReLU: dh -> triples
      SBnArgs a = bn_args(p, k.h, blocks[i].n2_w, blocks[i].n2_b, k.stats2);
      a.da = p.da; a.gpart = p.gpart;
      launch_bn_bwd_stats(a, st);
      LAUNCHED("bn_bwd_stats");
      a.dh3 = p.dht.p; a.dh_plane = p.dht.plane;
      a.dgamma = grads[i].n2_w; a.dbeta = grads[i].n2_b;
      launch_bn_bwd_dx(a, st);
      LAUNCHED("bn_bwd_dx");
    }
    // conv1
    launch_stem_wgrad(wgrad_args(p.dht, nullptr, k.a1, w1, N, H, W, H, W, C, C, 3, 1, 1), st);
    LAUNCHED("stem_wgrad");
    launch_stem_conv(conv_dgrad_args(p.dht, p.c1[i], p.da, N, H, W, H, W, 3, 1, 1), st);
    LAUNCHED("stem_conv");
    {   // dx = norm1'(da) + dy: the gradient of the block's input, which is the output gradient of block i - 1
      SBnArgs a = bn_args(p, p.xs[i], blocks[i].n1_w, blocks[i].n1_b, k.stats1);
      a.da = p.da; a.gpart = p.gpart;
      launch_bn_bwd_stats(a, st);
      LAUNCHED("bn_bwd_stats");
      a.skip = p.gf[cur]; a.dh = p.gf[cur ^ 1];
      if (i > 0) { a.dh3 = p.gt[cur ^ 1].p; a.dh_plane = p.gt[cur ^ 1].plane; }
      a.dgamma = grads[i].n1_w; a.dbeta = grads[i].n1_b;
      launch_bn_bwd_dx(a, st);
      LAUNCHED("bn_bwd_dx");
      cur ^= 1;
    }
    ra.job[nj++] = {w2.slab, grads[i].c2_w, nullptr, 0, w2.nsplit, C, C, 9};
    ra.job[nj++] = {w1.slab, grads[i].c1_w, nullptr, 0, w1.nsplit, C, C, 9};
    if (++slot == GROUP || i == 0) {     // the slab sets are free again behind this launch
      ra.njobs = nj;
      launch_stem_reduce(ra, st);
      LAUNCHED("stem_reduce");
      memset(&ra, 0, sizeof(ra));
      nj = 0; slot = 0;
    }
  }
  launch_stem_to_nchw(p.gf[cur], d_x, N, C, HW, st);
  return launch_ok("node_bntrunk_bwd");
}

}  // extern "C"
