// Retrieval evaluation (`evaluate.py retrieval` of the reference, evaluate.py:308-361): per query, the average precision of
// the database ranked by inner-product score, and the reference's AP@k.  Two kernels per chunk of query rows:
//
//   k_ret_scores  S[i][j] = Q[i] . X[j] on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32: exact f32 products, f32
//                 accumulation in k order).  64 x 64 tile per 256-thread workgroup, each wave one 32 x 32 tile; D is
//                 staged in chunks of 32 through LDS and zero-padded there (never in the caller's tensors).
//   k_ret_rank<NP> one 1024-thread workgroup per query row: the row's Nd scores become 64-bit keys
//                 (order-preserving score bits << 32 | database index), padded with zero keys to NP = 2^m >= max(Nd, 2048),
//                 bitonic-sorted DESCENDING in LDS (NP x 8 B <= 128 KiB).  Equal scores then sit together with the higher
//                 database index first: the stable ascending argsort reversed, which fixes which items of a tie group at the
//                 k boundary enter the top k.  -0.0 is keyed as +0.0 (sklearn's np.diff sees them as a tie).
//
// AP follows sklearn's average_precision_score: walking the ranking, a tie group is ONE threshold, and
//     AP = sum over groups (delta tp / P) * tp / (tp + fp)   =   (1 / P) * sum over relevant items p of tp(g(p)) / (g(p) + 1)
// where g(p) is the last position of p's tie group and tp(q) the relevant items in positions [0, q].  AP@k is the same sum
// over the window [0, min(k, Nd)) with g clipped to the window and P replaced by the relevant items inside it.  A row with
// no relevant item gives 0.0 (sklearn 1.7 returns 0 with a warning).  Sums in fp64, in a fixed order; no workgroup talks to
// another, so every output is bit-identical from run to run.
#include "node_internal.h"

namespace node {

namespace {

constexpr int SC_TILE = 64;      // score tile: 64 queries x 64 database items per workgroup
constexpr int SC_KC = 32;        // D staged per LDS chunk
constexpr int RK_THREADS = 1024;

typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void k_ret_scores(const float* __restrict__ q, const float* __restrict__ x, float* __restrict__ s,
                                                    int nq, int nd, int d) {
  __shared__ float qs[SC_TILE][SC_KC + 1];
  __shared__ float xs[SC_TILE][SC_KC + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.y * SC_TILE, x0 = blockIdx.x * SC_TILE;
  const int qw = (wave >> 1) * 32, xw = (wave & 1) * 32;
  const int r = lane & 31, h = lane >> 5;
  f32x16 acc;
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int k0 = 0; k0 < d; k0 += SC_KC) {
    for (int e = tid; e < SC_TILE * SC_KC; e += 256) {
      const int row = e / SC_KC, col = e % SC_KC, k = k0 + col;
      const int gq = q0 + row, gx = x0 + row;
      qs[row][col] = (gq < nq && k < d) ? q[(size_t)gq * d + k] : 0.f;
      xs[row][col] = (gx < nd && k < d) ? x[(size_t)gx * d + k] : 0.f;
    }
    __syncthreads();
    // lane (r, h) holds A[i = r][k = h] and B[k = h][j = r] of each 32 x 32 x 2 step
    for (int kk = 0; kk < SC_KC; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qs[qw + r][kk + h], xs[xw + r][kk + h], acc, 0, 0, 0);
    __syncthreads();
  }
  // C/D: column lane & 31, row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int gx = x0 + xw + r;
  if (gx >= nd) return;
  for (int i = 0; i < 16; ++i) {
    const int gq = q0 + qw + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (gq < nq) s[(size_t)gq * nd + gx] = acc[i];
  }
}

__device__ __forceinline__ unsigned long long rank_key(float v, int idx) {
  unsigned u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;                            // -0.0 ties with +0.0
  const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)ord << 32) | (unsigned)idx;
}

// exclusive prefix sum over the workgroup (1024 threads = 16 waves); *total <- the sum of all
__device__ __forceinline__ int block_exclusive_scan(int v, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int base = 0, all = 0;
  for (int w = 0; w < RK_THREADS / 64; ++w) {
    const int t = wsum[w];
    base += w < wave ? t : 0;
    all += t;
  }
  *total = all;
  return base + inc - v;
}

// fp64 sum over the workgroup in a fixed order: butterfly inside each wave, then the 16 wave partials in index order
__device__ __forceinline__ double block_sum(double v, double* wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (lane == 0) wsum[wave] = v;
  __syncthreads();
  double all = 0.0;
  for (int w = 0; w < RK_THREADS / 64; ++w) all += wsum[w];
  return all;
}

template <int NP>
__global__ __launch_bounds__(RK_THREADS) void k_ret_rank(const float* __restrict__ scores, int nd, const int* __restrict__ qlab,
                                                         const int* __restrict__ xlab, int k, double* __restrict__ ap,
                                                         double* __restrict__ ap_k) {
  constexpr int PER = NP / RK_THREADS;                    // consecutive ranks per thread after the sort (2..16)
  __shared__ unsigned long long key[NP];
  __shared__ int isum[RK_THREADS / 64];
  __shared__ double dsum[2][RK_THREADS / 64];
  const int tid = threadIdx.x, row = blockIdx.x;
  const float* __restrict__ srow = scores + (size_t)row * nd;
  for (int p = tid; p < NP; p += RK_THREADS) key[p] = p < nd ? rank_key(srow[p], p) : 0ull;
  __syncthreads();

  // bitonic sort, descending
  for (int len = 2; len <= NP; len <<= 1) {
    for (int j = len >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < NP / 2; i += RK_THREADS) {
        const int a = 2 * j * (i / j) + (i % j), b = a + j;
        const unsigned long long ka = key[a], kb = key[b];
        const bool desc = (a & len) == 0;
        if (desc ? ka < kb : ka > kb) {
          key[a] = kb;
          key[b] = ka;
        }
      }
      __syncthreads();
    }
  }

  // relevance of ranks [tid * PER, tid * PER + PER), then the running count of relevant items kept in the key's low word
  const int lab = qlab[row];
  const int p0 = tid * PER;
  unsigned rel = 0u;
  int cnt = 0;
  for (int c = 0; c < PER; ++c) {
    const int p = p0 + c;
    if (p < nd && xlab[(unsigned)key[p]] == lab) {
      rel |= 1u << c;
      ++cnt;
    }
  }
  int total;
  int run = block_exclusive_scan(cnt, isum, &total);
  for (int c = 0; c < PER; ++c) {
    const int p = p0 + c;
    if (p < nd) {
      run += (rel >> c) & 1u;
      key[p] = (key[p] & 0xFFFFFFFF00000000ull) | (unsigned)run;
    }
  }
  __syncthreads();

  const int kk = k < nd ? k : nd;
  double sa = 0.0, sk = 0.0;
  for (int c = 0; c < PER; ++c) {
    if (!((rel >> c) & 1u)) continue;
    const int p = p0 + c;
    const unsigned hi = (unsigned)(key[p] >> 32);
    int lo = p + 1, up = nd;                              // first rank after p with a lower score
    while (lo < up) {
      const int mid = (lo + up) >> 1;
      if ((unsigned)(key[mid] >> 32) == hi) lo = mid + 1;
      else up = mid;
    }
    const int g = lo - 1;
    sa += (double)(unsigned)key[g] / (double)(g + 1);
    if (p < kk) {
      const int gk = g < kk - 1 ? g : kk - 1;
      sk += (double)(unsigned)key[gk] / (double)(gk + 1);
    }
  }
  const int pk = (int)(unsigned)key[kk - 1];
  sa = block_sum(sa, dsum[0]);
  sk = block_sum(sk, dsum[1]);
  if (tid == 0) {
    ap[row] = total > 0 ? sa / (double)total : 0.0;
    ap_k[row] = pk > 0 ? sk / (double)pk : 0.0;
  }
}

}  // namespace

void launch_retrieval_scores(const float* q, const float* x, float* scores, int nq, int nd, int d, hipStream_t s) {
  dim3 grid((nd + SC_TILE - 1) / SC_TILE, (nq + SC_TILE - 1) / SC_TILE);
  hipLaunchKernelGGL(k_ret_scores, grid, dim3(256), 0, s, q, x, scores, nq, nd, d);
}

void launch_retrieval_rank(const float* scores, int nq, int nd, const int* qlab, const int* xlab, int k, double* ap, double* ap_k,
                           hipStream_t s) {
  if (nd <= 2048)
    hipLaunchKernelGGL(k_ret_rank<2048>, dim3(nq), dim3(RK_THREADS), 0, s, scores, nd, qlab, xlab, k, ap, ap_k);
  else if (nd <= 4096)
    hipLaunchKernelGGL(k_ret_rank<4096>, dim3(nq), dim3(RK_THREADS), 0, s, scores, nd, qlab, xlab, k, ap, ap_k);
  else if (nd <= 8192)
    hipLaunchKernelGGL(k_ret_rank<8192>, dim3(nq), dim3(RK_THREADS), 0, s, scores, nd, qlab, xlab, k, ap, ap_k);
  else
    hipLaunchKernelGGL(k_ret_rank<16384>, dim3(nq), dim3(RK_THREADS), 0, s, scores, nd, qlab, xlab, k, ap, ap_k);
}

}  // namespace node
