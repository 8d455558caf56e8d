// mvc_posterior.hip — posterior clustering summary of S draws of a labeling of
// n items on the device: the step the reference's script leaves to mcclust /
// mcclust.ext after run_gibbs_cpp (New_Simulation.R:5-7 loads them; :189
// scores only the last draw).  No counterpart in the reference's C++.
//
//   compare   every pair of draws (s, t), s < t, through its contingency table:
//             a = sum C(n_ij,2), sa = sum C(n_i.,2), sb = sum C(n_.j,2) (exact
//             uint64, as mvc_ari.hip) and the fp64 sums of x ln x over the
//             cells, the row margin and the column margin (mvc_log_nb).
//               Binder distance  B(s,t) = sa + sb - 2 a   (item pairs on which
//                 the draws disagree; an exact integer)
//               VI in bits (mcclust.ext::VI)
//                 VI(s,t) = ((sum n_i. ln n_i. + sum n_.j ln n_.j)
//                            - 2 sum n_ij ln n_ij) / n / ln 2
//             The diagonal is 0 by definition.  binder_sum[s] = sum_t B(s,t),
//             vi_sum[s] = sum_t VI(s,t) added serially in ascending t; best[0]
//             and best[1] are their argmins, ties to the lowest index.  For
//             Binder that is mcclust::minbinder(method = "draws") (its PSM loss
//             is linear in the draws).  For VI it is the exact posterior
//             expected VI over the draws, NOT mcclust.ext::minVI's lower bound
//             (which swaps the log and the expectation).
//   psm       counts[i][j] = draws in which i and j share a label (divide by S
//             for mcclust::comp.psm).
//   gather    label[r][i] = dish[r][table_of[r][i]] for the saved samples of a
//             result (get_final_clusters, New_Simulation.R:135-149, for every
//             sample instead of the last).
//
// Kernel shapes.  compare: one workgroup per pair.  The table and both margins
// are one LDS histogram when ra rb + ra + rb <= kPostLdsCells (128 KiB of the
// CU's 160 KiB; the reduction keeps 384 bytes of its own); wider pairs count
// into a global scratch table with integer atomics, a batch of pairs per
// launch, the scratch cleared by a memset between batches.  One call mixes
// both.  Integer sums are order-free.  The fp64 sums use a fixed order: each
// thread adds its strided cells in ascending index, then a butterfly over the
// wave, then the waves (or the blocks' partials) in ascending order; there is
// no floating-point atomic, so equal inputs give equal bits.  psm: one 64 x 64
// tile of (i, j) per workgroup, 4 x 4 pairs per thread, the tile's row and
// column labels of 32 draws at a time staged in LDS; tiles on or above the
// diagonal only, mirrored on the way out.
#include <algorithm>
#include <climits>
#include <vector>

#include "mvc_host.h"
#include "mvc_internal.h"
#include "mvc_pmath.h"
#include "mvc_posterior_host.h"

namespace {

constexpr int kPairThreads = 512;              // LDS pair kernel: 8 waves
constexpr int kPairWaves = kPairThreads / 64;
constexpr int kThreads = 256;
constexpr int kParts = 128;                    // blocks that reduce one global-path table
constexpr int kPsmTile = 64;
constexpr int kPsmDraws = 32;                  // draws staged per LDS pass
constexpr double kLn2 = 0.6931471805599453;    // M_LN2

__device__ __forceinline__ unsigned long long pairs2(uint32_t c) {
  return (unsigned long long)c * (c - (c > 0 ? 1u : 0u)) / 2ull;
}
__device__ __forceinline__ double xlnx(uint32_t c) {   // 0 ln 0 = 1 ln 1 = 0 exactly
  return c > 1u ? (double)c * mvc_log_nb((double)c) : 0.0;
}

// three integer and three fp64 running sums: cells, row margin, column margin
struct Acc {
  unsigned long long u[3] = {0, 0, 0};
  double f[3] = {0.0, 0.0, 0.0};
  __device__ __forceinline__ void add(int which, uint32_t c) {
    const unsigned long long p = pairs2(c);
    const double x = xlnx(c);
    for (int k = 0; k < 3; ++k) {   // selects, not an indexed array: the sums stay in registers (x + 0.0 == x)
      u[k] += which == k ? p : 0ull;
      f[k] += which == k ? x : 0.0;
    }
  }
  __device__ __forceinline__ void wave_reduce() {   // fixed butterfly: every lane ends with the same bits
    for (int o = 32; o > 0; o >>= 1)
      for (int k = 0; k < 3; ++k) {
        u[k] += __shfl_xor(u[k], o, 64);
        f[k] += __shfl_xor(f[k], o, 64);
      }
  }
};

__device__ __forceinline__ void write_pair(const Acc &A, int64_t n, int64_t S, int s, int t, unsigned long long *binder,
                                           double *vi) {
  const unsigned long long B = A.u[1] + A.u[2] - 2ull * A.u[0];
  const double v = (((A.f[1] + A.f[2]) - 2.0 * A.f[0]) / (double)n) / kLn2;
  binder[(int64_t)s * S + t] = B;
  binder[(int64_t)t * S + s] = B;
  vi[(int64_t)s * S + t] = v;
  vi[(int64_t)t * S + s] = v;
}

// rng[2 s] = min, rng[2 s + 1] = max of draw s = blockIdx.y
__global__ __launch_bounds__(kThreads) void mvc_post_range_kernel(const int32_t *labels, int64_t n, int32_t *rng) {
  const int32_t *a = labels + (int64_t)blockIdx.y * n;
  int lo = INT_MAX, hi = INT_MIN;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = a[i];
    lo = min(lo, x);
    hi = max(hi, x);
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o, 64));
    hi = max(hi, __shfl_xor(hi, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(rng + 2 * blockIdx.y, lo);
    atomicMax(rng + 2 * blockIdx.y + 1, hi);
  }
}

// Pair (s, t) = (blockIdx.y, blockIdx.x): the diagonal is written as 0, blocks
// below it and pairs wider than lds_words (the global path's) leave at once.
__global__ __launch_bounds__(kPairThreads) void mvc_post_pair_lds_kernel(const int32_t *labels, int64_t n, int64_t S,
                                                                         const int32_t *rng, int lds_words,
                                                                         unsigned long long *binder, double *vi) {
  extern __shared__ uint32_t s_h[];
  __shared__ unsigned long long s_u[3][kPairWaves];
  __shared__ double s_f[3][kPairWaves];
  const int s = blockIdx.y, t = blockIdx.x;
  if (t < s) return;
  if (t == s) {
    if (threadIdx.x == 0) {
      binder[(int64_t)s * S + s] = 0ull;
      vi[(int64_t)s * S + s] = 0.0;
    }
    return;
  }
  const int lo_a = rng[2 * s], lo_b = rng[2 * t];
  const int64_t ra = (int64_t)rng[2 * s + 1] - lo_a + 1, rb = (int64_t)rng[2 * t + 1] - lo_b + 1;
  if (ra > lds_words || rb > lds_words) return;   // keeps the product below 2^63
  const int64_t cells = ra * rb, total = cells + ra + rb;
  if (total > lds_words) return;
  for (int k = threadIdx.x; k < total; k += kPairThreads) s_h[k] = 0;
  __syncthreads();
  const int32_t *a = labels + (int64_t)s * n, *b = labels + (int64_t)t * n;
  for (int64_t i = threadIdx.x; i < n; i += kPairThreads) {
    const int r = a[i] - lo_a, c = b[i] - lo_b;
    atomicAdd(s_h + r * (int)rb + c, 1u);
    atomicAdd(s_h + (int)cells + r, 1u);
    atomicAdd(s_h + (int)(cells + ra) + c, 1u);
  }
  __syncthreads();
  Acc A;
  for (int k = threadIdx.x; k < total; k += kPairThreads) A.add(k < cells ? 0 : (k < cells + ra ? 1 : 2), s_h[k]);
  A.wave_reduce();
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 3; ++k) {
      s_u[k][threadIdx.x >> 6] = A.u[k];
      s_f[k][threadIdx.x >> 6] = A.f[k];
    }
  __syncthreads();
  if (threadIdx.x == 0) {
    Acc R;
    for (int w = 0; w < kPairWaves; ++w)
      for (int k = 0; k < 3; ++k) {
        R.u[k] += s_u[k][w];
        R.f[k] += s_f[k][w];
      }
    write_pair(R, n, S, s, t, binder, vi);
  }
}

// Global path, pair p = blockIdx.y of the batch: pr[3 p] = s, t, and
// off[p] the pair's first scratch word (table, then rows, then columns).
__global__ __launch_bounds__(kThreads) void mvc_post_pair_count_kernel(const int32_t *labels, int64_t n,
                                                                       const int32_t *rng, const int32_t *pr,
                                                                       const int64_t *off, uint32_t *scratch) {
  const int s = pr[2 * blockIdx.y], t = pr[2 * blockIdx.y + 1];
  const int lo_a = rng[2 * s], lo_b = rng[2 * t];
  const int64_t ra = (int64_t)rng[2 * s + 1] - lo_a + 1, rb = (int64_t)rng[2 * t + 1] - lo_b + 1;
  uint32_t *cont = scratch + off[blockIdx.y], *rows = cont + ra * rb, *cols = rows + ra;
  const int32_t *a = labels + (int64_t)s * n, *b = labels + (int64_t)t * n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = (int64_t)a[i] - lo_a, c = (int64_t)b[i] - lo_b;
    atomicAdd(cont + r * rb + c, 1u);
    atomicAdd(rows + r, 1u);
    atomicAdd(cols + c, 1u);
  }
}

// Block g = blockIdx.x of kParts reduces its strided share of pair p's table
// into part[(p kParts + g) * 3 ..]; the grid shape is fixed, so the order is.
__global__ __launch_bounds__(kThreads) void mvc_post_pair_part_kernel(const int32_t *rng, const int32_t *pr,
                                                                      const int64_t *off, const uint32_t *scratch,
                                                                      unsigned long long *part_u, double *part_f) {
  __shared__ unsigned long long s_u[3][kThreads / 64];
  __shared__ double s_f[3][kThreads / 64];
  const int s = pr[2 * blockIdx.y], t = pr[2 * blockIdx.y + 1];
  const int64_t ra = (int64_t)rng[2 * s + 1] - rng[2 * s] + 1, rb = (int64_t)rng[2 * t + 1] - rng[2 * t] + 1;
  const int64_t cells = ra * rb, total = cells + ra + rb;
  const uint32_t *h = scratch + off[blockIdx.y];
  Acc A;
  for (int64_t k = blockIdx.x * (int64_t)kThreads + threadIdx.x; k < total; k += (int64_t)kParts * kThreads)
    A.add(k < cells ? 0 : (k < cells + ra ? 1 : 2), h[k]);
  A.wave_reduce();
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 3; ++k) {
      s_u[k][threadIdx.x >> 6] = A.u[k];
      s_f[k][threadIdx.x >> 6] = A.f[k];
    }
  __syncthreads();
  if (threadIdx.x == 0) {
    Acc R;
    for (int w = 0; w < kThreads / 64; ++w)
      for (int k = 0; k < 3; ++k) {
        R.u[k] += s_u[k][w];
        R.f[k] += s_f[k][w];
      }
    const int64_t o = ((int64_t)blockIdx.y * kParts + blockIdx.x) * 3;
    for (int k = 0; k < 3; ++k) {
      part_u[o + k] = R.u[k];
      part_f[o + k] = R.f[k];
    }
  }
}

// One thread per pair of the batch: the kParts partials in ascending order.
__global__ __launch_bounds__(64) void mvc_post_pair_final_kernel(const int32_t *pr, int np, const unsigned long long *part_u,
                                                                 const double *part_f, int64_t n, int64_t S,
                                                                 unsigned long long *binder, double *vi) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= np) return;
  Acc R;
  for (int g = 0; g < kParts; ++g)
    for (int k = 0; k < 3; ++k) {
      R.u[k] += part_u[((int64_t)p * kParts + g) * 3 + k];
      R.f[k] += part_f[((int64_t)p * kParts + g) * 3 + k];
    }
  write_pair(R, n, S, pr[2 * p], pr[2 * p + 1], binder, vi);
}

// binder_sum[s], vi_sum[s]: row s added serially in ascending t.  The
// matrices are symmetric bit for bit, so column s is read (coalesced).
__global__ __launch_bounds__(kThreads) void mvc_post_loss_kernel(const unsigned long long *binder, const double *vi,
                                                                 int64_t S, unsigned long long *bsum, double *vsum) {
  const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (s >= S) return;
  unsigned long long b = 0;
  double v = 0.0;
  for (int64_t t = 0; t < S; ++t) {
    b += binder[t * S + s];
    v += vi[t * S + s];
  }
  bsum[s] = b;
  vsum[s] = v;
}

// best[0] = argmin binder_sum, best[1] = argmin vi_sum, ties to the lowest index (one block)
__global__ __launch_bounds__(kThreads) void mvc_post_argmin_kernel(const unsigned long long *bsum, const double *vsum,
                                                                   int64_t S, int32_t *best) {
  __shared__ unsigned long long s_b[kThreads];
  __shared__ double s_v[kThreads];
  __shared__ int s_bi[kThreads], s_vi[kThreads];
  unsigned long long b = ~0ull;
  double v = MVC_PM_INF;
  int bi = INT_MAX, vi = INT_MAX;
  for (int64_t s = threadIdx.x; s < S; s += kThreads) {   // ascending s: strict < keeps the lowest index
    if (bsum[s] < b || bi == INT_MAX) { b = bsum[s]; bi = (int)s; }
    if (vsum[s] < v || vi == INT_MAX) { v = vsum[s]; vi = (int)s; }
  }
  s_b[threadIdx.x] = b; s_bi[threadIdx.x] = bi;
  s_v[threadIdx.x] = v; s_vi[threadIdx.x] = vi;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      const int j = threadIdx.x + o;
      if (s_bi[j] != INT_MAX && (s_bi[threadIdx.x] == INT_MAX || s_b[j] < s_b[threadIdx.x] ||
                                 (s_b[j] == s_b[threadIdx.x] && s_bi[j] < s_bi[threadIdx.x]))) {
        s_b[threadIdx.x] = s_b[j];
        s_bi[threadIdx.x] = s_bi[j];
      }
      if (s_vi[j] != INT_MAX && (s_vi[threadIdx.x] == INT_MAX || s_v[j] < s_v[threadIdx.x] ||
                                 (s_v[j] == s_v[threadIdx.x] && s_vi[j] < s_vi[threadIdx.x]))) {
        s_v[threadIdx.x] = s_v[j];
        s_vi[threadIdx.x] = s_vi[j];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    best[0] = s_bi[0];
    best[1] = s_vi[0];
  }
}

// Tile (bi, bj) = (blockIdx.y, blockIdx.x) of 64 x 64 item pairs, bj >= bi;
// thread (ty, tx) of 16 x 16 owns rows 4 ty .. 4 ty + 3, columns 4 tx .. 4 tx + 3.
__global__ __launch_bounds__(kThreads) void mvc_post_psm_kernel(const int32_t *labels, int64_t S, int64_t n,
                                                                uint32_t *counts) {
  __shared__ int32_t s_r[kPsmDraws][kPsmTile], s_c[kPsmDraws][kPsmTile];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  const int64_t i0 = (int64_t)bi * kPsmTile, j0 = (int64_t)bj * kPsmTile;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  uint32_t cnt[4][4] = {};
  for (int64_t d0 = 0; d0 < S; d0 += kPsmDraws) {
    const int nd = (int)min((int64_t)kPsmDraws, S - d0);
    for (int k = threadIdx.x; k < nd * kPsmTile; k += kThreads) {
      const int d = k / kPsmTile, x = k % kPsmTile;
      const int32_t *row = labels + (d0 + d) * n;
      s_r[d][x] = i0 + x < n ? row[i0 + x] : 0;   // items past n: compared, never written
      s_c[d][x] = j0 + x < n ? row[j0 + x] : 0;
    }
    __syncthreads();
    for (int d = 0; d < nd; ++d) {
      int32_t r[4], c[4];
      for (int k = 0; k < 4; ++k) {
        r[k] = s_r[d][4 * ty + k];
        c[k] = s_c[d][4 * tx + k];
      }
      for (int p = 0; p < 4; ++p)
        for (int q = 0; q < 4; ++q) cnt[p][q] += r[p] == c[q] ? 1u : 0u;
    }
    __syncthreads();
  }
  for (int p = 0; p < 4; ++p)
    for (int q = 0; q < 4; ++q) {
      const int64_t i = i0 + 4 * ty + p, j = j0 + 4 * tx + q;
      if (i < n && j < n) {
        counts[i * n + j] = cnt[p][q];
        counts[j * n + i] = cnt[p][q];
      }
    }
}

// out[r][i] = dish[off[r] + table_of[r][i]], r = blockIdx.y; a table position
// outside the sample's tables (a corrupt result) gives -1 instead of a stray read.
__global__ __launch_bounds__(kThreads) void mvc_post_gather_kernel(const int32_t *table_of, int64_t n,
                                                                   const int32_t *dish, const int64_t *off,
                                                                   int32_t *out) {
  const int64_t r = blockIdx.y, T = off[r + 1] - off[r];
  const int32_t *t = table_of + r * n, *d = dish + off[r];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t x = t[i];
    out[r * n + i] = (x >= 0 && x < T) ? d[x] : -1;
  }
}

template <class Tp>
struct DMem {
  Tp *p = nullptr;
  explicit DMem(size_t n) { MVC_HIP(hipMalloc(&p, sizeof(Tp) * std::max<size_t>(n, 1))); }
  DMem(const DMem &) = delete;
  DMem &operator=(const DMem &) = delete;
  ~DMem() { if (p) hipFree(p); }
};

template <class Tp>
void upload(Tp *dst, const std::vector<Tp> &src, hipStream_t st) {
  if (!src.empty()) MVC_HIP(hipMemcpyAsync(dst, src.data(), sizeof(Tp) * src.size(), hipMemcpyHostToDevice, st));
}

}  // namespace

namespace mvc {

void partition_compare(int device, const int32_t *labels, int64_t S, int64_t n, uint64_t *binder, double *vi,
                       uint64_t *binder_sum, double *vi_sum, int32_t *best) {
  MVC_HIP(hipSetDevice(device));
  hipStream_t st = nullptr;
  DMem<int32_t> lab((size_t)S * n);
  DMem<int32_t> rng(2 * (size_t)S);
  MVC_HIP(hipMemcpyAsync(lab.p, labels, sizeof(int32_t) * (size_t)S * n, hipMemcpyHostToDevice, st));
  std::vector<int32_t> h_rng(2 * (size_t)S);
  for (int64_t s = 0; s < S; ++s) {
    h_rng[2 * s] = INT_MAX;
    h_rng[2 * s + 1] = INT_MIN;
  }
  upload(rng.p, h_rng, st);
  const unsigned gx = (unsigned)std::min<int64_t>(64, (n + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(mvc_post_range_kernel, dim3(gx, (unsigned)S), dim3(kThreads), 0, st, (const int32_t *)lab.p, n,
                     rng.p);
  MVC_HIP(hipGetLastError());
  MVC_HIP(hipMemcpyAsync(h_rng.data(), rng.p, sizeof(int32_t) * h_rng.size(), hipMemcpyDeviceToHost, st));
  MVC_HIP(hipStreamSynchronize(st));
  std::vector<int64_t> range((size_t)S);
  for (int64_t s = 0; s < S; ++s) range[s] = (int64_t)h_rng[2 * s + 1] - h_rng[2 * s] + 1;
  const PairPlan P = plan_pairs(range);
  if (P.too_wide)
    throw Error(MVC_ERR_UNSUPPORTED,
                "partition_compare: label ranges too wide for a pair's contingency table (range_s * range_t > 2^26)");

  DMem<unsigned long long> d_b((size_t)S * S), d_bs((size_t)S);
  DMem<double> d_v((size_t)S * S), d_vs((size_t)S);
  DMem<int32_t> d_best(2);
  // every pair that fits LDS, and the zero diagonal
  static_assert(sizeof(uint32_t) * kPostLdsCells + 2 * 3 * kPairWaves * 8 <= 160 * 1024, "LDS of one CU");
  const size_t lds_bytes = sizeof(uint32_t) * (size_t)P.lds_words;
  MVC_HIP(hipFuncSetAttribute((const void *)mvc_post_pair_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(sizeof(uint32_t) * kPostLdsCells)));
  hipLaunchKernelGGL(mvc_post_pair_lds_kernel, dim3((unsigned)S, (unsigned)S), dim3(kPairThreads), lds_bytes, st,
                     (const int32_t *)lab.p, n, S, (const int32_t *)rng.p, P.lds_words, d_b.p, d_v.p);
  MVC_HIP(hipGetLastError());
  // the wider pairs, a batch at a time through global scratch
  if (!P.global.empty()) {
    size_t most = 0;
    for (size_t b = 0; b + 1 < P.batch_begin.size(); ++b)
      most = std::max<size_t>(most, (size_t)(P.batch_begin[b + 1] - P.batch_begin[b]));
    DMem<uint32_t> scratch((size_t)P.scratch_words);
    DMem<int32_t> d_pr(2 * most);
    DMem<int64_t> d_off(most);
    DMem<unsigned long long> part_u(most * kParts * 3);
    DMem<double> part_f(most * kParts * 3);
    const unsigned cgx = (unsigned)std::min<int64_t>(1024, (n + kThreads - 1) / kThreads);
    for (size_t b = 0; b + 1 < P.batch_begin.size(); ++b) {
      const int64_t p0 = P.batch_begin[b], np = P.batch_begin[b + 1] - p0;
      std::vector<int32_t> pr(2 * (size_t)np);
      std::vector<int64_t> off((size_t)np);
      int64_t words = 0;
      for (int64_t p = 0; p < np; ++p) {
        const GlobalPair &g = P.global[p0 + p];
        pr[2 * p] = g.s;
        pr[2 * p + 1] = g.t;
        off[p] = g.off;
        words = std::max(words, g.off + pair_words(range[g.s], range[g.t]));
      }
      upload(d_pr.p, pr, st);
      upload(d_off.p, off, st);
      MVC_HIP(hipMemsetAsync(scratch.p, 0, sizeof(uint32_t) * (size_t)words, st));
      hipLaunchKernelGGL(mvc_post_pair_count_kernel, dim3(cgx, (unsigned)np), dim3(kThreads), 0, st,
                         (const int32_t *)lab.p, n, (const int32_t *)rng.p, (const int32_t *)d_pr.p,
                         (const int64_t *)d_off.p, scratch.p);
      MVC_HIP(hipGetLastError());
      hipLaunchKernelGGL(mvc_post_pair_part_kernel, dim3(kParts, (unsigned)np), dim3(kThreads), 0, st,
                         (const int32_t *)rng.p, (const int32_t *)d_pr.p, (const int64_t *)d_off.p,
                         (const uint32_t *)scratch.p, part_u.p, part_f.p);
      MVC_HIP(hipGetLastError());
      hipLaunchKernelGGL(mvc_post_pair_final_kernel, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, st,
                         (const int32_t *)d_pr.p, (int)np, (const unsigned long long *)part_u.p,
                         (const double *)part_f.p, n, S, d_b.p, d_v.p);
      MVC_HIP(hipGetLastError());
      MVC_HIP(hipStreamSynchronize(st));   // pr / off are reused by the next batch
    }
  }
  hipLaunchKernelGGL(mvc_post_loss_kernel, dim3((unsigned)((S + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                     (const unsigned long long *)d_b.p, (const double *)d_v.p, S, d_bs.p, d_vs.p);
  MVC_HIP(hipGetLastError());
  hipLaunchKernelGGL(mvc_post_argmin_kernel, dim3(1), dim3(kThreads), 0, st, (const unsigned long long *)d_bs.p,
                     (const double *)d_vs.p, S, d_best.p);
  MVC_HIP(hipGetLastError());
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "uint64_t outputs");
  if (binder) MVC_HIP(hipMemcpyAsync(binder, d_b.p, sizeof(uint64_t) * (size_t)S * S, hipMemcpyDeviceToHost, st));
  if (vi) MVC_HIP(hipMemcpyAsync(vi, d_v.p, sizeof(double) * (size_t)S * S, hipMemcpyDeviceToHost, st));
  if (binder_sum) MVC_HIP(hipMemcpyAsync(binder_sum, d_bs.p, sizeof(uint64_t) * (size_t)S, hipMemcpyDeviceToHost, st));
  if (vi_sum) MVC_HIP(hipMemcpyAsync(vi_sum, d_vs.p, sizeof(double) * (size_t)S, hipMemcpyDeviceToHost, st));
  if (best) MVC_HIP(hipMemcpyAsync(best, d_best.p, sizeof(int32_t) * 2, hipMemcpyDeviceToHost, st));
  MVC_HIP(hipStreamSynchronize(st));
}

void partition_psm(int device, const int32_t *labels, int64_t S, int64_t n, uint32_t *counts) {
  MVC_HIP(hipSetDevice(device));
  hipStream_t st = nullptr;
  DMem<int32_t> lab((size_t)S * n);
  DMem<uint32_t> cnt((size_t)n * n);
  MVC_HIP(hipMemcpyAsync(lab.p, labels, sizeof(int32_t) * (size_t)S * n, hipMemcpyHostToDevice, st));
  const unsigned nt = (unsigned)((n + kPsmTile - 1) / kPsmTile);   // <= 256 tiles a side
  hipLaunchKernelGGL(mvc_post_psm_kernel, dim3(nt, nt), dim3(kThreads), 0, st, (const int32_t *)lab.p, S, n, cnt.p);
  MVC_HIP(hipGetLastError());
  MVC_HIP(hipMemcpyAsync(counts, cnt.p, sizeof(uint32_t) * (size_t)n * n, hipMemcpyDeviceToHost, st));
  MVC_HIP(hipStreamSynchronize(st));
}

void gather_labels(int device, const int32_t *table_of, int64_t R, int64_t n, const std::vector<int32_t> &dish,
                   const std::vector<int64_t> &off, int32_t *out) {
  MVC_HIP(hipSetDevice(device));
  hipStream_t st = nullptr;
  DMem<int32_t> d_t((size_t)R * n), d_out((size_t)R * n), d_dish(dish.size());
  DMem<int64_t> d_off(off.size());
  MVC_HIP(hipMemcpyAsync(d_t.p, table_of, sizeof(int32_t) * (size_t)R * n, hipMemcpyHostToDevice, st));
  upload(d_dish.p, dish, st);
  upload(d_off.p, off, st);
  const unsigned gx = (unsigned)std::min<int64_t>(256, (n + kThreads - 1) / kThreads);
  // samples go on grid.y in slices of at most 32768
  for (int64_t r0 = 0; r0 < R; r0 += 32768) {
    const int64_t nr = std::min<int64_t>(32768, R - r0);
    hipLaunchKernelGGL(mvc_post_gather_kernel, dim3(gx, (unsigned)nr), dim3(kThreads), 0, st,
                       (const int32_t *)(d_t.p + r0 * n), n, (const int32_t *)d_dish.p,
                       (const int64_t *)(d_off.p + r0), d_out.p + r0 * n);
    MVC_HIP(hipGetLastError());
  }
  MVC_HIP(hipMemcpyAsync(out, d_out.p, sizeof(int32_t) * (size_t)R * n, hipMemcpyDeviceToHost, st));
  MVC_HIP(hipStreamSynchronize(st));
}

}  // namespace mvc
