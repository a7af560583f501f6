// Size reduction before the spectral path: what the reference
// gets from sklearn's AgglomerativeClustering(metric="cosine", linkage="complete" |
// "average") (reference spectral_clusterer.py:170-199, multi_stage_clusterer.py:109-112,
// fallback_clusterer.py:108-113) and utils.get_cluster_centroids (utils.py:159-176).
//
// sklearn delegates to scipy.cluster.hierarchy.linkage: pdist(cosine), the nearest-
// neighbour-chain algorithm, a stable sort of the merges by height and a union-find
// relabelling; sklearn then cuts the tree with a heap of node ids (_hc_cut).  Here:
//   * distances: the fp64 MFMA GEMM of the affinity stage on the row-normalised embeddings,
//     d_ij = 1 - clip(cos_ij) (k_cosine_distance); every tile of that product takes the whole K
//     (no split-K tail), so equal rows give bit-equal distance columns, as scipy's pdist does --
//     the tie rules below decide sklearn's label numbering on such inputs;
//   * nearest-neighbour chain: ONE persistent workgroup (k_ahc_nn_chain).  The chain is
//     inherently sequential (about 3 n steps); each step is a coalesced scan of one row of
//     the n x n distance matrix (first index of the minimum, the previous chain element wins
//     ties, exactly scipy's loop) or a Lance-Williams update of one row + column;
//   * the O(n log n) tree bookkeeping (sort, relabel, heap cut) runs on the host: ahc_tree.cpp;
//   * a stream pool (pool_api.hip) runs the three device steps for all its sessions in one launch
//     each: k_pool_cosine_distance, k_ahc_nn_chain_pool (a workgroup per session),
//     k_pool_centroids; its fallback stage (sessions of up to 128 rows, average linkage) runs the
//     first two as k_pool_linkage_lds: the distance matrix in LDS, a wavefront per session;
//   * a batch of utterances of any size (batch_reduce.hip: sc_batch_ahc, sc_predict_batch_reduced)
//     runs them from a table of per-member descriptors: k_batch_cosine_distance,
//     k_ahc_nn_chain_batch (a workgroup per member), k_batch_linkage_lds, k_batch_centroids;
//   * the FallbackClusterer single-cluster test of a batch (sc_batch_fallback_check) asks only
//     whether a cut at the threshold leaves one cluster: the verdict forms of the two linkage
//     kernels, k_ahc_nn_chain_verdict and k_batch_linkage_lds_verdict, write a two-double record
//     per member instead of a merge list.
#include <hip/hip_runtime.h>

#include "dpp.h"
#include "sc_internal.h"

namespace sc {

// d = 1 - clip(c): scipy clips the cosine to [-1, 1].  A row's distance to itself is 0, as in
// scipy's squareform(pdist(.)): the product of a unit row with itself misses 1 by a few ulp
// (2 at d = 24, 6.5 at d = 256 were measured), and although no scan or update reads the diagonal
// (they skip i == x), D is the distance matrix only with the zero there.
__device__ __forceinline__ double cosine_distance_value(double v, bool diagonal) {
  v = v > 1.0 ? 1.0 : (v < -1.0 ? -1.0 : v);
  return diagonal ? 0.0 : 1.0 - v;
}

__global__ __launch_bounds__(256) void k_cosine_distance(double* __restrict__ c, int n,
                                                         int ld) {
  const int row = blockIdx.y;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= n) return;
  c[(size_t)row * ld + col] = cosine_distance_value(c[(size_t)row * ld + col], row == col);
}

constexpr int kAhcThreads = 1024;

// (value, index) minimum over the workgroup: smallest value, then smallest index
__device__ __forceinline__ void block_argmin(double& v, int& idx, double* s_val, int* s_idx) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(idx, o);
    if (ov < v || (ov == v && oi < idx)) {
      v = ov;
      idx = oi;
    }
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_val[wave] = v;
    s_idx[wave] = idx;
  }
  __syncthreads();
  v = s_val[0];
  idx = s_idx[0];
#pragma unroll
  for (int w = 1; w < kAhcThreads / 64; ++w) {
    if (s_val[w] < v || (s_val[w] == v && s_idx[w] < idx)) {
      v = s_val[w];
      idx = s_idx[w];
    }
  }
  __syncthreads();
}

// method 1: complete linkage (max), 2: average linkage (size-weighted mean).
// Z[k] = (x, y, height, size) in merge order, x < y slot indices (slot y keeps the cluster).
// The whole chain of one problem on the calling workgroup (kAhcThreads threads); n >= 2.
// kVerdict: "does a cut at `threshold` leave one cluster?" -- no merge list; Z is the problem's
// two-double record {height, verdict}.  One cluster means no merge height >= threshold (the cut
// counts 1 + #{heights >= threshold}, whatever order the chain emits the merges in): the first
// such height settles it and ends the chain (record {that height, 0}); a chain that ends without
// one leaves {the largest height, 1}.  The distances, the scans and the updates are the same
// expressions, so the heights are the merge list's, bit for bit.
template <bool kVerdict>
__device__ __forceinline__ void ahc_nn_chain_body(double* __restrict__ D, int ld, int n,
                                                  int method, int* __restrict__ size,
                                                  int* __restrict__ chain,
                                                  double* __restrict__ Z, double* s_val,
                                                  int* s_idx, double threshold = 0.0) {
  const int tid = threadIdx.x;
  const double inf = __builtin_huge_val();
  double top = -inf;  // (kVerdict) the largest height so far
  for (int i = tid; i < n; i += kAhcThreads) size[i] = 1;
  __syncthreads();
  int chain_len = 0;
  for (int k = 0; k < n - 1; ++k) {
    if (chain_len == 0) {  // first slot that is still a cluster
      double v = inf;
      int first = 0x7fffffff;
      for (int i = tid; i < n; i += kAhcThreads)
        if (size[i] > 0 && i < first) first = i;
      v = (double)first;
      block_argmin(v, first, s_val, s_idx);
      if (tid == 0) chain[0] = first;
      chain_len = 1;
      __syncthreads();
    }
    int x, y;
    double cur;
    while (true) {
      x = chain[chain_len - 1];
      const int y0 = chain_len > 1 ? chain[chain_len - 2] : -1;
      cur = y0 >= 0 ? D[(size_t)x * ld + y0] : inf;
      double best = inf;
      int besti = 0x7fffffff;
      const double* row = D + (size_t)x * ld;
      for (int i = tid; i < n; i += kAhcThreads) {
        if (size[i] > 0 && i != x) {
          const double v = row[i];
          if (v < best) {
            best = v;
            besti = i;
          }
        }
      }
      block_argmin(best, besti, s_val, s_idx);
      y = y0;
      if (best < cur) {
        cur = best;
        y = besti;
      }
      if (chain_len > 1 && y == y0) break;
      if (tid == 0) chain[chain_len] = y;
      ++chain_len;
      __syncthreads();
    }
    chain_len -= 2;
    if (x > y) {
      const int t = x;
      x = y;
      y = t;
    }
    const int nx = size[x], ny = size[y];
    __syncthreads();  // every thread has read the sizes
    if constexpr (kVerdict) {
      if (cur >= threshold) {  // (cur is the same value in every thread: all of them leave)
        if (tid == 0) {
          Z[0] = cur;
          Z[1] = 0.0;
        }
        return;
      }
      top = cur > top ? cur : top;
    }
    if (tid == 0) {
      if constexpr (!kVerdict) {
        Z[(size_t)k * 4 + 0] = (double)x;
        Z[(size_t)k * 4 + 1] = (double)y;
        Z[(size_t)k * 4 + 2] = cur;
        Z[(size_t)k * 4 + 3] = (double)(nx + ny);
      }
      size[x] = 0;
      size[y] = nx + ny;
    }
    const double* rx = D + (size_t)x * ld;
    double* ry = D + (size_t)y * ld;
    for (int i = tid; i < n; i += kAhcThreads) {
      if (i == x || i == y) continue;
      if (size[i] <= 0) continue;  // x and y are excluded above, the rest is unchanged
      const double dx = rx[i], dy = ry[i];
      const double nv = method == 1 ? (dx > dy ? dx : dy)
                                    : ((double)nx * dx + (double)ny * dy) / (double)(nx + ny);
      ry[i] = nv;
      D[(size_t)i * ld + y] = nv;
    }
    __syncthreads();
  }
  if constexpr (kVerdict) {
    if (tid == 0) {
      Z[0] = top;
      Z[1] = 1.0;
    }
  }
}

__global__ __launch_bounds__(kAhcThreads) void k_ahc_nn_chain(double* __restrict__ D, int ld,
                                                              int n, int method,
                                                              int* __restrict__ size,
                                                              int* __restrict__ chain,
                                                              double* __restrict__ Z,
                                                              const int* __restrict__ bad) {
  __shared__ double s_val[kAhcThreads / 64];
  __shared__ int s_idx[kAhcThreads / 64];
  // a NaN row of D leaves the last scans without a neighbour (index -1): the body needs finite
  // distances, the host reports the word
  if (bad != nullptr && *bad != 0) return;
  ahc_nn_chain_body<false>(D, ld, n, method, size, chain, Z, s_val, s_idx);
}

// ---- a batch of problems of any size (sc_batch_ahc): a table of descriptors in device memory,
//      position z of a launch works on table[first + z] ----
// rows blockIdx.x, blockIdx.x + gridDim.x, ... of member blockIdx.y
__global__ __launch_bounds__(256) void k_batch_cosine_distance(
    const AhcBatchItem* __restrict__ table, int first) {
  const AhcBatchItem& it = table[first + blockIdx.y];
  const int n = it.n, ld = it.ld;
  double* __restrict__ c = it.D;
  for (int row = blockIdx.x; row < n; row += gridDim.x)
    for (int col = threadIdx.x; col < n; col += 256) {
      c[(size_t)row * ld + col] = cosine_distance_value(c[(size_t)row * ld + col], row == col);
    }
}

// One persistent workgroup per member; the workgroups are independent (no wait between them),
// so the grid may exceed what the device holds at once.
__global__ __launch_bounds__(kAhcThreads) void k_ahc_nn_chain_batch(
    const AhcBatchItem* __restrict__ table, int first) {
  __shared__ double s_val[kAhcThreads / 64];
  __shared__ int s_idx[kAhcThreads / 64];
  const AhcBatchItem& it = table[first + blockIdx.x];
  if (it.n < 2 || *it.bad != 0) return;  // before D is touched
  ahc_nn_chain_body<false>(it.D, it.ld, it.n, it.method, it.size, it.chain, it.Z, s_val, s_idx);
}

// The verdict form (average linkage): it.Z is the member's record {height, verdict}
__global__ __launch_bounds__(kAhcThreads) void k_ahc_nn_chain_verdict(
    const AhcBatchItem* __restrict__ table, int first, double threshold) {
  __shared__ double s_val[kAhcThreads / 64];
  __shared__ int s_idx[kAhcThreads / 64];
  const AhcBatchItem& it = table[first + blockIdx.x];
  if (it.n < 2 || *it.bad != 0) return;  // before D is touched
  ahc_nn_chain_body<true>(it.D, it.ld, it.n, 2, it.size, it.chain, it.Z, s_val, s_idx, threshold);
}

// ---- stream pool: the same three steps for every session of a step in one launch each ----
// (PoolSlabs, sc_internal.h; position z of the launch works on slot slots[z] with rows[z] rows)
__global__ __launch_bounds__(256) void k_pool_cosine_distance(const PoolSlabs p,
                                                              const int* __restrict__ slots,
                                                              const int* __restrict__ rows) {
  const int n = rows[blockIdx.z];
  const int row = blockIdx.y;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (row >= n || col >= n) return;
  double* c = p.D + (size_t)slots[blockIdx.z] * p.stride_d;
  c[(size_t)row * p.ldd + col] = cosine_distance_value(c[(size_t)row * p.ldd + col], row == col);
}

// One persistent workgroup per session: sessions of different sizes share the launch, each
// workgroup runs its own chain to the end.
__global__ __launch_bounds__(kAhcThreads) void k_ahc_nn_chain_pool(const PoolSlabs p,
                                                                   const int* __restrict__ slots,
                                                                   const int* __restrict__ rows,
                                                                   int method) {
  __shared__ double s_val[kAhcThreads / 64];
  __shared__ int s_idx[kAhcThreads / 64];
  const int b = blockIdx.x;
  const int n = rows[b];
  if (n < 2) return;
  ahc_nn_chain_body<false>(p.D + (size_t)slots[b] * p.stride_d, p.ldd, n, method,
                    p.size + (size_t)b * p.stride_n, p.chain + (size_t)b * p.stride_n,
                    p.Z + (size_t)b * p.stride_z, s_val, s_idx);
}

#if SC_POOL_LDS_LINKAGE_MAX > 0
// ---- stream pool, short sessions: the distance matrix in LDS, one wavefront per session ----
// A session of n <= kPoolLdsLinkageMax rows (the fallback stage of a stream: n < L) is about
// 3 n strictly dependent steps on a matrix of a few KB.  k_ahc_nn_chain_pool pays a global-memory
// row read, two 1024-thread reductions and four barriers for each of them; here the matrix, the
// cluster sizes and the chain stay in LDS, a lane scans columns lane and lane + 64, and the
// argmin is a DPP reduction inside the wave.  The arithmetic and every tie rule are
// ahc_nn_chain_body's (method 2), so the merge list is the one k_pool_cosine_distance +
// k_ahc_nn_chain_pool write for the same GEMM output, bit for bit.

// (value, index) minimum over the wave, in every lane: smallest value, then smallest index.
// The order of the combining steps does not matter: the pairs are totally ordered.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void argmin_step(double& v, int& idx) {
  const double ov = dpp_f64<CTRL, ROW_MASK>(v, v);
  const int oi = dpp_i32<CTRL, ROW_MASK>(idx, idx);
  if (ov < v || (ov == v && oi < idx)) {
    v = ov;
    idx = oi;
  }
}
__device__ __forceinline__ void wave_argmin(double& v, int& idx) {
  argmin_step<kDppRowShr1, 0xf>(v, idx);
  argmin_step<kDppRowShr2, 0xf>(v, idx);
  argmin_step<kDppRowShr4, 0xf>(v, idx);
  argmin_step<kDppRowShr8, 0xf>(v, idx);
  argmin_step<kDppRowBcast15, 0xa>(v, idx);
  argmin_step<kDppRowBcast31, 0xc>(v, idx);
  const long long b = __double_as_longlong(v);  // lane 63 holds the wave's minimum
  const int lo = __builtin_amdgcn_readlane((int)b, 63);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
  v = __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
  idx = __builtin_amdgcn_readlane(idx, 63);
}

// The whole linkage of one problem of 2 <= n <= kPoolLdsLinkageMax rows on the calling wavefront
// (a 64-thread workgroup): c the GEMM's cosines (pitch ldc), Z the merge list, lds_d the
// workgroup's dynamic LDS (pool_linkage_lds_bytes(n) at least).  A problem lays its matrix out
// with its own odd pitch n | 1.  kVerdict: as ahc_nn_chain_body<true> -- Z is the two-double
// record {height, verdict}, lane 0 writes it (vector stores), the first height >= threshold
// ends the work.
template <bool kVerdict>
__device__ __forceinline__ void linkage_lds_body(const double* __restrict__ c, int ldc, int n,
                                                 double* __restrict__ Z, double* lds_d,
                                                 double threshold = 0.0) {
  const int lane = threadIdx.x;
  double top = -__builtin_huge_val();  // (kVerdict) the largest height so far
  const int pitch = n | 1;  // odd: a column walk touches every bank pair once
  double* D = lds_d;                                   // n x pitch
  int* size = reinterpret_cast<int*>(D + n * pitch);   // n
  int* chain = size + n;                               // n
  const double inf = __builtin_huge_val();
  {  // the GEMM's cosines -> distances (k_pool_cosine_distance's expression)
    for (int e = lane; e < n * n; e += 64) {
      const int i = e / n, j = e - i * n;
      D[i * pitch + j] = cosine_distance_value(c[(size_t)i * ldc + j], i == j);
    }
  }
  const int i0 = lane, i1 = lane + 64;  // the two columns of this lane
  if (i0 < n) size[i0] = 1;
  if (i1 < n) size[i1] = 1;
  __syncthreads();
  int chain_len = 0;
  for (int k = 0; k < n - 1; ++k) {
    if (chain_len == 0) {  // first slot that is still a cluster
      int f = 0x7fffffff;
      if (i1 < n && size[i1] > 0) f = i1;
      if (i0 < n && size[i0] > 0) f = i0;
      double fv = (double)f;
      wave_argmin(fv, f);
      if (lane == 0) chain[0] = f;
      chain_len = 1;
      __syncthreads();
    }
    int x, y;
    double cur;
    while (true) {
      x = chain[chain_len - 1];
      const int y0 = chain_len > 1 ? chain[chain_len - 2] : -1;
      const double* row = D + x * pitch;
      cur = y0 >= 0 ? row[y0] : inf;
      double best = inf;
      int besti = 0x7fffffff;
      if (i0 < n && size[i0] > 0 && i0 != x) {
        const double v = row[i0];
        if (v < best) {
          best = v;
          besti = i0;
        }
      }
      if (i1 < n && size[i1] > 0 && i1 != x) {
        const double v = row[i1];
        if (v < best) {
          best = v;
          besti = i1;
        }
      }
      wave_argmin(best, besti);
      y = y0;
      if (best < cur) {
        cur = best;
        y = besti;
      }
      if (chain_len > 1 && y == y0) break;
      if (lane == 0) chain[chain_len] = y;
      ++chain_len;
      __syncthreads();
    }
    chain_len -= 2;
    if (x > y) {
      const int t = x;
      x = y;
      y = t;
    }
    const int nx = size[x], ny = size[y];
    __syncthreads();  // every lane has read the sizes
    if constexpr (kVerdict) {
      if (cur >= threshold) {  // (cur is the same value in every lane: the wavefront leaves)
        if (lane == 0) {
          Z[0] = cur;
          Z[1] = 0.0;
        }
        return;
      }
      top = cur > top ? cur : top;
    }
    if (lane == 0) {
      if constexpr (!kVerdict) {
        Z[(size_t)k * 4 + 0] = (double)x;
        Z[(size_t)k * 4 + 1] = (double)y;
        Z[(size_t)k * 4 + 2] = cur;
        Z[(size_t)k * 4 + 3] = (double)(nx + ny);
      }
      size[x] = 0;
      size[y] = nx + ny;
    }
    const double* rx = D + x * pitch;
    double* ry = D + y * pitch;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      if (i >= n || i == x || i == y) continue;
      if (size[i] <= 0) continue;  // x and y are excluded above, the rest is unchanged
      const double dx = rx[i], dy = ry[i];
      const double nv = ((double)nx * dx + (double)ny * dy) / (double)(nx + ny);
      ry[i] = nv;
      D[i * pitch + y] = nv;
    }
    __syncthreads();
  }
  if constexpr (kVerdict) {
    if (lane == 0) {
      Z[0] = top;
      Z[1] = 1.0;
    }
  }
}

// Workgroup blockIdx.x works on position first + blockIdx.x of the launch's lists.  The dynamic
// LDS is sized for the largest session of the launch (pool_linkage_lds_bytes).
__global__ __launch_bounds__(64) void k_pool_linkage_lds(const PoolSlabs p,
                                                         const int* __restrict__ slots,
                                                         const int* __restrict__ rows,
                                                         int first) {
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  const int b = first + blockIdx.x;
  const int n = rows[b];
  if (n < 2 || n > kPoolLdsLinkageMax) return;
  linkage_lds_body<false>(p.D + (size_t)slots[b] * p.stride_d, p.ldd, n, p.Z + (size_t)b * p.stride_z,
                   lds_d);
}

// ... and on member first + blockIdx.x of a batch table (sc_batch_ahc)
__global__ __launch_bounds__(64) void k_batch_linkage_lds(const AhcBatchItem* __restrict__ table,
                                                          int first) {
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  const AhcBatchItem& it = table[first + blockIdx.x];
  const int n = it.n;
  if (n < 2 || n > kPoolLdsLinkageMax || *it.bad != 0) return;
  linkage_lds_body<false>(it.D, it.ld, n, it.Z, lds_d);
}

// ... and its verdict form: it.Z is the member's record {height, verdict}
__global__ __launch_bounds__(64) void k_batch_linkage_lds_verdict(
    const AhcBatchItem* __restrict__ table, int first, double threshold) {
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  const AhcBatchItem& it = table[first + blockIdx.x];
  const int n = it.n;
  if (n < 2 || n > kPoolLdsLinkageMax || *it.bad != 0) return;
  linkage_lds_body<true>(it.D, it.ld, n, it.Z, lds_d, threshold);
}
#endif  // SC_POOL_LDS_LINKAGE_MAX > 0

// utils.get_cluster_centroids: out[c][f] = mean over members (rows in index order, the
// order np.mean(axis=0) adds them) of X[i][f]
__device__ __forceinline__ double cluster_centroid_value(const double* __restrict__ X, int ldx,
                                                         int n, const int* __restrict__ labels,
                                                         int c, int f) {
  double acc = 0.0;
  int count = 0;
  for (int i = 0; i < n; ++i) {
    if (labels[i] == c) {
      acc += X[(size_t)i * ldx + f];
      ++count;
    }
  }
  return acc / (double)count;  // empty cluster: 0 / 0 = NaN, as np.mean
}

__global__ __launch_bounds__(256) void k_pool_centroids(const PoolSlabs p,
                                                        const int* __restrict__ slots,
                                                        const int* __restrict__ rows) {
  const int z = blockIdx.z;
  const int c = blockIdx.y;
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= p.d) return;
  const int slot = slots[z];
  p.cent[(size_t)slot * p.stride_c + (size_t)c * p.d + f] = cluster_centroid_value(
      p.X + (size_t)slot * p.stride_x, p.ldx, rows[z], p.labels + (size_t)z * p.stride_n, c, f);
}

__global__ __launch_bounds__(256) void k_cluster_centroids(const double* __restrict__ X, int ldx,
                                                           int n, int d,
                                                           const int* __restrict__ labels,
                                                           double* __restrict__ out) {
  const int c = blockIdx.y;
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= d) return;
  out[(size_t)c * d + f] = cluster_centroid_value(X, ldx, n, labels, c, f);
}

// The same means for every member of a batch from a CSR of its rows grouped by cluster (rows
// ascending inside a cluster): an output adds its own rows only, in index order, from 0.0 --
// cluster_centroid_value's bits without its scan of all n labels.  blockIdx.y = member, a
// thread per (cluster, feature).
__global__ __launch_bounds__(256) void k_batch_centroids(const AhcBatchItem* __restrict__ table,
                                                         int first) {
  const AhcBatchItem& it = table[first + blockIdx.y];
  if (it.cent == nullptr) return;
  const int* __restrict__ csr = it.csr;
  const int k = csr[0], d = it.d;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= k * d) return;
  const int c = t / d, f = t - c * d;
  const int* __restrict__ rows = csr + it.kcap + 2;
  const int begin = csr[1 + c], end = csr[2 + c];
  double acc = 0.0;
  for (int r = begin; r < end; ++r) acc += it.X[(size_t)rows[r] * it.ldx + f];
  it.cent[(size_t)c * d + f] = acc / (double)(end - begin);  // empty: 0 / 0 = NaN, as np.mean
}

void launch_cosine_distance(hipStream_t s, double* c, int n, int ld) {
  hipLaunchKernelGGL(k_cosine_distance, dim3((n + 255) / 256, n), dim3(256), 0, s, c, n, ld);
}
void launch_ahc_nn_chain(hipStream_t s, double* D, int ld, int n, int method, int* size,
                         int* chain, double* Z, const int* bad) {
  hipLaunchKernelGGL(k_ahc_nn_chain, dim3(1), dim3(kAhcThreads), 0, s, D, ld, n, method, size,
                     chain, Z, bad);
}
constexpr int kBatchGridY = 32768;  // members per launch where the member is blockIdx.y
void launch_batch_cosine_distance(hipStream_t s, const AhcBatchItem* table, int first, int count,
                                  int max_rows) {
  // 64 workgroups walk the rows of a member: enough to fill the device with a few members,
  // and a batch of hundreds launches no workgroup that finds nothing to do
  for (int at = 0; at < count; at += kBatchGridY)
    hipLaunchKernelGGL(k_batch_cosine_distance,
                       dim3(std::min(max_rows, 64), std::min(kBatchGridY, count - at)), dim3(256),
                       0, s, table, first + at);
}
void launch_batch_nn_chain(hipStream_t s, const AhcBatchItem* table, int first, int count) {
  hipLaunchKernelGGL(k_ahc_nn_chain_batch, dim3(count), dim3(kAhcThreads), 0, s, table, first);
}
void launch_batch_nn_chain_verdict(hipStream_t s, const AhcBatchItem* table, int first, int count,
                                   double threshold) {
  hipLaunchKernelGGL(k_ahc_nn_chain_verdict, dim3(count), dim3(kAhcThreads), 0, s, table, first,
                     threshold);
}
void launch_batch_centroids(hipStream_t s, const AhcBatchItem* table, int first, int count,
                            int max_outputs) {
  for (int at = 0; at < count; at += kBatchGridY)
    hipLaunchKernelGGL(k_batch_centroids,
                       dim3((max_outputs + 255) / 256, std::min(kBatchGridY, count - at)),
                       dim3(256), 0, s, table, first + at);
}
void launch_cluster_centroids(hipStream_t s, const double* X, int ldx, int n, int d,
                              const int* labels, int k, double* out) {
  hipLaunchKernelGGL(k_cluster_centroids, dim3((d + 255) / 256, k), dim3(256), 0, s, X, ldx, n,
                     d, labels, out);
}
void launch_pool_cosine_distance(hipStream_t s, const PoolSlabs& p, const int* slots,
                                 const int* rows, int count, int max_rows) {
  hipLaunchKernelGGL(k_pool_cosine_distance, dim3((max_rows + 255) / 256, max_rows, count),
                     dim3(256), 0, s, p, slots, rows);
}
void launch_pool_nn_chain(hipStream_t s, const PoolSlabs& p, const int* slots, const int* rows,
                          int count, int method) {
  hipLaunchKernelGGL(k_ahc_nn_chain_pool, dim3(count), dim3(kAhcThreads), 0, s, p, slots, rows,
                     method);
}
#if SC_POOL_LDS_LINKAGE_MAX > 0
static_assert(kPoolLdsLinkageMax <= 128, "k_pool_linkage_lds: a lane scans two columns");
static size_t pool_linkage_lds_bytes(int n) {
  return (size_t)n * (n | 1) * sizeof(double) + 2 * (size_t)n * sizeof(int);
}
void launch_pool_linkage_lds(hipStream_t s, const PoolSlabs& p, const int* slots, const int* rows,
                             int first, int count, int max_rows) {
  // 128 rows: 128 * 129 * 8 B + 1 KB = 130 KB of the CU's 160 KB
  SC_OPT_IN_LDS(k_pool_linkage_lds, pool_linkage_lds_bytes(kPoolLdsLinkageMax));
  hipLaunchKernelGGL(k_pool_linkage_lds, dim3(count), dim3(64),
                     pool_linkage_lds_bytes(std::min(max_rows, kPoolLdsLinkageMax)), s, p, slots,
                     rows, first);
}
void launch_batch_linkage_lds(hipStream_t s, const AhcBatchItem* table, int first, int count,
                              int max_rows) {
  SC_OPT_IN_LDS(k_batch_linkage_lds, pool_linkage_lds_bytes(kPoolLdsLinkageMax));
  hipLaunchKernelGGL(k_batch_linkage_lds, dim3(count), dim3(64),
                     pool_linkage_lds_bytes(std::min(max_rows, kPoolLdsLinkageMax)), s, table,
                     first);
}
void launch_batch_linkage_lds_verdict(hipStream_t s, const AhcBatchItem* table, int first,
                                      int count, int max_rows, double threshold) {
  SC_OPT_IN_LDS(k_batch_linkage_lds_verdict, pool_linkage_lds_bytes(kPoolLdsLinkageMax));
  hipLaunchKernelGGL(k_batch_linkage_lds_verdict, dim3(count), dim3(64),
                     pool_linkage_lds_bytes(std::min(max_rows, kPoolLdsLinkageMax)), s, table,
                     first, threshold);
}
#endif
void launch_pool_centroids(hipStream_t s, const PoolSlabs& p, const int* slots, const int* rows,
                           int count, int k) {
  hipLaunchKernelGGL(k_pool_centroids, dim3((p.d + 255) / 256, k, count), dim3(256), 0, s, p,
                     slots, rows);
}

}  // namespace sc
