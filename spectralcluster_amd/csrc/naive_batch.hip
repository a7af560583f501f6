// The naive online clusterer for a whole wave of utterances (include/spectralcluster_amd.h
// sc_batch_naive_cluster, sc_batch_naive_check; host side batch_reduce.hip): the walk of
// k_naive_cluster (fallback.hip) from the empty state, one workgroup of 256 threads per member of
// a table of descriptors in device memory, so a wave of any sizes is ONE launch.
//   labels form   the full walk: labels, counts, centroids, n_clusters
//   verdict form  "does the walk end with one centroid?": the member's work ends at the row that
//                 would open a second centroid; one record {single, stopped_at}, one centroid of
//                 scratch, the count in a register
// The arithmetic is naive_common.h's, shared with k_naive_cluster: every cosine, every merge and
// so every threshold comparison gives that kernel's bits.
#include <hip/hip_runtime.h>

#include "naive_common.h"
#include "sc_internal.h"

namespace sc {

namespace {

// Is a row of the member zero or non-finite?  The rule (and the sum) of normalize_one_row
// (rowops.hip): a wavefront per row, accumulator w of lane l adds the elements 64 w + l + 256 i,
// each is reduced across the wave (32, 16, ... 1), then (s0 + s1) + (s2 + s3).
__device__ __forceinline__ bool member_has_bad_row(const NaiveBatchItem& it) {
  const int lane = threadIdx.x & 63;
  bool bad = false;
  for (int r = threadIdx.x >> 6; r < it.n; r += 4) {
    const double* x = it.X + (size_t)r * it.ldx;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < it.d; j0 += 256) {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int j = j0 + 64 * w + lane;
        if (j < it.d) acc[w] += x[j] * x[j];
      }
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[w] += __shfl_xor(acc[w], o);
    }
    const double norm = sqrt((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if (!(norm > 0.0 && isfinite(norm))) bad = true;
  }
  return bad;
}

}  // namespace

template <bool VERDICT>
__global__ __launch_bounds__(256) void k_naive_cluster_batch(
    const NaiveBatchItem* __restrict__ table, double threshold, double adapt_threshold) {
  __shared__ double s_red[4];
  const NaiveBatchItem it = table[blockIdx.x];
  const int tid = threadIdx.x;
  const int n = it.n, d = it.d;
  if (VERDICT && it.bad != nullptr) {
    if (member_has_bad_row(it) && (tid & 63) == 0) *it.bad = 1;  // (any wavefront may latch it)
  }
  double* centroids = it.cent;
  // first embedding: naive_clusterer.py:68-71
  for (int f = tid; f < d; f += 256) centroids[f] = it.X[f];
  if (!VERDICT && tid == 0) {
    it.counts[0] = 1;
    it.labels[0] = 0;
  }
  int k = 1;
  int count0 = 1;   // verdict form: the one centroid's count
  int stopped = n;  // verdict form: the row that would open a second centroid
  __syncthreads();
  for (int i = 1; i < n; ++i) {
    const double* e = it.X + (size_t)i * it.ldx;
    const double enorm = naive_norm(e, d, s_red);
    double best = -__builtin_huge_val();
    int label = 0;
    for (int c = 0; c < k; ++c) {
      const double sim = naive_cosine(centroids + (size_t)c * d, e, d, enorm, s_red);  // :19-22
      if (sim > best) {  // np.argmax: first maximum
        best = sim;
        label = c;
      }
    }
    // (best holds the same bits in every thread: the branches below are uniform)
    if (best < threshold) {  // new cluster, :77-80
      if (VERDICT) {
        stopped = i;
        break;
      }
      for (int f = tid; f < d; f += 256) centroids[(size_t)k * d + f] = e[f];
      if (tid == 0) {
        it.counts[k] = 1;
        it.labels[i] = k;
      }
      ++k;
    } else {
      if (best > adapt_threshold) {  // merge, :13-17
        const double cnt = VERDICT ? (double)count0 : (double)it.counts[label];
        naive_merge(centroids + (size_t)label * d, e, d, cnt);
        if (VERDICT) {
          ++count0;
        } else {
          __syncthreads();
          if (tid == 0) it.counts[label] += 1;
        }
      }
      if (!VERDICT && tid == 0) it.labels[i] = label;
    }
    if (!VERDICT) __syncthreads();  // (counts; a thread reads back only centroid values it wrote)
  }
  if (tid == 0) {
    if (VERDICT) {
      it.out[0] = stopped == n ? 1 : 0;
      it.out[1] = stopped;
    } else {
      it.out[0] = k;
    }
  }
}

void launch_naive_cluster_batch(hipStream_t s, const NaiveBatchItem* table, int count,
                                double threshold, double adapt_threshold, bool verdict) {
  if (count <= 0) return;
  if (verdict)
    hipLaunchKernelGGL(k_naive_cluster_batch<true>, dim3(count), dim3(256), 0, s, table, threshold,
                       adapt_threshold);
  else
    hipLaunchKernelGGL(k_naive_cluster_batch<false>, dim3(count), dim3(256), 0, s, table,
                       threshold, adapt_threshold);
}

}  // namespace sc
