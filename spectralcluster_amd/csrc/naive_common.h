// The arithmetic of the naive online clusterer (naive_clusterer.py:13-22), shared by
// k_naive_cluster (fallback.hip: one utterance, continuing a state) and k_naive_cluster_batch
// (naive_batch.hip: a workgroup per utterance of a wave, from the empty state), so that the two
// give the same bits: thread t of 256 sums the features f = t, t + 256, ...; a 64-lane xor
// butterfly (1, 2, ... 32) adds the lanes of a wavefront; the four wavefronts combine as
// (s0 + s1) + (s2 + s3).
#ifndef SPECTRALCLUSTER_AMD_NAIVE_COMMON_H_
#define SPECTRALCLUSTER_AMD_NAIVE_COMMON_H_

#include <hip/hip_runtime.h>

namespace sc {

// sum over the 256 threads of a workgroup, in every thread; s_red: 4 doubles of LDS
__device__ __forceinline__ double block_sum_256(double v, double* s_red) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[wave] = v;
  __syncthreads();
  return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// ||e||: every thread's result
__device__ __forceinline__ double naive_norm(const double* __restrict__ e, int d, double* s_red) {
  double ee = 0.0;
  for (int f = threadIdx.x; f < d; f += 256) ee += e[f] * e[f];
  return sqrt(block_sum_256(ee, s_red));
}

// NaiveCentroid.cosine (:19-22) of centroid cv and row e of norm enorm
__device__ __forceinline__ double naive_cosine(const double* cv, const double* __restrict__ e,
                                               int d, double enorm, double* s_red) {
  double dot = 0.0, cc = 0.0;
  for (int f = threadIdx.x; f < d; f += 256) {
    dot += cv[f] * e[f];
    cc += cv[f] * cv[f];
  }
  dot = block_sum_256(dot, s_red);
  cc = block_sum_256(cc, s_red);
  return dot / (sqrt(cc) * enorm);
}

// NaiveCentroid.merge (:13-17): the running mean of cnt members takes e in
__device__ __forceinline__ void naive_merge(double* cv, const double* __restrict__ e, int d,
                                            double cnt) {
  for (int f = threadIdx.x; f < d; f += 256) cv[f] = (cv[f] * cnt + e[f]) / (cnt + 1.0);
}

}  // namespace sc

#endif  // SPECTRALCLUSTER_AMD_NAIVE_COMMON_H_
