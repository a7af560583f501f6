// Device-side arithmetic the k-means kernels share (kmeans.hip, kmeans_chain.hip,
// kmeans_general.hip): the wave and workgroup sums, numpy's pairwise row mean, and the scipy
// cdist metrics of the custom-distance loop.  One statement of each, so a fix reaches every
// kernel.  The library is compiled with -ffp-contract=off: an expression rounds the same
// inside these inline functions as it did written out in a kernel.
#ifndef SPECTRALCLUSTER_AMD_KMEANS_COMMON_H_
#define SPECTRALCLUSTER_AMD_KMEANS_COMMON_H_

#include <hip/hip_runtime.h>

#include "sc_internal.h"

namespace sc {

// butterfly sum over the 64 lanes, same value in every lane; a fixed order
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// sum over a workgroup of WAVES waves, same value in every thread: the wave sums folded in
// wave order.  sm: WAVES doubles
template <int WAVES>
__device__ __forceinline__ double block_sum(double v, double* sm) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) t += sm[w];
  return t;
}

// Mean of at(0) .. at(m - 1) in numpy's summation order (pairwise_sum, numpy/core/src/umath/
// loops_utils.h): fewer than 8 elements one by one; up to PW_BLOCKSIZE = 128 eight running sums
// folded as a tree, then the tail; longer runs split at cnt / 2 rounded down to a multiple of 8
// and the halves' sums added, recursively -- an explicit stack here, depth <= log2(m / 128) + 1.
// scipy's `correlation` centres both operands by this mean (scipy 1.15 spatial/distance.py
// _correlation_cdist_wrap: X - X.mean(axis=1, keepdims=True)).
template <typename At>
__device__ double pw_leaf(At at, int lo, int cnt) {
  double s;
  if (cnt < 8) {
    s = 0.0;
    for (int j = 0; j < cnt; ++j) s += at(lo + j);
  } else {
    double a8[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) a8[q] = at(lo + q);
    int j = 8;
    for (; j < cnt - (cnt % 8); j += 8) {
#pragma unroll
      for (int q = 0; q < 8; ++q) a8[q] += at(lo + j + q);
    }
    s = ((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7]));
    for (; j < cnt; ++j) s += at(lo + j);
  }
  return s;
}
template <typename At>
__device__ double pw_mean(At at, int m) {
  if (m <= 128) return pw_leaf(at, 0, m) / (double)m;
  int lo[32], cnt[32], stage[32];
  double left[32];
  int sp = 0;
  lo[0] = 0;
  cnt[0] = m;
  stage[0] = 0;
  double ret = 0.0;
  while (sp >= 0) {
    if (stage[sp] == 0) {
      if (cnt[sp] <= 128) {
        ret = pw_leaf(at, lo[sp], cnt[sp]);
        --sp;
        continue;
      }
      int half = cnt[sp] / 2;
      half -= half % 8;
      stage[sp] = 1;
      lo[sp + 1] = lo[sp];
      cnt[sp + 1] = half;
      stage[sp + 1] = 0;
      ++sp;
    } else if (stage[sp] == 1) {
      left[sp] = ret;
      int half = cnt[sp] / 2;
      half -= half % 8;
      stage[sp] = 2;
      lo[sp + 1] = lo[sp] + half;
      cnt[sp + 1] = cnt[sp] - half;
      stage[sp + 1] = 0;
      ++sp;
    } else {
      ret = left[sp] + ret;
      --sp;
    }
  }
  return ret / (double)m;
}

// One column of scipy's cdist between a row and a centroid: x and cv are the two elements,
// acc / aux the running sums of the pair.  correlation: x arrives with its row mean already
// subtracted, cmean is the centroid's (unused by the other metrics).  `metric` may be a
// compile-time constant, in which case the branches fold.
__device__ __forceinline__ void metric_accumulate(int metric, double x, double cv, double cmean,
                                                  double& acc, double& aux) {
  if (metric == kKmeansCosine) {
    acc += x * cv;
  } else if (metric == kKmeansCorrelation) {
    acc += x * (cv - cmean);
  } else if (metric == kKmeansCityblock) {
    acc += fabs(x - cv);
  } else if (metric == kKmeansChebyshev) {
    acc = fmax(acc, fabs(x - cv));
  } else if (metric == kKmeansBraycurtis) {  // sum |u - v| / sum |u + v|
    acc += fabs(x - cv);
    aux += fabs(x + cv);
  } else if (metric == kKmeansCanberra) {  // sum |u - v| / (|u| + |v|), 0 / 0 = 0
    const double den = fabs(x) + fabs(cv);
    if (den > 0.0) acc += fabs(x - cv) / den;
  } else {  // (squared) Euclidean
    acc += (x - cv) * (x - cv);
  }
}
// ... and the distance from the finished sums.  nu / cnorm: the norms of the row and of the
// centroid (of the centred ones for correlation); only cosine and correlation read them.
__device__ __forceinline__ double metric_finish(int metric, double acc, double aux, double nu,
                                                double cnorm) {
  if (metric == kKmeansCosine || metric == kKmeansCorrelation) {
    double cosine = acc / (nu * cnorm);
    if (fabs(cosine) > 1.0) cosine = copysign(1.0, cosine);
    return 1.0 - cosine;
  }
  if (metric == kKmeansBraycurtis) return acc / aux;
  return metric == kKmeansEuclidean ? sqrt(acc) : acc;
}

}  // namespace sc

#endif  // SPECTRALCLUSTER_AMD_KMEANS_COMMON_H_
