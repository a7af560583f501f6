// K1/K2: run_kmeans with custom_dist="cosine" (reference
// custom_distance_kmeans.py:13-141) on the (n, k) spectral embedding; any k (k <= 64 with the
// per-cluster arrays in LDS, more through a global workspace: k_kmeans<true>).
//
//   seeds   = sklearn 1.7.2 KMeans(init="k-means++", max_iter=1, random_state=0,
//             n_init="auto").fit(E).cluster_centers_   (:39-43), restated:
//             centre E, k-means++ with RandomState(0) doubles (host MT19937,
//             passed in `rnd`), one Euclidean Lloyd step, add the mean back;
//   loop    = CustomKMeans.predict (:85-141): cosine cdist, argmin, mean
//             distance stop rule, centroid means incl. the `.any()`-on-indices
//             quirk (:137-138).
//
// The whole stage is ONE single-workgroup kernel (1024 threads), whatever k and the metric: the
// form every metric but cosine runs, and cosine beyond what the chain of kmeans_chain.hip takes
// (more than 32 clusters, or n above its limit).  The per-metric arithmetic and the pairwise
// row mean are in kmeans_common.h, shared with kmeans_general.hip.  Compiled with
// -ffp-contract=off.
#include <cstdlib>

#include "kmeans_common.h"
#include "sc_internal.h"

namespace sc {

constexpr int KT = 1024;  // threads
constexpr int KW = KT / 64;

// E is stored COLUMN-MAJOR on the device (one eigenvector = one contiguous run of
// n doubles, ET[j * lde + r]): every per-row loop below then reads 512 contiguous
// bytes per wave instruction instead of 64 scattered lines.
__global__ __launch_bounds__(256) void k_row_renorm(double* __restrict__ ET, int lde,
                                                    int n, int k) {
  // spectral_clusterer.py:301-305: rows of the spectral embedding to unit L2 norm
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  double s = 0.0;
  for (int j = 0; j < k; ++j) s += ET[(size_t)j * lde + r] * ET[(size_t)j * lde + r];
  const double nrm = sqrt(s);
  for (int j = 0; j < k; ++j) ET[(size_t)j * lde + r] = ET[(size_t)j * lde + r] / nrm;
}

// (n, k) row-major  ->  column-major with leading dimension ldt (stage API input, any width)
__global__ __launch_bounds__(256) void k_to_colmajor(const double* __restrict__ src, int n,
                                                     int k, double* __restrict__ dst, int ldt) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)n * k) return;
  const size_t r = e / k, j = e - r * k;
  dst[j * ldt + r] = src[e];
}

// Per-cluster means of the member rows, data column-major (data[j * ld + r]).
// Each thread owns rows tid, tid + KT, ...; for one cluster it adds up only its own
// member rows, then the k partial sums are reduced wave -> LDS -> fixed-order total
// (deterministic).
//   mode 0 (Lloyd, centred data):  mean of members + mean[j]; empty cluster keeps seed
//   mode 1 (custom-distance loop): mean of members iff some member index > 0
__device__ __forceinline__ void cluster_means(const double* __restrict__ data, int ld,
                                              int n, int k, const int* __restrict__ lab,
                                              double* cent, const double* mean, int mode,
                                              double* wpart /* 2 * KW * kst */, int kst,
                                              int* counts, int* nzcounts) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int c = 0; c < k; ++c) {
    int cnt = 0, nz = 0;
    double* wp = wpart + (c & 1) * (KW * kst);  // double-buffered by parity
    for (int j0 = 0; j0 < k; j0 += 8) {
      double acc[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] = 0.0;
#pragma unroll 4
      for (int r = tid; r < n; r += KT) {
        if (lab[r] == c) {
          if (j0 == 0) { ++cnt; nz += r > 0; }
#pragma unroll
          for (int q = 0; q < 8; ++q)
            if (j0 + q < k) acc[q] += data[(size_t)(j0 + q) * ld + r];
        }
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const double v = wave_sum(acc[q]);
        if (lane == 0 && j0 + q < k) wp[wave * kst + j0 + q] = v;
      }
    }
    cnt = wave_sum(cnt);
    nz = wave_sum(nz);
    if (lane == 0) {
      atomicAdd(&counts[c], cnt);   // integer: order-independent
      atomicAdd(&nzcounts[c], nz);
    }
    __syncthreads();
    // (the counters were built by atomics, which execute in L2: in the large-k form they live
    //  in global memory, and a plain load could be served from this CU's L1 with the zero that
    //  was stored before the atomics -- read them the way they were written)
    const int count_c = __hip_atomic_load(&counts[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int nz_c = __hip_atomic_load(&nzcounts[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int t = tid; t < k; t += KT) {  // (k <= 64: one trip; the large-k form strides)
      double tot = 0.0;
#pragma unroll
      for (int w = 0; w < KW; ++w) tot += wp[w * kst + t];
      const int q = c * k + t;
      if (mode == 0) {
        const double v = count_c > 0 ? tot / (double)count_c : cent[q];
        cent[q] = v + mean[t];
      } else if (nz_c > 0) {
        cent[q] = tot / (double)count_c;
      }
    }
  }
  __syncthreads();
}

// BIG: more than kMaxVectors clusters (the reference has no limit: custom_distance_kmeans.py:
// 13-52 takes any k) -- the per-cluster arrays live in a global workspace `gws` / `gwi` instead
// of LDS (one workgroup: its own stores are visible to it behind __syncthreads), everything else
// is the same code.  gws: k (2 + 8 + 2 KW) + k^2 doubles, gwi: 3 k ints.
// (16 k-means++ trial slots in the BIG form: sklearn draws 2 + int(log k) candidates per centre,
//  more than 8 from k = 1097 on; 16 cover every k a 32-bit sample count allows)
size_t kmeans_big_workspace_doubles(int k) { return (size_t)k * (2 + 16 + 2 * KW) + (size_t)k * k; }
template <bool BIG>
__global__ __launch_bounds__(KT) void k_kmeans(
    const double* __restrict__ ET, int lde, int n, int k, int max_iter,
    int first_center, int trials, double* __restrict__ XcT, double* __restrict__ xsq,
    double* __restrict__ closest, double* __restrict__ cand_d,
    double* __restrict__ enorm, const double* __restrict__ rnd,
    double* __restrict__ cent_out, int* __restrict__ labels32,
    long long* __restrict__ labels64, int* __restrict__ info, int metric,
    double* __restrict__ gws, int* __restrict__ gwi, int* __restrict__ seeds_out) {
  constexpr int KL = BIG ? 1 : kMaxVectors;  // LDS footprint of the per-cluster arrays
  __shared__ double sm[KW];
  __shared__ double s_mean[KL];
  __shared__ double s_cent[KL * KL];   // k x k, stride k
  __shared__ double s_cnorm[KL];
  constexpr int TS = BIG ? 16 : 8;              // k-means++ trial slots (2 + int(log k) used)
  __shared__ double s_candrow[8 * KL];          // candidate rows, stride k
  __shared__ double candsq[TS];
  __shared__ double scan[KT];
  __shared__ double pots[TS];
  __shared__ double rvals[TS];
  __shared__ int cand[TS];
  __shared__ int s_seeds[KL];
  __shared__ int s_counts[KL];
  __shared__ int s_nzcounts[KL];
  __shared__ double s_wpart[2 * KW * KL];
  const int kst = BIG ? k : kMaxVectors;  // stride of the per-wave partial sums
  double* mean = BIG ? gws : s_mean;
  double* cnorm = BIG ? gws + k : s_cnorm;
  double* candrow = BIG ? gws + 2 * (size_t)k : s_candrow;
  double* wpart = BIG ? gws + (2 + TS) * (size_t)k : s_wpart;
  double* cent = BIG ? gws + (size_t)k * (2 + TS + 2 * KW) : s_cent;
  int* seeds = BIG ? gwi : s_seeds;
  int* counts = BIG ? gwi + k : s_counts;
  int* nzcounts = BIG ? gwi + 2 * (size_t)k : s_nzcounts;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const long long t_start = wall_clock64();  // 100 MHz; phase times go to info[1..4]

  // ---- column means (numpy mean(axis=0)), centred copy, row norms ---------------
  for (int j = wave; j < k; j += KW) {
    double s = 0.0;
    for (int r = lane; r < n; r += 64) s += ET[(size_t)j * lde + r];
    s = wave_sum(s);
    if (lane == 0) mean[j] = s / (double)n;
  }
  __syncthreads();
  for (int r = tid; r < n; r += KT) {
    double s = 0.0, en = 0.0;
    for (int j = 0; j < k; ++j) {
      const double e = ET[(size_t)j * lde + r];
      const double v = e - mean[j];
      XcT[(size_t)j * n + r] = v;
      s += v * v;
      en += e * e;
    }
    xsq[r] = s;
    enorm[r] = sqrt(en);
  }
  __syncthreads();

  // ---- k-means++ (sklearn _kmeans_plusplus, unit sample weights) --------------
  if (tid == 0) info[1] = (int)(wall_clock64() - t_start);
  if (tid == 0) seeds[0] = first_center;
  for (int t = tid; t < k; t += KT) candrow[t] = XcT[(size_t)t * n + first_center];
  __syncthreads();
  double pot;
  {
    const double csq = xsq[first_center];
    double part = 0.0;
    for (int r = tid; r < n; r += KT) {
      double dot = 0.0;
      for (int j = 0; j < k; ++j) dot += candrow[j] * XcT[(size_t)j * n + r];
      double d = -2.0 * dot;
      d += csq;
      d += xsq[r];
      d = fmax(d, 0.0);
      closest[r] = d;
      part += d;
    }
    pot = block_sum<KW>(part, sm);
  }
  int rpos = 0;
  const int chunk = (n + KT - 1) / KT;
  for (int c = 1; c < k; ++c) {
    if (tid < trials) {
      rvals[tid] = rnd[rpos + tid] * pot;
      cand[tid] = n - 1;  // np.clip(candidate_ids, None, n - 1)
    }
    rpos += trials;
    // inclusive scan of per-thread chunk sums of `closest`
    const int beg = min(n, tid * chunk), end = min(n, beg + chunk);
    double mysum = 0.0;
    for (int r = beg; r < end; ++r) mysum += closest[r];
    {
      double v = mysum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl_up(v, o);
        if (lane >= o) v += u;
      }
      __syncthreads();
      if (lane == 63) sm[wave] = v;
      __syncthreads();
      double off = 0.0;
      for (int w = 0; w < wave; ++w) off += sm[w];
      scan[tid] = v + off;  // inclusive prefix over threads
    }
    __syncthreads();
    {
      const double excl = tid == 0 ? 0.0 : scan[tid - 1];
      const double incl = scan[tid];
      for (int t = 0; t < trials; ++t) {
        const double rv = rvals[t];
        // searchsorted(cumsum, rv, 'left'): first index with cumsum >= rv
        if (beg < end && (rv > excl || tid == 0) && rv <= incl) {
          double run = excl;
          int hit = end - 1;
          for (int r = beg; r < end - 1; ++r) {
            run += closest[r];
            if (run >= rv) { hit = r; break; }
          }
          atomicMin(&cand[t], hit);
        }
      }
    }
    __syncthreads();
    // candidate rows -> LDS, then ONE pass over the data for all trials
    for (int e = tid; e < trials * k; e += KT) {
      const int t = e / k, j = e - t * k;
      candrow[t * k + j] = XcT[(size_t)j * n + cand[t]];
    }
    if (tid < trials) candsq[tid] = xsq[cand[tid]];
    __syncthreads();
    double part[TS];
#pragma unroll
    for (int t = 0; t < TS; ++t) part[t] = 0.0;
#pragma unroll 4
    for (int r = tid; r < n; r += KT) {
      double dot[TS];
#pragma unroll
      for (int t = 0; t < TS; ++t) dot[t] = 0.0;
      for (int j = 0; j < k; ++j) {
        const double x = XcT[(size_t)j * n + r];
#pragma unroll
        for (int t = 0; t < TS; ++t)
          if (t < trials) dot[t] += candrow[t * k + j] * x;
      }
      const double xs = xsq[r], cl = closest[r];
#pragma unroll
      for (int t = 0; t < TS; ++t) {
        if (t < trials) {
          double d = -2.0 * dot[t];
          d += candsq[t];
          d += xs;
          d = fmax(d, 0.0);
          d = fmin(cl, d);
          cand_d[(size_t)t * n + r] = d;
          part[t] += d;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < TS; ++t) {
      if (t < trials) {  // uniform
        const double tot = block_sum<KW>(part[t], sm);
        if (tid == 0) pots[t] = tot;
      }
    }
    __syncthreads();
    int best = 0;
    for (int t = 1; t < trials; ++t)
      if (pots[t] < pots[best]) best = t;  // np.argmin: first minimum
    pot = pots[best];
#pragma unroll 4
    for (int r = tid; r < n; r += KT) closest[r] = cand_d[(size_t)best * n + r];
    if (tid == 0) seeds[c] = cand[best];
    __syncthreads();
  }

  // ---- one Euclidean Lloyd step on the centred data (max_iter = 1) -------------
  if (tid == 0) info[2] = (int)(wall_clock64() - t_start);
  for (int e = tid; e < k * k; e += KT) {
    const int c = e / k, j = e - c * k;
    cent[e] = XcT[(size_t)j * n + seeds[c]];
  }
  __syncthreads();
  for (int t = tid; t < k; t += KT) {
    double s = 0.0;
    for (int j = 0; j < k; ++j) s += cent[t * k + j] * cent[t * k + j];
    cnorm[t] = s;  // squared norms here
  }
  __syncthreads();
#pragma unroll 2
  for (int r = tid; r < n; r += KT) {
    int best = 0;
    double bd = INFINITY;
    for (int c0 = 0; c0 < k; c0 += 8) {
      double dot[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) dot[q] = 0.0;
      for (int j = 0; j < k; ++j) {
        const double x = XcT[(size_t)j * n + r];
#pragma unroll
        for (int q = 0; q < 8; ++q)
          if (c0 + q < k) dot[q] += x * cent[(c0 + q) * k + j];
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (c0 + q < k) {
          const double d = cnorm[c0 + q] - 2.0 * dot[q];
          if (d < bd) { bd = d; best = c0 + q; }
        }
      }
    }
    labels32[r] = best;
  }
  for (int t = tid; t < k; t += KT) { counts[t] = 0; nzcounts[t] = 0; }
  __syncthreads();
  // empty cluster: keeps its seed (sklearn relocates; unreachable from k-means++
  // seeds, each of which is its own nearest centre); best_centers += X_mean
  cluster_means(XcT, n, n, k, labels32, cent, mean, 0, wpart, kst, counts, nzcounts);

  // ---- CustomKMeans.predict (custom_distance_kmeans.py:118-141), scipy cdist metric --
  if (tid == 0) info[3] = (int)(wall_clock64() - t_start);
  double prev = 0.0;
  int it = 0;
  // (`correlation`: scipy's cosine distance on row-centred operands, the row means in numpy's
  //  summation order -- pw_mean, kmeans_common.h)
  for (;; ++it) {
    for (int t = tid; t < k; t += KT) {
      double s = 0.0;
      if (metric == kKmeansCorrelation) {
        const double mc = pw_mean([&](int j) { return cent[t * k + j]; }, k);
        for (int j = 0; j < k; ++j) s += (cent[t * k + j] - mc) * (cent[t * k + j] - mc);
        // (the centred centroid's mean rides in the wave-partial scratch: free at this point)
        wpart[t] = mc;
      } else {
        for (int j = 0; j < k; ++j) s += cent[t * k + j] * cent[t * k + j];
      }
      cnorm[t] = sqrt(s);
    }
    __syncthreads();
    double part = 0.0;
#pragma unroll 2
    for (int r = tid; r < n; r += KT) {
      int best = 0;
      double bd = INFINITY;
      double nu = enorm[r], mx = 0.0;
      if (metric == kKmeansCorrelation) {
        mx = pw_mean([&](int j) { return ET[(size_t)j * lde + r]; }, k);
        double s = 0.0;
        for (int j = 0; j < k; ++j) {
          const double e = ET[(size_t)j * lde + r] - mx;
          s += e * e;
        }
        nu = sqrt(s);
      }
      for (int c0 = 0; c0 < k; c0 += 8) {
        double dot[8], aux[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) dot[q] = aux[q] = 0.0;
        for (int j = 0; j < k; ++j) {
          double x = ET[(size_t)j * lde + r];
          if (metric == kKmeansCorrelation) x = x - mx;
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            if (c0 + q < k) {
              const double cmean = metric == kKmeansCorrelation ? wpart[c0 + q] : 0.0;
              metric_accumulate(metric, x, cent[(c0 + q) * k + j], cmean, dot[q], aux[q]);
            }
          }
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          if (c0 + q < k) {
            const double d = metric_finish(metric, dot[q], aux[q], nu, cnorm[c0 + q]);
            if (d < bd) { bd = d; best = c0 + q; }
          }
        }
      }
      labels32[r] = best;
      part += bd;
    }
    const double mean_d = block_sum<KW>(part, sm) / (double)n;
    // (:131-133)
    if ((mean_d <= prev && mean_d >= (1.0 - 0.001) * prev) || it == max_iter) break;
    prev = mean_d;
    for (int t = tid; t < k; t += KT) { counts[t] = 0; nzcounts[t] = 0; }
    __syncthreads();
    // centroid <- mean of members iff `.any()` of the member INDICES (:137-138)
    cluster_means(ET, lde, n, k, labels32, cent, mean, 1, wpart, kst, counts, nzcounts);
  }
  for (int r = tid; r < n; r += KT) labels64[r] = labels32[r];
  for (int e = tid; e < k * k; e += KT) cent_out[e] = cent[e];
  if (seeds_out)  // (the trace entry; production passes null)
    for (int t = tid; t < k; t += KT) seeds_out[t] = seeds[t];
  if (tid == 0) {
    info[0] = it + 1;
    info[4] = (int)(wall_clock64() - t_start);
  }
}

void launch_row_renorm(hipStream_t s, double* ET, int lde, int n, int k) {
  hipLaunchKernelGGL(k_row_renorm, dim3((n + 255) / 256), dim3(256), 0, s, ET, lde, n,
                     k);
}

void launch_to_colmajor(hipStream_t s, const double* src, int n, int k, double* dst,
                        int ldt) {
  const size_t nel = (size_t)n * k;
  hipLaunchKernelGGL(k_to_colmajor, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, s, src, n,
                     k, dst, ldt);
}

void launch_kmeans(hipStream_t s, const double* ET, int lde, int n, int k,
                   int max_iter, int first_center, int trials,
                   const KmeansWorkspace& ws, int metric, int* seeds_out) {
  if (k > kMaxVectors) {  // (this form's seeds are in ws.big_words already)
    hipLaunchKernelGGL(k_kmeans<true>, dim3(1), dim3(KT), 0, s, ET, lde, n, k, max_iter,
                       first_center, trials, ws.Xc, ws.xsq, ws.closest, ws.cand, ws.enorm, ws.rnd,
                       ws.centroids, ws.labels32, ws.labels64, ws.info, metric, ws.big,
                       ws.big_words, static_cast<int*>(nullptr));
    return;
  }
  hipLaunchKernelGGL(k_kmeans<false>, dim3(1), dim3(KT), 0, s, ET, lde, n, k, max_iter,
                     first_center, trials, ws.Xc, ws.xsq, ws.closest, ws.cand,
                     ws.enorm, ws.rnd, ws.centroids, ws.labels32, ws.labels64,
                     ws.info, metric, static_cast<double*>(nullptr), static_cast<int*>(nullptr),
                     seeds_out);
}

}  // namespace sc
