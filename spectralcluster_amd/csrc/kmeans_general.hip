// K1 general form: run_kmeans / CustomKMeans.predict (reference custom_distance_kmeans.py:13-52,
// :85-141) on an (n, dim) input whose width is independent of the cluster count k.
//
//   seeds   = sklearn 1.7.2 KMeans(init="k-means++", max_iter=1, random_state=0,
//             n_init="auto").fit(X).cluster_centers_, restated as in kmeans.hip: centre X by its
//             column means, k-means++ with 2 + int(log k) trials per centre on sklearn's
//             -2 x.c + |x|^2 + |c|^2 (clamped at 0) with the host MT19937 RandomState(0)
//             doubles, one Euclidean Lloyd step (an empty cluster keeps its seed), add the mean
//             back.  Skipped when the caller supplies the initial centroids;
//   loop    = CustomKMeans.predict: scipy cdist per metric, first-minimum argmin, mean
//             distance stop rule with the caller's tol, centroid means with the `.any()`-on-
//             indices quirk (:137-138).
//
// Layout: X column-major (X[j * ld + r], ld = round_up(n, 16)), centroids row-major (k, dim).
// Every pass over X is a grid:
//   * row passes (k-means++ candidate distances, the Lloyd E-step, each loop assignment): one
//     row per thread, KG_ROWS rows per workgroup, centroids staged through LDS eight at a time in
//     chunks of KG_JC columns (8 * KG_JC * 8 B = 16 KiB), so any k * dim works; per-workgroup
//     partial sums go to global memory and the next launch adds them in workgroup order;
//   * centroid update: one workgroup per column of X, eight clusters per sweep over the labels;
//   * the serial steps (k-means++ cumsum + searchsorted, argmin of the trial pots, the stop
//     rule) are short single-workgroup launches.
// Every sum is taken in a fixed order, so two calls give bit-identical results.  The library
// is compiled with -ffp-contract=off; the per-metric arithmetic restates kmeans.hip's loop.
#include <algorithm>
#include <cmath>
#include <vector>

#include "handle.h"

namespace sc {
namespace {

constexpr int KG_ROWS = 64;   // rows (threads) per workgroup of the row passes: one wave
constexpr int KG_JC = 256;    // centroid columns per LDS chunk
constexpr int KG_TS = 16;     // k-means++ trial slots (2 + int(log k) used)
constexpr int KG_UT = 256;    // threads of the column-parallel update / column means
constexpr int KG_ST = 1024;   // threads of the k-means++ select launch
constexpr int KG_ITERS = 4;   // loop iterations enqueued per host synchronisation

enum { kModePP = 100, kModeLloyd = 101 };
// int words: done, iterations, best trial of the last k-means++ pass
enum { kWDone = 0, kWIters = 1, kWBest = 2, kWords = 4 };
// double scalars: pot, prev mean distance
enum { kSPot = 0, kSPrev = 1, kScalars = 4 };

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// numpy's pairwise sum (numpy/core/src/umath/loops_utils.h), as kmeans.hip restates it for
// scipy's correlation row means: fewer than 8 elements one by one; up to 128 eight running sums
// folded as a tree, then the tail; longer runs split at cnt / 2 rounded down to a multiple of 8
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

// (n, dim) row-major -> column-major with leading dimension ld
__global__ __launch_bounds__(256) void k_g_colmajor(const double* __restrict__ src, int n,
                                                    int dim, double* __restrict__ dst,
                                                    int ld) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)n * dim) return;
  const size_t r = e / dim, j = e - r * dim;
  dst[j * ld + r] = src[e];
}

// column means: one workgroup per column, thread-strided partials folded in a fixed order
__global__ __launch_bounds__(KG_UT) void k_g_colmean(const double* __restrict__ X, int ld,
                                                     int n, double* __restrict__ mean) {
  __shared__ double sm[KG_UT / 64];
  const int j = blockIdx.x, tid = threadIdx.x;
  double s = 0.0;
  for (int r = tid; r < n; r += KG_UT) s += X[(size_t)j * ld + r];
  s = wave_sum(s);
  if ((tid & 63) == 0) sm[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < KG_UT / 64; ++w) t += sm[w];
    mean[j] = t / (double)n;
  }
}

// per-row constants: |x - mean|^2 (k-means++), |x| (cosine), the row mean and the centred norm
// (correlation)
__global__ __launch_bounds__(KG_ROWS) void k_g_rowstats(
    const double* __restrict__ X, int ld, int n, int dim, const double* __restrict__ mean,
    double* __restrict__ xsq, double* __restrict__ enorm, double* __restrict__ rmx,
    double* __restrict__ cnu, int correlation) {
  const int r = blockIdx.x * KG_ROWS + threadIdx.x;
  if (r >= n) return;
  double s = 0.0, en = 0.0;
  for (int j = 0; j < dim; ++j) {
    const double e = X[(size_t)j * ld + r];
    const double v = e - mean[j];
    s += v * v;
    en += e * e;
  }
  xsq[r] = s;
  enorm[r] = sqrt(en);
  if (correlation) {
    const double mx = pw_mean([&](int j) { return X[(size_t)j * ld + r]; }, dim);
    double c = 0.0;
    for (int j = 0; j < dim; ++j) {
      const double e = X[(size_t)j * ld + r] - mx;
      c += e * e;
    }
    rmx[r] = mx;
    cnu[r] = sqrt(c);
  }
}

struct KgArgs {
  const double* X;
  int ld, n, dim;
  const double* mean;     // column means (k-means++ / Lloyd: distances on centred data)
  const double* C;        // (m, dim) row-major centres
  int m;
  const double* cval;     // per centre: |c|^2 (k-means++ / Lloyd) or |c| (cosine, correlation)
  const double* cmx;      // per centre row mean (correlation)
  const double* xsq;      // per row |x - mean|^2
  const double* enorm;    // per row |x|
  const double* rmx;      // per row mean (correlation)
  const double* cnu;      // per row centred norm (correlation)
  const double* cd_prev;  // k-means++: the previous pass's trial distances (closest = slot best)
  double* cd_out;         // k-means++: this pass's trial distances, (m, n)
  double* part;           // per-workgroup partial sums: (grid, KG_TS) k-means++, (grid) loop
  int* lab32;
  long long* lab64;
  const int* words;       // kWBest (k-means++), kWDone (loop)
};

// Row pass: one row per thread against every centre, centres staged through LDS eight at a time.
//   MODE = kModePP:    k-means++ trial distances min(closest, max(-2 x.c + |c|^2 + |x|^2, 0))
//   MODE = kModeLloyd: sklearn's E-step argmin |c|^2 - 2 x.c on centred data
//   MODE = kKmeans*:   the custom loop's scipy metric, argmin, partial sum of the minima
template <int MODE>
__global__ __launch_bounds__(KG_ROWS) void k_g_rows(KgArgs a) {
  constexpr bool kLoop = MODE != kModePP && MODE != kModeLloyd;
  constexpr bool kCentred = !kLoop;
  if (kLoop && a.words[kWDone]) return;
  __shared__ double s_c[8 * KG_JC];
  __shared__ double s_m[KG_JC];
  __shared__ double s_cmx[8];
  const int tid = threadIdx.x;
  const int r = blockIdx.x * KG_ROWS + tid;
  const bool valid = r < a.n;
  const int rr = valid ? r : a.n - 1;  // every thread takes part in the staging barriers
  const double* xr = a.X + rr;
  double nu = 0.0, mx = 0.0, xs = 0.0, cl = 0.0;
  if (MODE == kKmeansCosine) nu = a.enorm[rr];
  if (MODE == kKmeansCorrelation) {
    nu = a.cnu[rr];
    mx = a.rmx[rr];
  }
  const double* closest = nullptr;
  if (MODE == kModePP) {
    xs = a.xsq[rr];
    if (a.cd_prev) {
      closest = a.cd_prev + (size_t)a.words[kWBest] * a.n;
      cl = closest[rr];
    }
  }
  int best = 0;
  double bd = INFINITY;
  for (int c0 = 0; c0 < a.m; c0 += 8) {
    double acc[8], aux[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = aux[q] = 0.0;
    __syncthreads();  // the previous group's reads of s_cmx are done
    if (MODE == kKmeansCorrelation && tid < 8)
      s_cmx[tid] = c0 + tid < a.m ? a.cmx[c0 + tid] : 0.0;
    for (int j0 = 0; j0 < a.dim; j0 += KG_JC) {
      const int jn = min(KG_JC, a.dim - j0);
      __syncthreads();
      for (int e = tid; e < 8 * jn; e += KG_ROWS) {
        const int q = e / jn, jj = e - q * jn;
        s_c[q * KG_JC + jj] = c0 + q < a.m ? a.C[(size_t)(c0 + q) * a.dim + j0 + jj] : 0.0;
      }
      if (kCentred)
        for (int jj = tid; jj < jn; jj += KG_ROWS) s_m[jj] = a.mean[j0 + jj];
      __syncthreads();
      // columns in order; eight loads of X in flight before their arithmetic
      auto column = [&](double x, int jj) {
        if (kCentred) x = x - s_m[jj];
        if (MODE == kKmeansCorrelation) x = x - mx;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          if (c0 + q < a.m) {
            const double cv = s_c[q * KG_JC + jj];
            if (kCentred || MODE == kKmeansCosine) {
              acc[q] += x * cv;
            } else if (MODE == kKmeansCorrelation) {
              acc[q] += x * (cv - s_cmx[q]);
            } else if (MODE == kKmeansCityblock) {
              acc[q] += fabs(x - cv);
            } else if (MODE == kKmeansChebyshev) {
              acc[q] = fmax(acc[q], fabs(x - cv));
            } else if (MODE == kKmeansBraycurtis) {  // sum |u - v| / sum |u + v|
              acc[q] += fabs(x - cv);
              aux[q] += fabs(x + cv);
            } else if (MODE == kKmeansCanberra) {  // sum |u - v| / (|u| + |v|), 0 / 0 = 0
              const double den = fabs(x) + fabs(cv);
              if (den > 0.0) acc[q] += fabs(x - cv) / den;
            } else {  // (squared) Euclidean
              acc[q] += (x - cv) * (x - cv);
            }
          }
        }
      };
      int jj = 0;
      for (; jj + 8 <= jn; jj += 8) {
        double xv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xv[u] = xr[(size_t)(j0 + jj + u) * a.ld];
#pragma unroll
        for (int u = 0; u < 8; ++u) column(xv[u], jj + u);
      }
      for (; jj < jn; ++jj) column(xr[(size_t)(j0 + jj) * a.ld], jj);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int c = c0 + q;
      if (c >= a.m) continue;
      if (MODE == kModePP) {
        double d = -2.0 * acc[q];
        d += a.cval[c];
        d += xs;
        d = fmax(d, 0.0);
        if (closest) d = fmin(cl, d);
        if (valid) a.cd_out[(size_t)c * a.n + r] = d;
        const double p = wave_sum(valid ? d : 0.0);
        if (tid == 0) a.part[(size_t)blockIdx.x * KG_TS + c] = p;
      } else {
        double d;
        if (MODE == kModeLloyd) {
          d = a.cval[c] - 2.0 * acc[q];
        } else if (MODE == kKmeansCosine || MODE == kKmeansCorrelation) {
          double cosine = acc[q] / (nu * a.cval[c]);
          if (fabs(cosine) > 1.0) cosine = copysign(1.0, cosine);
          d = 1.0 - cosine;
        } else if (MODE == kKmeansBraycurtis) {
          d = acc[q] / aux[q];
        } else if (MODE == kKmeansEuclidean) {
          d = sqrt(acc[q]);
        } else {
          d = acc[q];
        }
        if (d < bd) {  // argmin: first minimum
          bd = d;
          best = c;
        }
      }
    }
  }
  if (MODE == kModePP) return;
  if (valid) {
    a.lab32[r] = best;
    if (kLoop) a.lab64[r] = best;
  }
  if (kLoop) {
    const double p = wave_sum(valid ? bd : 0.0);
    if (tid == 0) a.part[blockIdx.x] = p;
  }
}

// k-means++ step: the pots of the pass over `ntr` trials (partials added in workgroup order),
// argmin -> seeds[c]; then, unless c is the last centre, the next centre's trials: cumsum of the
// chosen distances + searchsorted('left') of rnd * pot, their centred rows and |x|^2.
__global__ __launch_bounds__(KG_ST) void k_g_select(
    int c, int k, int ntr, int trials, int grid, const double* __restrict__ part,
    const double* __restrict__ cd, const double* __restrict__ X, int ld, int n, int dim,
    const double* __restrict__ mean, const double* __restrict__ xsq,
    const double* __restrict__ rnd, int* __restrict__ seeds, int* __restrict__ cand,
    double* __restrict__ crow, double* __restrict__ csq, int* __restrict__ words,
    double* __restrict__ scal) {
  __shared__ double pots[KG_TS];
  __shared__ double rvals[KG_TS];
  __shared__ double sm[KG_ST / 64];
  __shared__ double scan[KG_ST];
  __shared__ int s_best;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (wave < ntr) {  // one wave per trial: lane-strided partials, then the wave's tree
    double s = 0.0;
    for (int g = lane; g < grid; g += 64) s += part[(size_t)g * KG_TS + wave];
    s = wave_sum(s);
    if (lane == 0) pots[wave] = s;
  }
  __syncthreads();
  if (tid == 0) {
    int b = 0;
    for (int t = 1; t < ntr; ++t)
      if (pots[t] < pots[b]) b = t;  // np.argmin: first minimum
    s_best = b;
    words[kWBest] = b;
    seeds[c] = cand[b];
    scal[kSPot] = pots[b];
  }
  __syncthreads();
  if (c + 1 >= k) return;
  const double pot = pots[s_best];
  const double* closest = cd + (size_t)s_best * n;
  __syncthreads();  // every thread has read cand[best] (through seeds) before cand is reset
  if (tid < trials) {
    rvals[tid] = rnd[(size_t)c * trials + tid] * pot;
    cand[tid] = n - 1;  // np.clip(candidate_ids, None, n - 1)
  }
  // inclusive scan of per-thread chunk sums of `closest`
  const int chunk = (n + KG_ST - 1) / KG_ST;
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
    if (lane == 63) sm[wave] = v;
    __syncthreads();
    double off = 0.0;
    for (int w = 0; w < wave; ++w) off += sm[w];
    scan[tid] = v + off;
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
          if (run >= rv) {
            hit = r;
            break;
          }
        }
        atomicMin(&cand[t], hit);
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < trials * dim; e += KG_ST) {
    const int t = e / dim, j = e - t * dim;
    crow[(size_t)t * dim + j] = X[(size_t)j * ld + cand[t]] - mean[j];
  }
  if (tid < trials) csq[tid] = xsq[cand[tid]];
}

// first k-means++ centre: its centred row and |x|^2 as the single trial of pass 0
__global__ __launch_bounds__(256) void k_g_first(int first, const double* __restrict__ X, int ld,
                                                 int dim, const double* __restrict__ mean,
                                                 const double* __restrict__ xsq,
                                                 int* __restrict__ cand,
                                                 double* __restrict__ crow,
                                                 double* __restrict__ csq) {
  for (int j = threadIdx.x; j < dim; j += 256) crow[j] = X[(size_t)j * ld + first] - mean[j];
  if (threadIdx.x == 0) {
    cand[0] = first;
    csq[0] = xsq[first];
  }
}

// Lloyd seeds: the centred rows of the k-means++ picks
__global__ __launch_bounds__(256) void k_g_seedrows(const double* __restrict__ X, int ld,
                                                    int dim, const double* __restrict__ mean,
                                                    const int* __restrict__ seeds,
                                                    double* __restrict__ cent) {
  const int c = blockIdx.x;
  for (int j = threadIdx.x; j < dim; j += 256)
    cent[(size_t)c * dim + j] = X[(size_t)j * ld + seeds[c]] - mean[j];
}

// per-centre constants, one thread per centre, sequential over the columns:
//   kind 0: |c|^2 (Lloyd);  1: |c| (cosine);  2: row mean + centred norm (correlation)
__global__ __launch_bounds__(64) void k_g_cnorm(const double* __restrict__ cent, int k, int dim,
                                                double* __restrict__ cval,
                                                double* __restrict__ cmx, int kind,
                                                const int* __restrict__ words) {
  if (words && words[kWDone]) return;
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= k) return;
  const double* row = cent + (size_t)c * dim;
  double s = 0.0;
  if (kind == 2) {
    const double mc = pw_mean([&](int j) { return row[j]; }, dim);
    for (int j = 0; j < dim; ++j) s += (row[j] - mc) * (row[j] - mc);
    cmx[c] = mc;
  } else {
    for (int j = 0; j < dim; ++j) s += row[j] * row[j];
  }
  cval[c] = kind == 0 ? s : sqrt(s);
}

// Centroid update, one workgroup per column j, eight clusters per sweep over the labels.
//   mode 0 (Lloyd, centred data): mean of members + mean[j]; an empty cluster keeps its seed
//   mode 1 (custom loop): mean of members iff some member INDEX is > 0 (`.any()`, :137-138)
__global__ __launch_bounds__(KG_UT) void k_g_update(const double* __restrict__ X, int ld, int n,
                                                    int dim, int k, const int* __restrict__ lab,
                                                    double* __restrict__ cent,
                                                    const double* __restrict__ mean, int mode,
                                                    const int* __restrict__ words) {
  if (mode == 1 && words[kWDone]) return;
  __shared__ double s_sum[KG_UT / 64][8];
  __shared__ int s_cnt[KG_UT / 64][8];
  const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* col = X + (size_t)j * ld;
  const double mj = mode == 0 ? mean[j] : 0.0;
  const int lab0 = lab[0];
  for (int c0 = 0; c0 < k; c0 += 8) {
    double acc[8];
    int cnt[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      acc[q] = 0.0;
      cnt[q] = 0;
    }
    for (int r = tid; r < n; r += KG_UT) {
      const int l = lab[r] - c0;
      if (l < 0 || l >= 8) continue;
      double x = col[r];
      if (mode == 0) x = x - mj;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (l == q) {
          acc[q] += x;
          ++cnt[q];
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const double v = wave_sum(acc[q]);
      const int cc = wave_sum_int(cnt[q]);
      if (lane == 0) {
        s_sum[wave][q] = v;
        s_cnt[wave][q] = cc;
      }
    }
    __syncthreads();
    if (tid < 8 && c0 + tid < k) {
      const int c = c0 + tid;
      double tot = 0.0;
      int count = 0;
      for (int w = 0; w < KG_UT / 64; ++w) {
        tot += s_sum[w][tid];
        count += s_cnt[w][tid];
      }
      const size_t q = (size_t)c * dim + j;
      if (mode == 0) {
        const double v = count > 0 ? tot / (double)count : cent[q];
        cent[q] = v + mj;
      } else if (count - (lab0 == c ? 1 : 0) > 0) {
        cent[q] = tot / (double)count;
      }
    }
    __syncthreads();
  }
}

// stop rule (:131-133) on the mean of the chosen distances (partials in workgroup order)
__global__ __launch_bounds__(64) void k_g_stop(const double* __restrict__ part, int grid, int n,
                                               int it, int max_iter, double tol,
                                               int* __restrict__ words,
                                               double* __restrict__ scal) {
  if (words[kWDone]) return;
  double s = 0.0;
  for (int g = threadIdx.x; g < grid; g += 64) s += part[g];
  s = wave_sum(s);
  if (threadIdx.x != 0) return;
  const double mean_d = s / (double)n;
  const double prev = scal[kSPrev];
  if ((mean_d <= prev && mean_d >= (1.0 - tol) * prev) || it == max_iter) {
    words[kWDone] = 1;
    words[kWIters] = it + 1;
  } else {
    scal[kSPrev] = mean_d;
  }
}

template <int MODE>
void launch_rows(hipStream_t s, int grid, const KgArgs& a) {
  hipLaunchKernelGGL(k_g_rows<MODE>, dim3(grid), dim3(KG_ROWS), 0, s, a);
}

void launch_loop_rows(hipStream_t s, int grid, const KgArgs& a, int metric) {
  switch (metric) {
    case kKmeansCosine: launch_rows<kKmeansCosine>(s, grid, a); break;
    case kKmeansEuclidean: launch_rows<kKmeansEuclidean>(s, grid, a); break;
    case kKmeansSqeuclidean: launch_rows<kKmeansSqeuclidean>(s, grid, a); break;
    case kKmeansCityblock: launch_rows<kKmeansCityblock>(s, grid, a); break;
    case kKmeansChebyshev: launch_rows<kKmeansChebyshev>(s, grid, a); break;
    case kKmeansCorrelation: launch_rows<kKmeansCorrelation>(s, grid, a); break;
    case kKmeansBraycurtis: launch_rows<kKmeansBraycurtis>(s, grid, a); break;
    default: launch_rows<kKmeansCanberra>(s, grid, a); break;
  }
}

}  // namespace
}  // namespace sc

// workspace of sc_stage_kmeans_general: the handle's kgen buffers, grown on demand, never shared
// with the predict() path
enum { kgX, kgIo, kgRow, kgVec, kgCd, kgPart, kgRnd, kgLab32, kgLab64, kgInt, kgCount };
static_assert(kgCount <= kKgenBufs, "handle.h kgen buffers");

static int ensure_kmeans_general(sc_handle h, int n, int dim, int k, int trials, int grid) {
  const size_t ld = round_up(n, 16);
  SC_TRY(grow(h, h->kgen[kgX], ld * dim * sizeof(double)));
  SC_TRY(grow(h, h->kgen[kgIo], (size_t)n * dim * sizeof(double)));
  SC_TRY(grow(h, h->kgen[kgRow], 4 * ld * sizeof(double)));
  // mean (dim) | centroids (k dim) | cval (k) | cmx (k) | trial rows (KG_TS dim) | csq (KG_TS)
  // | scalars
  SC_TRY(grow(h, h->kgen[kgVec],
              ((size_t)dim * (1 + k + KG_TS) + 2 * (size_t)k + KG_TS + kScalars) *
                  sizeof(double)));
  SC_TRY(grow(h, h->kgen[kgCd], 2 * (size_t)KG_TS * n * sizeof(double)));
  SC_TRY(grow(h, h->kgen[kgPart], (size_t)grid * KG_TS * sizeof(double)));
  SC_TRY(grow(h, h->kgen[kgRnd], (size_t)std::max(1, (k - 1) * trials) * sizeof(double)));
  SC_TRY(grow(h, h->kgen[kgLab32], (size_t)n * sizeof(int)));
  SC_TRY(grow(h, h->kgen[kgLab64], (size_t)n * sizeof(long long)));
  // seeds (k) | trial rows' indices (KG_TS) | words
  SC_TRY(grow(h, h->kgen[kgInt], ((size_t)k + KG_TS + kWords) * sizeof(int)));
  return SC_OK;
}

extern "C" int sc_stage_kmeans_general(sc_handle h, const double* x, int n, int dim, int k,
                                       int max_iter, int metric, double tol,
                                       const double* init_centroids, int64_t* labels,
                                       double* centroids_out, int* iterations) {
  if (!h) return SC_ERR_INVALID;
  if (!x || !labels || n <= 0 || dim <= 0 || k <= 0)
    return fail(h, SC_ERR_INVALID, "bad k-means input");
  if ((long long)n * dim > 0x7fffffffLL)
    return fail(h, SC_ERR_INVALID, "k-means input larger than 2^31 elements");
  if (metric < kKmeansCosine || metric > kKmeansCanberra)
    return fail(h, SC_ERR_UNSUPPORTED,
                "custom_dist on the device: cosine, euclidean (minkowski), sqeuclidean, "
                "cityblock, chebyshev, correlation, braycurtis, canberra");
  if (max_iter <= 0)
    return fail(h, SC_ERR_INVALID, "Number of iterations should be a positive number");
  if (n < k) return fail(h, SC_ERR_INVALID, "n_samples should be >= n_clusters");
  const int trials = 2 + (int)std::log((double)k);
  if (trials > KG_TS) return fail(h, SC_ERR_UNSUPPORTED, "too many k-means++ trials");
  SC_HIP(h, hipSetDevice(h->device));
  const int ld = round_up(n, 16);
  const int grid = (n + KG_ROWS - 1) / KG_ROWS;
  SC_TRY(ensure_kmeans_general(h, n, dim, k, trials, grid));
  hipStream_t s = h->stream;
  double* X = ptr<double>(h->kgen[kgX]);
  double* row = ptr<double>(h->kgen[kgRow]);
  double *xsq = row, *enorm = row + ld, *rmx = row + 2 * (size_t)ld, *cnu = row + 3 * (size_t)ld;
  double* vec = ptr<double>(h->kgen[kgVec]);
  double* mean = vec;
  double* cent = mean + dim;
  double* cval = cent + (size_t)k * dim;
  double* cmx = cval + k;
  double* crow = cmx + k;
  double* csq = crow + (size_t)KG_TS * dim;
  double* scal = csq + KG_TS;
  double* cd = ptr<double>(h->kgen[kgCd]);
  double* part = ptr<double>(h->kgen[kgPart]);
  double* rnd = ptr<double>(h->kgen[kgRnd]);
  int* lab32 = ptr<int>(h->kgen[kgLab32]);
  long long* lab64 = ptr<long long>(h->kgen[kgLab64]);
  int* seeds = ptr<int>(h->kgen[kgInt]);
  int* cand = seeds + k;
  int* words = cand + KG_TS;

  SC_HIP(h, hipMemcpyAsync(h->kgen[kgIo].p, x, (size_t)n * dim * sizeof(double),
                           hipMemcpyHostToDevice, s));
  const size_t nel = (size_t)n * dim;
  hipLaunchKernelGGL(k_g_colmajor, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, s,
                     ptr<double>(h->kgen[kgIo]), n, dim, X, ld);
  SC_HIP(h, hipMemsetAsync(words, 0, kWords * sizeof(int), s));
  SC_HIP(h, hipMemsetAsync(scal, 0, kScalars * sizeof(double), s));
  hipLaunchKernelGGL(k_g_colmean, dim3(dim), dim3(KG_UT), 0, s, X, ld, n, mean);
  hipLaunchKernelGGL(k_g_rowstats, dim3(grid), dim3(KG_ROWS), 0, s, X, ld, n, dim, mean, xsq,
                     enorm, rmx, cnu, metric == kKmeansCorrelation ? 1 : 0);

  KgArgs a{};
  a.X = X;
  a.ld = ld;
  a.n = n;
  a.dim = dim;
  a.mean = mean;
  a.xsq = xsq;
  a.enorm = enorm;
  a.rmx = rmx;
  a.cnu = cnu;
  a.part = part;
  a.lab32 = lab32;
  a.lab64 = lab64;
  a.words = words;
  std::vector<double> rv;  // RandomState(0) doubles: alive until the first synchronisation
  if (init_centroids) {
    SC_HIP(h, hipMemcpyAsync(cent, init_centroids, (size_t)k * dim * sizeof(double),
                             hipMemcpyHostToDevice, s));
  } else {
    // k-means++ (sklearn _kmeans_plusplus, unit sample weights), RandomState(0) stream
    double u_first;
    int tr;
    kmeans_seed_constants(k, &u_first, &tr, &rv);
    SC_HIP(h, hipMemcpyAsync(rnd, rv.data(), rv.size() * sizeof(double), hipMemcpyHostToDevice,
                             s));
    const int first = sc_uniform_choice(n, u_first);
    hipLaunchKernelGGL(k_g_first, dim3(1), dim3(256), 0, s, first, X, ld, dim, mean, xsq, cand,
                       crow, csq);
    KgArgs p = a;
    p.C = crow;
    p.cval = csq;
    for (int c = 0; c < k; ++c) {
      const int ntr = c == 0 ? 1 : trials;
      p.m = ntr;
      p.cd_prev = c == 0 ? nullptr : cd + (size_t)((c - 1) & 1) * KG_TS * n;
      p.cd_out = cd + (size_t)(c & 1) * KG_TS * n;
      launch_rows<kModePP>(s, grid, p);
      hipLaunchKernelGGL(k_g_select, dim3(1), dim3(KG_ST), 0, s, c, k, ntr, trials, grid, part,
                         p.cd_out, X, ld, n, dim, mean, xsq, rnd, seeds, cand, crow, csq,
                         words, scal);
    }
    // one Euclidean Lloyd step on the centred data (max_iter = 1)
    hipLaunchKernelGGL(k_g_seedrows, dim3(k), dim3(256), 0, s, X, ld, dim, mean, seeds, cent);
    hipLaunchKernelGGL(k_g_cnorm, dim3((k + 63) / 64), dim3(64), 0, s, cent, k, dim, cval, cmx,
                       0, nullptr);
    KgArgs l = a;
    l.C = cent;
    l.m = k;
    l.cval = cval;
    launch_rows<kModeLloyd>(s, grid, l);
    hipLaunchKernelGGL(k_g_update, dim3(dim), dim3(KG_UT), 0, s, X, ld, n, dim, k, lab32, cent,
                       mean, 0, words);
  }
  SC_TRY(check_last(h, "k-means seeding launch"));

  // the custom loop, KG_ITERS iterations per host synchronisation; kernels after the stop rule
  // fired return at once, `done` comes back with the labels
  KgArgs l = a;
  l.C = cent;
  l.m = k;
  l.cval = cval;
  l.cmx = cmx;
  const int kind = metric == kKmeansCorrelation ? 2 : 1;
  int w[kWords] = {0};
  for (int it0 = 0;; it0 += KG_ITERS) {
    for (int it = it0; it < it0 + KG_ITERS && it <= max_iter; ++it) {
      if (metric == kKmeansCosine || metric == kKmeansCorrelation)
        hipLaunchKernelGGL(k_g_cnorm, dim3((k + 63) / 64), dim3(64), 0, s, cent, k, dim, cval,
                           cmx, kind, words);
      launch_loop_rows(s, grid, l, metric);
      hipLaunchKernelGGL(k_g_stop, dim3(1), dim3(64), 0, s, part, grid, n, it, max_iter, tol,
                         words, scal);
      hipLaunchKernelGGL(k_g_update, dim3(dim), dim3(KG_UT), 0, s, X, ld, n, dim, k, lab32,
                         cent, mean, 1, words);
    }
    SC_TRY(check_last(h, "k-means loop launch"));
    SC_HIP(h, hipMemcpyAsync(w, words, kWords * sizeof(int), hipMemcpyDeviceToHost, s));
    SC_HIP(h, hipStreamSynchronize(s));
    if (w[kWDone]) break;
    if (it0 > max_iter) return fail(h, SC_ERR_HIP, "k-means loop did not reach its stop rule");
  }
  SC_HIP(h, hipMemcpyAsync(labels, lab64, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost,
                           s));
  if (centroids_out)
    SC_HIP(h, hipMemcpyAsync(centroids_out, cent, (size_t)k * dim * sizeof(double),
                             hipMemcpyDeviceToHost, s));
  SC_HIP(h, hipStreamSynchronize(s));
  if (iterations) *iterations = w[kWIters];
  return SC_OK;
}
