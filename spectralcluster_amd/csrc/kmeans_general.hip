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
// is compiled with -ffp-contract=off; the per-metric arithmetic is kmeans_common.h's, shared with
// kmeans.hip.  Kernels and launchers only: sc_stage_kmeans_general drives them (kmeans_api.hip).
#include "kmeans_common.h"
#include "sc_internal.h"

namespace sc {
namespace {

constexpr int KG_ROWS = 64;   // rows (threads) per workgroup of the row passes: one wave
constexpr int KG_JC = 256;    // centroid columns per LDS chunk
constexpr int KG_TS = kKgenTrialSlots;  // k-means++ trial slots (2 + int(log k) used)
constexpr int KG_UT = 256;    // threads of the column-parallel update / column means
constexpr int KG_ST = 1024;   // threads of the k-means++ select launch

enum { kModePP = 100, kModeLloyd = 101 };
enum { kSPot = 0, kSPrev = 1 };  // double scalars: pot, prev mean distance (of kKgenScalars)

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
  const int* words;       // kKgenBest (k-means++), kKgenDone (loop)
};

// Row pass: one row per thread against every centre, centres staged through LDS eight at a time.
//   MODE = kModePP:    k-means++ trial distances min(closest, max(-2 x.c + |c|^2 + |x|^2, 0))
//   MODE = kModeLloyd: sklearn's E-step argmin |c|^2 - 2 x.c on centred data
//   MODE = kKmeans*:   the custom loop's scipy metric, argmin, partial sum of the minima
template <int MODE>
__global__ __launch_bounds__(KG_ROWS) void k_g_rows(KgArgs a) {
  constexpr bool kLoop = MODE != kModePP && MODE != kModeLloyd;
  constexpr bool kCentred = !kLoop;
  if (kLoop && a.words[kKgenDone]) return;
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
      closest = a.cd_prev + (size_t)a.words[kKgenBest] * a.n;
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
            if (kCentred)
              acc[q] += x * cv;
            else
              metric_accumulate(MODE, x, cv, MODE == kKmeansCorrelation ? s_cmx[q] : 0.0, acc[q],
                                aux[q]);
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
        const double d = MODE == kModeLloyd ? a.cval[c] - 2.0 * acc[q]
                                            : metric_finish(MODE, acc[q], aux[q], nu, a.cval[c]);
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
    words[kKgenBest] = b;
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
  if (words && words[kKgenDone]) return;
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
  if (mode == 1 && words[kKgenDone]) return;
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
      const int cc = wave_sum(cnt[q]);
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
  if (words[kKgenDone]) return;
  double s = 0.0;
  for (int g = threadIdx.x; g < grid; g += 64) s += part[g];
  s = wave_sum(s);
  if (threadIdx.x != 0) return;
  const double mean_d = s / (double)n;
  const double prev = scal[kSPrev];
  if ((mean_d <= prev && mean_d >= (1.0 - tol) * prev) || it == max_iter) {
    words[kKgenDone] = 1;
    words[kKgenIters] = it + 1;
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

KgArgs kg_args(const KmeansGeneralWorkspace& ws, int n, int dim) {
  KgArgs a{};
  a.X = ws.X;
  a.ld = ws.ld;
  a.n = n;
  a.dim = dim;
  a.mean = ws.mean;
  a.xsq = ws.xsq;
  a.enorm = ws.enorm;
  a.rmx = ws.rmx;
  a.cnu = ws.cnu;
  a.part = ws.part;
  a.lab32 = ws.lab32;
  a.lab64 = ws.lab64;
  a.words = ws.words;
  return a;
}

}  // namespace

int kmeans_general_grid(int n) { return (n + KG_ROWS - 1) / KG_ROWS; }

// column means and the per-row constants of X (ws.words and ws.scal are zero)
void launch_kmeans_general_stats(hipStream_t s, const KmeansGeneralWorkspace& ws, int n, int dim,
                                 int metric) {
  hipLaunchKernelGGL(k_g_colmean, dim3(dim), dim3(KG_UT), 0, s, ws.X, ws.ld, n, ws.mean);
  hipLaunchKernelGGL(k_g_rowstats, dim3(kmeans_general_grid(n)), dim3(KG_ROWS), 0, s, ws.X, ws.ld,
                     n, dim, ws.mean, ws.xsq, ws.enorm, ws.rmx, ws.cnu,
                     metric == kKmeansCorrelation ? 1 : 0);
}

// ws.cent <- sklearn's seeds: k-means++ (unit sample weights) from row `first` with the
// RandomState(0) doubles in ws.rnd, then one Euclidean Lloyd step on the centred data
void launch_kmeans_general_seed(hipStream_t s, const KmeansGeneralWorkspace& ws, int n, int dim,
                                int k, int trials, int first) {
  const int grid = kmeans_general_grid(n);
  hipLaunchKernelGGL(k_g_first, dim3(1), dim3(256), 0, s, first, ws.X, ws.ld, dim, ws.mean,
                     ws.xsq, ws.cand, ws.crow, ws.csq);
  KgArgs p = kg_args(ws, n, dim);
  p.C = ws.crow;
  p.cval = ws.csq;
  for (int c = 0; c < k; ++c) {
    const int ntr = c == 0 ? 1 : trials;
    p.m = ntr;
    p.cd_prev = c == 0 ? nullptr : ws.cd + (size_t)((c - 1) & 1) * KG_TS * n;
    p.cd_out = ws.cd + (size_t)(c & 1) * KG_TS * n;
    launch_rows<kModePP>(s, grid, p);
    hipLaunchKernelGGL(k_g_select, dim3(1), dim3(KG_ST), 0, s, c, k, ntr, trials, grid, ws.part,
                       p.cd_out, ws.X, ws.ld, n, dim, ws.mean, ws.xsq, ws.rnd, ws.seeds, ws.cand,
                       ws.crow, ws.csq, ws.words, ws.scal);
  }
  // one Euclidean Lloyd step on the centred data (max_iter = 1)
  hipLaunchKernelGGL(k_g_seedrows, dim3(k), dim3(256), 0, s, ws.X, ws.ld, dim, ws.mean, ws.seeds,
                     ws.cent);
  hipLaunchKernelGGL(k_g_cnorm, dim3((k + 63) / 64), dim3(64), 0, s, ws.cent, k, dim, ws.cval,
                     ws.cmx, 0, nullptr);
  KgArgs l = kg_args(ws, n, dim);
  l.C = ws.cent;
  l.m = k;
  l.cval = ws.cval;
  launch_rows<kModeLloyd>(s, grid, l);
  hipLaunchKernelGGL(k_g_update, dim3(dim), dim3(KG_UT), 0, s, ws.X, ws.ld, n, dim, k, ws.lab32,
                     ws.cent, ws.mean, 0, ws.words);
}

// iteration `it` of the custom loop: assignment, stop rule, centroid update.  Once the stop rule
// has fired (ws.words[kKgenDone]) every kernel returns at once.
void launch_kmeans_general_iteration(hipStream_t s, const KmeansGeneralWorkspace& ws, int n,
                                     int dim, int k, int metric, int it, int max_iter,
                                     double tol) {
  const int grid = kmeans_general_grid(n);
  KgArgs l = kg_args(ws, n, dim);
  l.C = ws.cent;
  l.m = k;
  l.cval = ws.cval;
  l.cmx = ws.cmx;
  if (metric == kKmeansCosine || metric == kKmeansCorrelation)
    hipLaunchKernelGGL(k_g_cnorm, dim3((k + 63) / 64), dim3(64), 0, s, ws.cent, k, dim, ws.cval,
                       ws.cmx, metric == kKmeansCorrelation ? 2 : 1, ws.words);
  launch_loop_rows(s, grid, l, metric);
  hipLaunchKernelGGL(k_g_stop, dim3(1), dim3(64), 0, s, ws.part, grid, n, it, max_iter, tol,
                     ws.words, ws.scal);
  hipLaunchKernelGGL(k_g_update, dim3(dim), dim3(KG_UT), 0, s, ws.X, ws.ld, n, dim, k, ws.lab32,
                     ws.cent, ws.mean, 1, ws.words);
}

}  // namespace sc
