// Host driver of the k-means stage: workspaces, the RandomState(0) seeding constants, the choice
// between the kernel chain (kmeans_chain.hip) and the single-workgroup kernel (kmeans.hip) for
// the (n, k) spectral embedding, the general form for an (n, dim) input of any width
// (kmeans_general.hip), and the C ABI entry points sc_cluster / sc_stage_kmeans*.
// Host code only decides and launches.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "handle.h"

// ------------------------------------------------------------------------------
// workspaces
// ------------------------------------------------------------------------------
int ensure_kmeans(sc_handle h, int n, int k) {
  const int cols = std::max(k, kMaxCols), kk = std::max(k, kMaxVectors);
  SC_TRY(grow(h, h->Ek, (size_t)round_up(n, 16) * cols * sizeof(double)));
  SC_TRY(grow(h, h->Eio, (size_t)n * cols * sizeof(double)));
  SC_TRY(grow(h, h->kXc, (size_t)n * kk * sizeof(double)));
  SC_TRY(grow(h, h->kxsq, (size_t)n * sizeof(double)));
  SC_TRY(grow(h, h->kclosest, (size_t)n * sizeof(double)));
  SC_TRY(grow(h, h->kcand, (size_t)(k > kMaxVectors ? 16 : 8) * n * sizeof(double)));
  SC_TRY(grow(h, h->kenorm, (size_t)n * sizeof(double)));
  SC_TRY(grow(h, h->krnd, (size_t)std::max(1024, 16 * kk) * sizeof(double)));
  SC_TRY(grow(h, h->kcent, (size_t)kk * kk * sizeof(double)));
  if (k > kMaxVectors) {  // the large-k form keeps its per-cluster arrays in global memory
    SC_TRY(grow(h, h->kbig, kmeans_big_workspace_doubles(k) * sizeof(double)));
    SC_TRY(grow(h, h->kbigw, (size_t)3 * k * sizeof(int)));
  }
  SC_TRY(grow(h, h->klab32, (size_t)n * sizeof(int)));
  SC_TRY(grow(h, h->klab64, (size_t)n * sizeof(long long)));
  SC_TRY(grow(h, h->kinfo, 16 * sizeof(int)));
  SC_TRY(grow(h, h->kchain, kmeans_chain_workspace_doubles(n) * sizeof(double)));
  return SC_OK;
}

KmeansWorkspace kmeans_workspace(sc_handle h) {
  KmeansWorkspace ws;
  ws.Xc = ptr<double>(h->kXc);
  ws.xsq = ptr<double>(h->kxsq);
  ws.closest = ptr<double>(h->kclosest);
  ws.cand = ptr<double>(h->kcand);
  ws.enorm = ptr<double>(h->kenorm);
  ws.rnd = ptr<double>(h->krnd);
  ws.centroids = ptr<double>(h->kcent);
  ws.labels32 = ptr<int>(h->klab32);
  ws.labels64 = ptr<long long>(h->klab64);
  ws.info = ptr<int>(h->kinfo);
  ws.chain = ptr<double>(h->kchain);
  ws.big = ptr<double>(h->kbig);
  ws.big_words = ptr<int>(h->kbigw);
  return ws;
}

// workspace of sc_stage_kmeans_general: the handle's kgen buffers, grown on demand, never shared
// with the predict() path
enum { kgX, kgIo, kgRow, kgVec, kgCd, kgPart, kgRnd, kgLab32, kgLab64, kgInt, kgCount };
static_assert(kgCount <= kKgenBufs, "handle.h kgen buffers");

// (`row_major_io`: the (n, dim) fp64 copy of a compact host input, which k_to_colmajor reads)
static int ensure_kmeans_general(sc_handle h, int n, int dim, int k, int trials,
                                 bool row_major_io, KmeansGeneralWorkspace* ws) {
  constexpr int TS = kKgenTrialSlots;
  const size_t ld = round_up(n, 16);
  SC_TRY(grow(h, h->kgen[kgX], ld * dim * sizeof(double)));
  if (row_major_io) SC_TRY(grow(h, h->kgen[kgIo], (size_t)n * dim * sizeof(double)));
  SC_TRY(grow(h, h->kgen[kgRow], 4 * ld * sizeof(double)));
  // mean (dim) | centroids (k dim) | cval (k) | cmx (k) | trial rows (TS dim) | csq (TS) | scalars
  SC_TRY(grow(h, h->kgen[kgVec],
              ((size_t)dim * (1 + k + TS) + 2 * (size_t)k + TS + kKgenScalars) * sizeof(double)));
  SC_TRY(grow(h, h->kgen[kgCd], 2 * (size_t)TS * n * sizeof(double)));
  SC_TRY(grow(h, h->kgen[kgPart], (size_t)kmeans_general_grid(n) * TS * sizeof(double)));
  SC_TRY(grow(h, h->kgen[kgRnd], (size_t)std::max(1, (k - 1) * trials) * sizeof(double)));
  SC_TRY(grow(h, h->kgen[kgLab32], (size_t)n * sizeof(int)));
  SC_TRY(grow(h, h->kgen[kgLab64], (size_t)n * sizeof(long long)));
  // seeds (k) | trial rows' indices (TS) | words
  SC_TRY(grow(h, h->kgen[kgInt], ((size_t)k + TS + kKgenWords) * sizeof(int)));
  ws->X = ptr<double>(h->kgen[kgX]);
  ws->ld = (int)ld;
  ws->xsq = ptr<double>(h->kgen[kgRow]);
  ws->enorm = ws->xsq + ld;
  ws->rmx = ws->xsq + 2 * ld;
  ws->cnu = ws->xsq + 3 * ld;
  ws->mean = ptr<double>(h->kgen[kgVec]);
  ws->cent = ws->mean + dim;
  ws->cval = ws->cent + (size_t)k * dim;
  ws->cmx = ws->cval + k;
  ws->crow = ws->cmx + k;
  ws->csq = ws->crow + (size_t)TS * dim;
  ws->scal = ws->csq + TS;
  ws->cd = ptr<double>(h->kgen[kgCd]);
  ws->part = ptr<double>(h->kgen[kgPart]);
  ws->rnd = ptr<double>(h->kgen[kgRnd]);
  ws->lab32 = ptr<int>(h->kgen[kgLab32]);
  ws->lab64 = ptr<long long>(h->kgen[kgLab64]);
  ws->seeds = ptr<int>(h->kgen[kgInt]);
  ws->cand = ws->seeds + k;
  ws->words = ws->cand + TS;
  return SC_OK;
}

// ------------------------------------------------------------------------------
// what both forms ask of their arguments, and the seeding constants
// ------------------------------------------------------------------------------
void kmeans_seed_constants(int k, double* u_first, int* trials, std::vector<double>* rnd) {
  *trials = 2 + (int)std::log((double)k);
  const size_t nrnd = (size_t)std::max(1, (k - 1) * *trials);
  std::vector<double> stream(1 + nrnd);
  sc_random_state_doubles(0, (int)stream.size(), stream.data());
  *u_first = stream[0];
  rnd->assign(stream.begin() + 1, stream.end());
}

// `slots`: k-means++ trial slots of the kernel that will run (sklearn draws 2 + int(log k)
// candidates per centre: at most 6 up to 64 centres; 16 cover every k an int holds)
static int check_kmeans_request(sc_handle h, int n, int k, int max_iter, int metric, int slots) {
  if (metric < kKmeansCosine || metric > kKmeansCanberra)
    return fail(h, SC_ERR_UNSUPPORTED,
                "custom_dist on the device: cosine, euclidean (minkowski), sqeuclidean, "
                "cityblock, chebyshev, correlation, braycurtis, canberra");
  if (max_iter <= 0)
    return fail(h, SC_ERR_INVALID, "Number of iterations should be a positive number");
  if (n < k) return fail(h, SC_ERR_INVALID, "n_samples should be >= n_clusters");
  if (k < 1) return fail(h, SC_ERR_INVALID, "n_clusters must be positive");
  if (2 + (int)std::log((double)k) > slots)
    return fail(h, SC_ERR_UNSUPPORTED, "too many k-means++ trials");
  return SC_OK;
}

// ------------------------------------------------------------------------------
// the (n, k) spectral embedding
// ------------------------------------------------------------------------------
// the RandomState(0) constants are functions of n and k: what the last call left is reused
// (h->kfirst, h->krnd_trials, and the doubles in h->krnd)
static int kmeans_seed_state(sc_handle h, int n, int k) {
  if (h->kfirst_n != n || h->krnd_k != k) {
    double u_first;
    int trials;
    std::vector<double> rnd;
    kmeans_seed_constants(k, &u_first, &trials, &rnd);
    // first centre via choice(n, p=uniform) = cdf.searchsorted(u, 'right')
    if (h->kfirst_n != n) {  // (two passes of n dependent adds: ~20 us at n = 8192)
      h->kfirst = sc_uniform_choice(n, u_first);
      h->kfirst_n = n;
    }
    if (h->krnd_k != k) {
      SC_HIP(h, hipMemcpyAsync(h->krnd.p, rnd.data(), rnd.size() * sizeof(double),
                               hipMemcpyHostToDevice, h->stream));
      SC_HIP(h, hipStreamSynchronize(h->stream));  // rnd is a local
      h->krnd_k = k;
      h->krnd_trials = trials;
    }
  }
  return SC_OK;
}

static int kmeans_on_device(sc_handle h, const double* E, int lde, int n, int k, int max_iter,
                            int64_t* labels, double* centroids_out, int* iterations,
                            int metric = kKmeansCosine) {
  // 8 trial slots up to kMaxVectors centres, 16 in the large-k form
  SC_TRY(check_kmeans_request(h, n, k, max_iter, metric, k > kMaxVectors ? 16 : 8));
  SC_TRY(ensure_kmeans(h, n, k));
  SC_TRY(kmeans_seed_state(h, n, k));
  const int first = h->kfirst, trials = h->krnd_trials;
  const KmeansWorkspace ws = kmeans_workspace(h);
  int info[16] = {0};
  if (metric == kKmeansCosine && kmeans_chain_supported(n, k, trials) &&
      !sw::kmeans_single()) {
    // chain of short multi-workgroup kernels; cosine iterations four launches at a time
    // (the typical run stops after two or three), `done` comes back with the labels
    for (int it = 0;; it += 4) {
      launch_kmeans_chain(h->stream, E, lde, n, k, max_iter, first, trials, ws, it, 4);
      SC_TRY(check_last(h, "kmeans launch"));
      SC_HIP(h, hipMemcpyAsync(labels, h->klab64.p, (size_t)n * sizeof(int64_t),
                               hipMemcpyDeviceToHost, h->stream));
      SC_HIP(h, hipMemcpyAsync(info, h->kinfo.p, 9 * sizeof(int), hipMemcpyDeviceToHost,
                               h->stream));
      SC_HIP(h, hipStreamSynchronize(h->stream));
      if (info[8] != 0) break;
      if (it > max_iter + 4)
        return fail(h, SC_ERR_HIP, "k-means chain did not reach its stop rule");
    }
    if (centroids_out) {
      SC_HIP(h, hipMemcpyAsync(centroids_out, h->kcent.p, (size_t)k * k * sizeof(double),
                               hipMemcpyDeviceToHost, h->stream));
      SC_HIP(h, hipStreamSynchronize(h->stream));
    }
    if (iterations) *iterations = info[0];
    return SC_OK;
  }
  SC_HIP(h, hipMemsetAsync(h->kinfo.p, 0, 8 * sizeof(int), h->stream));
  launch_kmeans(h->stream, E, lde, n, k, max_iter, first, trials, ws, metric);
  SC_TRY(check_last(h, "kmeans launch"));
  SC_HIP(h, hipMemcpyAsync(labels, h->klab64.p, (size_t)n * sizeof(int64_t),
                           hipMemcpyDeviceToHost, h->stream));
  SC_HIP(h, hipMemcpyAsync(info, h->kinfo.p, 6 * sizeof(int), hipMemcpyDeviceToHost,
                           h->stream));
  if (centroids_out)
    SC_HIP(h, hipMemcpyAsync(centroids_out, h->kcent.p, (size_t)k * k * sizeof(double),
                             hipMemcpyDeviceToHost, h->stream));
  SC_HIP(h, hipStreamSynchronize(h->stream));
  if (iterations) *iterations = info[0];
  if (sw::kmeans_trace())
    fprintf(stderr, "[sc] kmeans n=%d k=%d iters=%d  us: centre %.1f  kmeans++ %.1f  lloyd %.1f"
            "  cosine-loop %.1f\n", n, k, info[0], info[1] * 0.01, (info[2] - info[1]) * 0.01,
            (info[3] - info[2]) * 0.01, (info[4] - info[3]) * 0.01);
  if (sw::kmeans_trace() && k > kMaxVectors) {  // the large-k form keeps its seeds in global memory
    std::vector<int> seeds(k);
    hipMemcpy(seeds.data(), h->kbigw.p, (size_t)k * sizeof(int), hipMemcpyDeviceToHost);
    fprintf(stderr, "[sc] kmeans++ seeds:");
    for (int i = 0; i < k; ++i) fprintf(stderr, " %d", seeds[i]);
    fprintf(stderr, "\n");
  }
  return SC_OK;
}

extern "C" int sc_cluster(sc_handle h, const sc_config* cfg, int n_clusters, int64_t* labels,
                          sc_diag* diag) {
  if (!h) return SC_ERR_INVALID;
  if (!cfg || !labels) return fail(h, SC_ERR_INVALID, "NULL argument");
  if (h->n_vec <= 0) return fail(h, SC_ERR_INVALID, "no eigenvectors resident");
  if (n_clusters < 1 || n_clusters > h->n_vec)
    return fail(h, SC_ERR_INVALID, "n_clusters exceeds the resident eigenvectors");
  SC_HIP(h, hipSetDevice(h->device));
  const int n = h->n;
  int e0, e1;
  ev_rec(h, &e0);
  const double* E = ptr<double>(h->E);
  const int lde = round_up(n, 16);
  if (cfg->row_wise_renorm) {
    SC_TRY(ensure_kmeans(h, n, n_clusters));
    SC_HIP(h, hipMemcpyAsync(h->Ek.p, h->E.p, (size_t)lde * n_clusters * sizeof(double),
                             hipMemcpyDeviceToDevice, h->stream));
    launch_row_renorm(h->stream, ptr<double>(h->Ek), lde, n, n_clusters);
    E = ptr<double>(h->Ek);
  }
  int iters = 0;
  SC_TRY(kmeans_on_device(h, E, lde, n, n_clusters, cfg->max_iter, labels, nullptr, &iters,
                          cfg->kmeans_metric));
  ev_rec(h, &e1);
  SC_HIP(h, hipStreamSynchronize(h->stream));
  if (diag) {
    diag->n_clusters = n_clusters;
    diag->kmeans_iterations = iters;
    diag->stage_ms[SC_STAGE_KMEANS] = ev_ms(h, e0, e1);
  }
  return SC_OK;
}

// the (n, k) embedding `e` (validated) into h->Ek, column-major: compact host fp64 rows by the
// copy and the transposition they have always had, every other source by the widening ingest
static int kmeans_metric_on(sc_handle h, const sc_array& e, int max_iter, int metric,
                            int64_t* labels, double* centroids_out, int* iterations) {
  const int n = (int)e.rows, k = (int)e.cols, lde = round_up(n, 16);
  SC_TRY(check_kmeans_request(h, n, k, max_iter, metric, k > kMaxVectors ? 16 : 8));
  SC_HIP(h, hipSetDevice(h->device));
  SC_TRY(ensure_kmeans(h, n, k));
  if (array_is_compact_host_f64(e)) {
    SC_HIP(h, hipMemcpyAsync(h->Eio.p, e.data, (size_t)n * k * sizeof(double),
                             hipMemcpyHostToDevice, h->stream));
    launch_to_colmajor(h->stream, ptr<double>(h->Eio), n, k, ptr<double>(h->Ek), lde);
  } else {
    SC_TRY(ingest_columns_into(h, e, ptr<double>(h->Ek), lde, h->stream));
  }
  return kmeans_on_device(h, ptr<double>(h->Ek), lde, n, k, max_iter, labels, centroids_out,
                          iterations, metric);
}

extern "C" int sc_stage_kmeans_metric(sc_handle h, const double* e, int n, int k, int max_iter,
                                      int metric, int64_t* labels, double* centroids_out,
                                      int* iterations) {
  if (!h) return SC_ERR_INVALID;
  if (!e || !labels || n <= 0 || k <= 0) return fail(h, SC_ERR_INVALID, "bad k-means input");
  return kmeans_metric_on(h, host_f64_array(e, n, k), max_iter, metric, labels, centroids_out,
                          iterations);
}

extern "C" int sc_stage_kmeans_metric_array(sc_handle h, const sc_array* e, int max_iter,
                                            int metric, int64_t* labels, double* centroids_out,
                                            int* iterations) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_kmeans_array(h, e));
  if (!labels) return fail(h, SC_ERR_INVALID, "labels is NULL");
  return kmeans_metric_on(h, *e, max_iter, metric, labels, centroids_out, iterations);
}

extern "C" int sc_stage_kmeans(sc_handle h, const double* e, int n, int k, int max_iter,
                               int64_t* labels, double* centroids_out, int* iterations) {
  return sc_stage_kmeans_metric(h, e, n, k, max_iter, SC_KMEANS_COSINE, labels, centroids_out,
                                iterations);
}

// ------------------------------------------------------------------------------
// an (n, dim) input of any width: run_kmeans with dim != k, CustomKMeans
// ------------------------------------------------------------------------------
// `x`: a validated source of at most 2^31 - 1 elements
static int kmeans_general_on(sc_handle h, const sc_array& x, int k, int max_iter, int metric,
                             double tol, const double* init_centroids, int64_t* labels,
                             double* centroids_out, int* iterations) {
  constexpr int kItersPerSync = 4;  // loop iterations enqueued per host synchronisation
  const int n = (int)x.rows, dim = (int)x.cols;
  const bool compact = array_is_compact_host_f64(x);
  SC_TRY(check_kmeans_request(h, n, k, max_iter, metric, kKgenTrialSlots));
  double u_first;
  int trials;
  std::vector<double> rnd;  // alive until the first synchronisation
  kmeans_seed_constants(k, &u_first, &trials, &rnd);
  SC_HIP(h, hipSetDevice(h->device));
  KmeansGeneralWorkspace ws;
  SC_TRY(ensure_kmeans_general(h, n, dim, k, trials, compact, &ws));
  hipStream_t s = h->stream;

  if (compact) {
    SC_HIP(h, hipMemcpyAsync(h->kgen[kgIo].p, x.data, (size_t)n * dim * sizeof(double),
                             hipMemcpyHostToDevice, s));
    launch_to_colmajor(s, ptr<double>(h->kgen[kgIo]), n, dim, ws.X, ws.ld);
  } else {
    SC_TRY(ingest_columns_into(h, x, ws.X, ws.ld, s));
  }
  SC_HIP(h, hipMemsetAsync(ws.words, 0, kKgenWords * sizeof(int), s));
  SC_HIP(h, hipMemsetAsync(ws.scal, 0, kKgenScalars * sizeof(double), s));
  launch_kmeans_general_stats(s, ws, n, dim, metric);
  if (init_centroids) {
    SC_HIP(h, hipMemcpyAsync(ws.cent, init_centroids, (size_t)k * dim * sizeof(double),
                             hipMemcpyHostToDevice, s));
  } else {
    SC_HIP(h, hipMemcpyAsync(ws.rnd, rnd.data(), rnd.size() * sizeof(double),
                             hipMemcpyHostToDevice, s));
    launch_kmeans_general_seed(s, ws, n, dim, k, trials, sc_uniform_choice(n, u_first));
  }
  SC_TRY(check_last(h, "k-means seeding launch"));

  // the custom loop; kernels after the stop rule fired return at once, `done` comes back with
  // the labels
  int w[kKgenWords] = {0};
  for (int it0 = 0;; it0 += kItersPerSync) {
    for (int it = it0; it < it0 + kItersPerSync && it <= max_iter; ++it)
      launch_kmeans_general_iteration(s, ws, n, dim, k, metric, it, max_iter, tol);
    SC_TRY(check_last(h, "k-means loop launch"));
    SC_HIP(h, hipMemcpyAsync(w, ws.words, kKgenWords * sizeof(int), hipMemcpyDeviceToHost, s));
    SC_HIP(h, hipStreamSynchronize(s));
    if (w[kKgenDone]) break;
    if (it0 > max_iter) return fail(h, SC_ERR_HIP, "k-means loop did not reach its stop rule");
  }
  SC_HIP(h, hipMemcpyAsync(labels, ws.lab64, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost,
                           s));
  if (centroids_out)
    SC_HIP(h, hipMemcpyAsync(centroids_out, ws.cent, (size_t)k * dim * sizeof(double),
                             hipMemcpyDeviceToHost, s));
  SC_HIP(h, hipStreamSynchronize(s));
  if (iterations) *iterations = w[kKgenIters];
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
  return kmeans_general_on(h, host_f64_array(x, n, dim), k, max_iter, metric, tol, init_centroids,
                           labels, centroids_out, iterations);
}

extern "C" int sc_stage_kmeans_general_array(sc_handle h, const sc_array* x, int k, int max_iter,
                                             int metric, double tol,
                                             const double* init_centroids, int64_t* labels,
                                             double* centroids_out, int* iterations) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_kmeans_array(h, x));
  if (!labels || k <= 0) return fail(h, SC_ERR_INVALID, "bad k-means input");
  return kmeans_general_on(h, *x, k, max_iter, metric, tol, init_centroids, labels,
                           centroids_out, iterations);
}

extern "C" int sc_stage_ingest_columns(sc_handle h, const sc_array* x, double* out) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_kmeans_array(h, x));
  if (!out) return fail(h, SC_ERR_INVALID, "out is NULL");
  SC_HIP(h, hipSetDevice(h->device));
  const size_t ld = round_up((int)x->rows, 16), bytes = ld * (size_t)x->cols * sizeof(double);
  SC_TRY(grow(h, h->kgen[kgX], bytes));
  SC_HIP(h, hipMemsetAsync(h->kgen[kgX].p, 0xff, bytes, h->stream));  // NaNs
  SC_TRY(ingest_columns_into(h, *x, ptr<double>(h->kgen[kgX]), (int)ld, h->stream));
  SC_HIP(h, hipMemcpyAsync(out, h->kgen[kgX].p, bytes, hipMemcpyDeviceToHost, h->stream));
  SC_HIP(h, hipStreamSynchronize(h->stream));
  return SC_OK;
}

// ------------------------------------------------------------------------------
// stage/test entries that expose what the k-means kernels compute on the way
// ------------------------------------------------------------------------------
namespace {

struct KmTraceOut {  // any pointer may be null
  double* col_means = nullptr;      // [k]
  int* seeds = nullptr;             // [k]
  int* last_candidates = nullptr;   // [8], the first `trials` of the last k-means++ round
  double* last_potentials = nullptr;  // [8]
  double* lloyd_centroids = nullptr;  // [k * k]
  int64_t* first_labels = nullptr;  // [n]
  double* mean_dist = nullptr;      // [cap]
  int cap = 0;
  int* iterations = nullptr;
  double* centroids = nullptr;      // [k * k]
  int64_t* labels = nullptr;        // [n]
};

// synchronous device -> host copy of `count` T's (the stream has been drained)
template <typename T>
hipError_t fetch(T* dst, const void* src, size_t count) {
  if (!dst || count == 0) return hipSuccess;
  return hipMemcpy(dst, src, count * sizeof(T), hipMemcpyDeviceToHost);
}

// The chain on km[0..count) (n = 0: idle), enqueued by `launch(it_begin, it_count)`: pass 0
// alone, so that the seeds, the Lloyd-step centroids and the first assignment can be read
// before pass 1 overwrites them, then passes 1-3 and four at a time as production does.  A
// member that met its stop rule is read out and goes idle (km[q].n = 0), as in the grouped batch.
template <typename Launch>
int drive_chain_trace(sc_handle h, hipStream_t s, KmGroupItem* km, int count, const KmTraceOut* outs,
                      int max_iter, Launch launch) {
  int running = 0;
  for (int q = 0; q < count; ++q) running += km[q].n > 0;
  std::vector<double> ring(kKmMeand);
  for (int b = 0, c = 1; running > 0;) {
    launch(b, c);
    SC_TRY(check_last(h, "kmeans trace launch"));
    SC_HIP(h, hipStreamSynchronize(s));
    for (int q = 0; q < count; ++q) {
      const int n = km[q].n, k = km[q].k;
      if (n <= 0) continue;
      const KmTraceOut& o = outs[q];
      const KmChainView v = kmeans_chain_view(n, km[q].ws);
      if (b == 0) {
        SC_HIP(h, fetch(o.col_means, v.meang, k));
        SC_HIP(h, fetch(o.seeds, v.seeds, k));
        SC_HIP(h, fetch(o.lloyd_centroids, v.cent0, (size_t)k * k));
        SC_HIP(h, fetch(o.first_labels, km[q].ws.labels64, n));
        if (k > 1) {
          SC_HIP(h, fetch(o.last_candidates, v.cand[(k - 1) & 1], 8));
          if (o.last_potentials) {  // the partial sums in workgroup order, as km_best_trial adds
            std::vector<double> pT((size_t)v.G * 8);
            SC_HIP(h, fetch(pT.data(), v.pT, pT.size()));
            for (int t = 0; t < 8; ++t) {
              double acc = 0.0;
              for (int g = 0; g < v.G; ++g) acc += pT[(size_t)g * 8 + t];
              o.last_potentials[t] = t < km[q].trials ? acc : 0.0;
            }
          }
        }
      }
      if (o.mean_dist) {  // passes whose stop rule this enqueue tested: b - 1 .. b + c - 2
        SC_HIP(h, fetch(ring.data(), v.meand, kKmMeand));
        for (int p = std::max(b, 1) - 1; p < b + c - 1; ++p)
          if (p < o.cap) o.mean_dist[p] = ring[p & (kKmMeand - 1)];
      }
      int info[9] = {0};
      SC_HIP(h, fetch(info, km[q].ws.info, 9));
      if (info[8] == 0) continue;
      if (o.iterations) *o.iterations = info[0];
      SC_HIP(h, fetch(o.centroids, km[q].ws.centroids, (size_t)k * k));
      SC_HIP(h, fetch(o.labels, km[q].ws.labels64, n));
      km[q].n = 0;  // idle from here on
      --running;
    }
    if (running > 0 && b > max_iter + 4)
      return fail(h, SC_ERR_HIP, "k-means chain did not reach its stop rule");
    if (b == 0) {
      b = 1;
      c = 3;
    } else {
      b += c;
      c = 4;
    }
  }
  return SC_OK;
}

struct DeviceSlabs {  // device allocations of one call, freed when it returns
  std::vector<void*> p;
  ~DeviceSlabs() {
    for (void* q : p) hipFree(q);
  }
};

}  // namespace

extern "C" int sc_set_batch_any_metric(sc_handle h, int on) {
  if (!h) return SC_ERR_INVALID;
  h->batch_any_metric = on != 0;
  return SC_OK;
}

extern "C" int sc_stage_kmeans_trace_metric(sc_handle h, const double* e, int n, int k,
                                            int max_iter, int form, int metric, int* form_run,
                                            double* col_means, int* seeds, int* last_candidates,
                                            double* last_potentials, double* lloyd_centroids,
                                            int64_t* first_labels, double* mean_dist,
                                            int mean_dist_cap, int* iterations, double* centroids,
                                            int64_t* labels) {
  if (!h) return SC_ERR_INVALID;
  if (!e || !labels || n <= 0 || k <= 0) return fail(h, SC_ERR_INVALID, "bad k-means input");
  if (form < SC_KMEANS_FORM_AUTO || form > SC_KMEANS_FORM_SINGLE)
    return fail(h, SC_ERR_INVALID, "k-means form: auto, chain or single");
  SC_TRY(check_kmeans_request(h, n, k, max_iter, metric, k > kMaxVectors ? 16 : 8));
  SC_HIP(h, hipSetDevice(h->device));
  SC_TRY(ensure_kmeans(h, n, k));
  SC_TRY(kmeans_seed_state(h, n, k));
  const int first = h->kfirst, trials = h->krnd_trials, lde = round_up(n, 16);
  const bool chain_ok = kmeans_chain_supported(n, k, trials);
  if (form == SC_KMEANS_FORM_CHAIN && !chain_ok)
    return fail(h, SC_ERR_UNSUPPORTED, "the k-means chain does not take this (n, k)");
  // (auto: what kmeans_on_device chooses -- the chain for cosine alone)
  const bool chain = form == SC_KMEANS_FORM_CHAIN ||
                     (form == SC_KMEANS_FORM_AUTO && metric == kKmeansCosine && chain_ok &&
                      !sw::kmeans_single());
  hipStream_t s = h->stream;
  SC_HIP(h, hipMemcpyAsync(h->Eio.p, e, (size_t)n * k * sizeof(double), hipMemcpyHostToDevice, s));
  const double* E = ptr<double>(h->Ek);
  launch_to_colmajor(s, ptr<double>(h->Eio), n, k, ptr<double>(h->Ek), lde);
  const KmeansWorkspace ws = kmeans_workspace(h);
  if (chain) {
    if (form_run) *form_run = 1;
    KmGroupItem km;
    km.ET = E;
    km.lde = lde;
    km.n = n;
    km.k = k;
    km.max_iter = max_iter;
    km.first_center = first;
    km.trials = trials;
    km.metric = metric;
    km.ws = ws;
    KmTraceOut o;
    o.col_means = col_means;
    o.seeds = seeds;
    o.last_candidates = last_candidates;
    o.last_potentials = last_potentials;
    o.lloyd_centroids = lloyd_centroids;
    o.first_labels = first_labels;
    o.mean_dist = mean_dist;
    o.cap = mean_dist_cap;
    o.iterations = iterations;
    o.centroids = centroids;
    o.labels = labels;
    return drive_chain_trace(h, s, &km, 1, &o, max_iter, [&](int b, int c) {
      launch_kmeans_chain(s, E, lde, n, k, max_iter, first, trials, ws, b, c, metric);
    });
  }
  // the single-workgroup kernel: the small form writes its seeds through the optional pointer,
  // the large-k form keeps them in its global workspace
  const bool big = k > kMaxVectors;
  if (form_run) *form_run = big ? 3 : 2;
  if (!big) SC_TRY(grow(h, h->kbigw, (size_t)3 * kMaxVectors * sizeof(int)));
  SC_HIP(h, hipMemsetAsync(h->kinfo.p, 0, 8 * sizeof(int), s));
  launch_kmeans(s, E, lde, n, k, max_iter, first, trials, ws, metric,
                big ? nullptr : ptr<int>(h->kbigw));
  SC_TRY(check_last(h, "kmeans launch"));
  SC_HIP(h, hipStreamSynchronize(s));
  int info[6] = {0};
  SC_HIP(h, fetch(info, h->kinfo.p, 6));
  SC_HIP(h, fetch(seeds, h->kbigw.p, k));
  SC_HIP(h, fetch(centroids, h->kcent.p, (size_t)k * k));
  SC_HIP(h, fetch(labels, h->klab64.p, n));
  if (iterations) *iterations = info[0];
  return SC_OK;
}

extern "C" int sc_stage_kmeans_trace(sc_handle h, const double* e, int n, int k, int max_iter,
                                     int form, int* form_run, double* col_means, int* seeds,
                                     int* last_candidates, double* last_potentials,
                                     double* lloyd_centroids, int64_t* first_labels,
                                     double* mean_dist, int mean_dist_cap, int* iterations,
                                     double* centroids, int64_t* labels) {
  return sc_stage_kmeans_trace_metric(h, e, n, k, max_iter, form, SC_KMEANS_COSINE, form_run,
                                      col_means, seeds, last_candidates, last_potentials,
                                      lloyd_centroids, first_labels, mean_dist, mean_dist_cap,
                                      iterations, centroids, labels);
}

extern "C" int sc_stage_kmeans_trace_group_metric(
    sc_handle h, const double* es, const int* ns, const int* ks, int count, int max_iter,
    int metric, double* col_means, int* seeds, int* last_candidates, double* last_potentials,
    double* lloyd_centroids, int64_t* first_labels, double* mean_dist, int mean_dist_cap,
    int* iterations, double* centroids, int64_t* labels) {
  if (!h) return SC_ERR_INVALID;
  if (!es || !ns || !ks || !labels || count < 1 || count > kGroupMax)
    return fail(h, SC_ERR_INVALID, "bad grouped k-means input");
  SC_HIP(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  KmGroupItem km[kGroupMax];
  KmTraceOut outs[kGroupMax];
  DeviceSlabs slabs;
  std::vector<std::vector<double>> staged(count);  // alive until the first synchronisation
  size_t e_off = 0, row_off = 0;
  for (int z = 0; z < count; ++z) {
    const int n = ns[z], k = ks[z];
    if (n < 0 || (n > 0 && k < 1)) return fail(h, SC_ERR_INVALID, "bad grouped k-means input");
    if (n == 0) continue;  // an idle position
    SC_TRY(check_kmeans_request(h, n, k, max_iter, metric, 8));
    double u_first;
    int trials;
    std::vector<double> rnd;
    kmeans_seed_constants(k, &u_first, &trials, &rnd);
    if (!kmeans_chain_supported(n, k, trials))
      return fail(h, SC_ERR_UNSUPPORTED, "the k-means chain does not take this (n, k)");
    // one slab per member: ET | rnd | closest | xsq | labels64 | centroids | chain | info
    const size_t lde = round_up(n, 16), chain = kmeans_chain_workspace_doubles(n);
    const size_t total = lde * k + rnd.size() + 3 * (size_t)n + 32 * 32 + chain + 8;
    void* slab = nullptr;
    SC_HIP(h, hipMalloc(&slab, total * sizeof(double)));
    slabs.p.push_back(slab);
    SC_HIP(h, hipMemsetAsync(slab, 0, total * sizeof(double), s));
    std::vector<double>& st = staged[z];
    st.assign(lde * k + rnd.size(), 0.0);
    for (int r = 0; r < n; ++r)
      for (int j = 0; j < k; ++j) st[(size_t)j * lde + r] = es[e_off + (size_t)r * k + j];
    std::copy(rnd.begin(), rnd.end(), st.begin() + lde * k);
    SC_HIP(h, hipMemcpyAsync(slab, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice,
                             s));
    double* p = static_cast<double*>(slab);
    KmGroupItem& it = km[z];
    it.ET = p;                 p += lde * k;
    it.ws.rnd = p;             p += rnd.size();
    it.ws.closest = p;         p += n;
    it.ws.xsq = p;             p += n;
    it.ws.labels64 = reinterpret_cast<long long*>(p);  p += n;
    it.ws.centroids = p;       p += 32 * 32;
    it.ws.chain = p;           p += chain;
    it.ws.info = reinterpret_cast<int*>(p);
    it.lde = (int)lde;
    it.n = n;
    it.k = k;
    it.max_iter = max_iter;
    it.first_center = sc_uniform_choice(n, u_first);
    it.trials = trials;
    it.metric = metric;
    KmTraceOut& o = outs[z];
    if (col_means) o.col_means = col_means + (size_t)z * 32;
    if (seeds) o.seeds = seeds + (size_t)z * 32;
    if (last_candidates) o.last_candidates = last_candidates + (size_t)z * 8;
    if (last_potentials) o.last_potentials = last_potentials + (size_t)z * 8;
    if (lloyd_centroids) o.lloyd_centroids = lloyd_centroids + (size_t)z * 32 * 32;
    if (first_labels) o.first_labels = first_labels + row_off;
    if (mean_dist) o.mean_dist = mean_dist + (size_t)z * mean_dist_cap;
    o.cap = mean_dist_cap;
    if (iterations) o.iterations = iterations + z;
    if (centroids) o.centroids = centroids + (size_t)z * 32 * 32;
    o.labels = labels + row_off;
    e_off += (size_t)n * k;
    row_off += (size_t)n;
  }
  SC_HIP(h, hipStreamSynchronize(s));
  const int rc = drive_chain_trace(h, s, km, count, outs, max_iter, [&](int b, int c) {
    launch_kmeans_chain_group(s, km, count, b, c);
  });
  hipStreamSynchronize(s);  // nothing of the slabs is in use when they are freed
  return rc;
}

extern "C" int sc_stage_kmeans_trace_group(sc_handle h, const double* es, const int* ns,
                                           const int* ks, int count, int max_iter,
                                           double* col_means, int* seeds, int* last_candidates,
                                           double* last_potentials, double* lloyd_centroids,
                                           int64_t* first_labels, double* mean_dist,
                                           int mean_dist_cap, int* iterations, double* centroids,
                                           int64_t* labels) {
  return sc_stage_kmeans_trace_group_metric(h, es, ns, ks, count, max_iter, SC_KMEANS_COSINE,
                                            col_means, seeds, last_candidates, last_potentials,
                                            lloyd_centroids, first_labels, mean_dist,
                                            mean_dist_cap, iterations, centroids, labels);
}
