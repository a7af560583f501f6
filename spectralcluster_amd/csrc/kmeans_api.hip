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

static int ensure_kmeans_general(sc_handle h, int n, int dim, int k, int trials,
                                 KmeansGeneralWorkspace* ws) {
  constexpr int TS = kKgenTrialSlots;
  const size_t ld = round_up(n, 16);
  SC_TRY(grow(h, h->kgen[kgX], ld * dim * sizeof(double)));
  SC_TRY(grow(h, h->kgen[kgIo], (size_t)n * dim * sizeof(double)));
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
static int kmeans_on_device(sc_handle h, const double* E, int lde, int n, int k, int max_iter,
                            int64_t* labels, double* centroids_out, int* iterations,
                            int metric = kKmeansCosine) {
  // 8 trial slots up to kMaxVectors centres, 16 in the large-k form
  SC_TRY(check_kmeans_request(h, n, k, max_iter, metric, k > kMaxVectors ? 16 : 8));
  SC_TRY(ensure_kmeans(h, n, k));
  // the RandomState(0) constants are functions of n and k: what the last call left is reused
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

extern "C" int sc_stage_kmeans_metric(sc_handle h, const double* e, int n, int k, int max_iter,
                                      int metric, int64_t* labels, double* centroids_out,
                                      int* iterations) {
  if (!h) return SC_ERR_INVALID;
  if (!e || !labels || n <= 0 || k <= 0) return fail(h, SC_ERR_INVALID, "bad k-means input");
  SC_HIP(h, hipSetDevice(h->device));
  SC_TRY(ensure_kmeans(h, n, k));
  SC_HIP(h, hipMemcpyAsync(h->Eio.p, e, (size_t)n * k * sizeof(double), hipMemcpyHostToDevice,
                           h->stream));
  launch_to_colmajor(h->stream, ptr<double>(h->Eio), n, k, ptr<double>(h->Ek),
                     round_up(n, 16));
  return kmeans_on_device(h, ptr<double>(h->Ek), round_up(n, 16), n, k, max_iter, labels,
                          centroids_out, iterations, metric);
}

extern "C" int sc_stage_kmeans(sc_handle h, const double* e, int n, int k, int max_iter,
                               int64_t* labels, double* centroids_out, int* iterations) {
  return sc_stage_kmeans_metric(h, e, n, k, max_iter, SC_KMEANS_COSINE, labels, centroids_out,
                                iterations);
}

// ------------------------------------------------------------------------------
// an (n, dim) input of any width: run_kmeans with dim != k, CustomKMeans
// ------------------------------------------------------------------------------
extern "C" int sc_stage_kmeans_general(sc_handle h, const double* x, int n, int dim, int k,
                                       int max_iter, int metric, double tol,
                                       const double* init_centroids, int64_t* labels,
                                       double* centroids_out, int* iterations) {
  constexpr int kItersPerSync = 4;  // loop iterations enqueued per host synchronisation
  if (!h) return SC_ERR_INVALID;
  if (!x || !labels || n <= 0 || dim <= 0 || k <= 0)
    return fail(h, SC_ERR_INVALID, "bad k-means input");
  if ((long long)n * dim > 0x7fffffffLL)
    return fail(h, SC_ERR_INVALID, "k-means input larger than 2^31 elements");
  SC_TRY(check_kmeans_request(h, n, k, max_iter, metric, kKgenTrialSlots));
  double u_first;
  int trials;
  std::vector<double> rnd;  // alive until the first synchronisation
  kmeans_seed_constants(k, &u_first, &trials, &rnd);
  SC_HIP(h, hipSetDevice(h->device));
  KmeansGeneralWorkspace ws;
  SC_TRY(ensure_kmeans_general(h, n, dim, k, trials, &ws));
  hipStream_t s = h->stream;

  SC_HIP(h, hipMemcpyAsync(h->kgen[kgIo].p, x, (size_t)n * dim * sizeof(double),
                           hipMemcpyHostToDevice, s));
  launch_to_colmajor(s, ptr<double>(h->kgen[kgIo]), n, dim, ws.X, ws.ld);
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
