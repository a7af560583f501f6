// C ABI (include/spectralcluster_amd.h) and host-side orchestration: device arena,
// the refinement / Laplacian / eigen pipeline, the eigengap scalar loop and the MT19937 stream
// that seeds k-means++.  (Eigen control loops: eig_driver.hip; constraints: constraint_api.hip;
// size reduction and fallback decisions: callers_api.hip; the k-means stage: kmeans_api.hip.)
// Host code only decides and launches; every O(n) or larger computation runs in
// the HIP kernels of this library.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>

#include "handle.h"
#include "host_pool.h"

// ------------------------------------------------------------------------------
// device arena
// ------------------------------------------------------------------------------
int ensure_matrices(sc_handle h, int n, int d, bool affinity_copy) {
  h->krylov_m = 0;  // a new problem: the last solve's state is no longer reported
  h->arnoldi_m = 0;
  const size_t ldn = matrix_ld(n);
  const size_t nn = (size_t)n * ldn * sizeof(double);
  if (affinity_copy) SC_TRY(grow(h, h->A0, nn));
  SC_TRY(grow(h, h->B1, nn));
  SC_TRY(grow(h, h->B2, nn));
  if (d > 0) {
    const size_t ldx = round_up(d, 16);
    SC_TRY(grow(h, h->X, (size_t)n * ldx * sizeof(double)));
    SC_TRY(grow(h, h->Xn, (size_t)n * ldx * sizeof(double)));
  }
  const size_t nv = (size_t)round_up(n, 16) * sizeof(double);
  SC_TRY(grow(h, h->rowmax, nv));
  SC_TRY(grow(h, h->rowsum, nv));
  SC_TRY(grow(h, h->cvec, nv));
  SC_TRY(grow(h, h->pvec, nv));
  SC_TRY(grow(h, h->tvec, nv));
  SC_TRY(grow(h, h->deg, nv));
  SC_TRY(grow(h, h->splitk, gemm_splitk_workspace_bytes()));
  SC_TRY(grow(h, h->dvec, nv));
  SC_TRY(grow(h, h->cut, nv));
  SC_TRY(grow(h, h->cropval, nv));
  SC_TRY(grow(h, h->statp, (size_t)2 * n * gemm_tile_dim(n) * sizeof(double)));
  SC_TRY(grow(h, h->rmpart, (size_t)n * blur_tile_columns(n, 8) * sizeof(double)));
  SC_TRY(grow(h, h->blurw, (2 * SC_MAX_BLUR_RADIUS + 1) * sizeof(double)));
  return SC_OK;
}

// Tile orders of the symmetric GEMM for every tile-grid size up to kTilemapTableMax live in
// one device table built once per handle: a change of n between calls costs no upload and no
// synchronisation (batches of short utterances change it with every call).
int ensure_tilemap(sc_handle h, int n) {
  const int nt = gemm_tile_dim(n);
  if (nt <= kTilemapTableMax) {
    if (!h->tilemap_table.p) {
      std::vector<int2> all, one;
      for (int t = 1; t <= kTilemapTableMax; ++t) {
        h->tilemap_off[t] = (int)all.size();
        gemm_build_sym_tilemap(t, &one);
        all.insert(all.end(), one.begin(), one.end());
      }
      SC_TRY(grow(h, h->tilemap_table, all.size() * sizeof(int2)));
      SC_HIP(h, hipMemcpyAsync(h->tilemap_table.p, all.data(), all.size() * sizeof(int2),
                               hipMemcpyHostToDevice, h->stream));
      SC_HIP(h, hipStreamSynchronize(h->stream));  // `all` is a local
    }
    h->tilemap_cur = ptr<int2>(h->tilemap_table) + h->tilemap_off[nt];
    return SC_OK;
  }
  if (h->tilemap_nt != nt) {
    std::vector<int2> map;
    gemm_build_sym_tilemap(nt, &map);
    SC_TRY(grow(h, h->tilemap, map.size() * sizeof(int2)));
    SC_HIP(h, hipMemcpyAsync(h->tilemap.p, map.data(), map.size() * sizeof(int2),
                             hipMemcpyHostToDevice, h->stream));
    SC_HIP(h, hipStreamSynchronize(h->stream));  // `map` is a local
    h->tilemap_nt = nt;
  }
  h->tilemap_cur = ptr<int2>(h->tilemap);
  return SC_OK;
}

int ensure_eig(sc_handle h, int n) {
  const size_t nq = (size_t)n * kLdq * sizeof(double);
  if (h->Q.bytes < nq) h->krylov_m = h->arnoldi_m = 0;  // (the basis is about to be reallocated)
  SC_TRY(grow(h, h->Q, nq));
  SC_TRY(grow(h, h->Q2, nq));
  SC_TRY(grow(h, h->Vs, (size_t)n * kEigBlock * sizeof(double)));
  SC_TRY(grow(h, h->W, (size_t)n * kEigBlock * sizeof(double)));
  SC_TRY(grow(h, h->partial, std::max((size_t)kProjBlocks * kLdq * kEigBlock,
                                       lz_partial_doubles(n)) * sizeof(double)));
  SC_TRY(grow(h, h->T, (size_t)kLdq * kLdq * sizeof(double)));
  SC_TRY(grow(h, h->Y, (size_t)kLdq * kLdq * sizeof(double)));
  SC_TRY(grow(h, h->Yt, (size_t)kLdq * kLdq * sizeof(double)));
  SC_TRY(grow(h, h->theta, kLdq * sizeof(double)));
  SC_TRY(grow(h, h->resid, kLdq * sizeof(double)));
  SC_TRY(grow(h, h->G, 256 * sizeof(double)));
  SC_TRY(grow(h, h->Rinv, 256 * sizeof(double)));
  SC_TRY(grow(h, h->Hbuf, (size_t)kLdq * kEigBlock * sizeof(double)));
  SC_TRY(grow(h, h->hsq, 16 * sizeof(double)));
  SC_TRY(grow(h, h->colnorm, (size_t)kProjBlocks * kMaxVectors * sizeof(double)));
  if (h->flags.bytes < 16 * sizeof(int)) {
    SC_TRY(grow(h, h->flags, 16 * sizeof(int)));
    SC_HIP(h, hipMemsetAsync(h->flags.p, 0, 16 * sizeof(int), h->stream));
  }
  SC_TRY(grow(h, h->mvsym, matvec_sym_workspace_doubles(n) * sizeof(double)));
  SC_TRY(ensure_vectors(h, n, kMaxCols));
  return SC_OK;
}

// room for `cols` eigenvector columns (the arena holds kMaxCols; a request that selects more
// clusters than that -- the reference has no limit, spectral_clusterer.py:295-299 -- grows it)
int ensure_vectors(sc_handle h, int n, int cols) {
  cols = std::max(cols, kMaxCols);
  SC_TRY(grow(h, h->E, (size_t)round_up(n, 16) * cols * sizeof(double)));
  SC_TRY(grow(h, h->Eio, (size_t)n * cols * sizeof(double)));
  return SC_OK;
}

int ensure_gen(sc_handle h, int n) {
  const size_t ldv = round_up(n, 16);
  const size_t nv = ldv * sizeof(double);
  SC_TRY(grow(h, h->crvec, nv));
  SC_TRY(grow(h, h->thetai, kLdq * sizeof(double)));
  SC_TRY(grow(h, h->Vre, ldv * kGenMax * sizeof(double)));
  SC_TRY(grow(h, h->Vim, ldv * kGenMax * sizeof(double)));
  SC_TRY(grow(h, h->gpart, (size_t)gen_residual_blocks(n) * 32 * sizeof(double)));
  SC_TRY(grow(h, h->gsrc, 16 * sizeof(int)));
  SC_TRY(grow(h, h->genL, (size_t)kGenMax * kGenMax * sizeof(double)));
  return SC_OK;
}

// ------------------------------------------------------------------------------
// library / device
// ------------------------------------------------------------------------------
extern "C" int sc_abi_version(void) { return SC_ABI_VERSION; }
extern "C" int sc_struct_sizes(int* config_bytes, int* diag_bytes) {
  if (config_bytes) *config_bytes = (int)sizeof(sc_config);
  if (diag_bytes) *diag_bytes = (int)sizeof(sc_diag);
  return SC_OK;
}

extern "C" int sc_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

extern "C" int sc_device_info(int device, char* name, int name_len, char* arch,
                              int arch_len, int* compute_units,
                              int64_t* total_mem_bytes) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return SC_ERR_HIP;
  if (name && name_len > 0) snprintf(name, name_len, "%s", prop.name);
  if (arch && arch_len > 0) snprintf(arch, arch_len, "%s", prop.gcnArchName);
  if (compute_units) *compute_units = prop.multiProcessorCount;
  if (total_mem_bytes) *total_mem_bytes = (int64_t)prop.totalGlobalMem;
  return SC_OK;
}

// Hardware queues.  The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES
// hardware queues (4 by default) and streams that share one run one after the other.  The grouped
// batch keeps nine streams busy (three lanes: lockstep chains + two banks of fronts each) and
// picks them so that they share as little as the runtime allows (independent_streams,
// batch_group.hip); with eight queues only two fronts double up.  Config 5, utterances/s:
// 4 queues 3720-4160 from run to run, 6: 3720-3970, 8: 4130-4260, 12 / 16 the same, 24: 3450.
// (The older multi-stream form of predict_batch, one arena and host thread per stream, likes it
// the other way: 2040 with 4 queues, 1820 with 8.)  The library does NOT touch the process
// environment (rounds 2-3 set the variable from a load-time constructor: that changed the queue
// configuration of every other HIP user of the process and depended on the import order): a
// caller that wants the grouped batch at its best exports GPU_MAX_HW_QUEUES=8 before the first
// HIP call of the process -- bench.py does, INTEGRATION.md section 4 says so.

extern "C" int sc_create(int device, sc_handle* out) {
  if (!out) return SC_ERR_INVALID;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return SC_ERR_HIP;
  if (device < 0 || device >= count) return SC_ERR_INVALID;
  sc_handle h = new sc_handle_s();
  h->device = device;
  if (hipSetDevice(device) != hipSuccess ||
      hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return SC_ERR_HIP;
  }
  // stage timers only (never used to synchronise, never to make memory visible): without the
  // system-scope fence a recorded event would otherwise carry -- a cache write-back and
  // invalidate between the stages it separates
  const unsigned ev_flags = hipEventDisableSystemFence;
  for (int i = 0; i < 48; ++i) {
    if (hipEventCreateWithFlags(&h->ev[i], ev_flags) != hipSuccess) {
      delete h;
      return SC_ERR_HIP;
    }
  }
  if (hipHostMalloc(reinterpret_cast<void**>(&h->h_theta), 3 * kLdq * sizeof(double)) !=
          hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&h->h_flags), 16 * sizeof(int)) !=
          hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&h->h_rr),
                    (2 * kHostRRSingle * kHostRRSingle + 64) * sizeof(double)) != hipSuccess) {
    delete h;
    return SC_ERR_HIP;
  }
  *out = h;
  return SC_OK;
}

extern "C" int sc_destroy(sc_handle h) {
  if (!h) return SC_OK;
  for (sc_handle sub : h->pool) sc_destroy(sub);
  h->pool.clear();
  for (sc_handle sub : h->gslots) sc_destroy(sub);
  h->gslots.clear();
  for (sc_handle sub : h->gshort) sc_destroy(sub);
  h->gshort.clear();
  hipSetDevice(h->device);
  hipStreamSynchronize(h->stream);
  DevBuf* bufs[] = {&h->X,     &h->Xn,    &h->A0,     &h->B1,      &h->B2,    &h->rowmax,
                    &h->rowsum, &h->cvec,  &h->pvec,   &h->tvec,    &h->deg,   &h->blurw, &h->blur_tmp, &h->dvec, &h->cut, &h->rmpart, &h->splitk, &h->tilemap, &h->tilemap_table, &h->cropval, &h->statp, &h->crvec, &h->thetai, &h->Vre, &h->Vim, &h->gpart, &h->gsrc, &h->genL, &h->ahc_size, &h->ahc_chain, &h->ahc_Z, &h->ahc_lab, &h->ahc_cent, &h->fb_part, &h->fb_small, &h->sck_slots, &h->sck_part, &h->sck_rec, &h->sck_mats, &h->fb_x, &h->fb_cent, &h->fb_int, &h->Cq, &h->Cband, &h->Cpairs, &h->Cporig, &h->cp[0], &h->cp[1], &h->cp[2], &h->cp[3], &h->cp[4], &h->symflag,
                    &h->Q,     &h->Q2,    &h->Vs,     &h->W,       &h->partial, &h->T,
                    &h->Y,     &h->Yt,    &h->theta,  &h->resid,   &h->G,     &h->Rinv,
                    &h->Hbuf,  &h->hsq,   &h->colnorm, &h->flags,  &h->E,     &h->Ek,   &h->Eio,
                    &h->td_d,  &h->td_e,  &h->td_theta, &h->td_work, &h->td_tau, &h->td_panel, &h->mvsym,
                    &h->kXc,   &h->kxsq,  &h->kclosest, &h->kcand, &h->kenorm, &h->krnd,
                    &h->kcent, &h->klab32, &h->klab64, &h->kinfo, &h->kchain, &h->gkrnd, &h->gpack, &h->gypack, &h->ginfo, &h->glabels, &h->gjtab, &h->gsftab, &h->gswtab,
                    &h->kbig, &h->kbigw, &h->fq, &h->ft32, &h->fy1, &h->fR, &h->fscal, &h->fwords, &h->fcand, &h->fY, &h->fsplit, &h->fypart, &h->frpart, &h->fq2part, &h->fmx64, &h->ftau64, &h->fplan, &h->Xalt, &h->Xstage, &h->gneg, &h->cen_in, &h->cen_out};
  for (DevBuf* b : bufs)
    if (b->p) hipFree(b->p);
  for (DevBuf& b : h->kgen)
    if (b.p) hipFree(b.p);
  for (int i = 0; i < 48; ++i) hipEventDestroy(h->ev[i]);
  if (h->h_theta) hipHostFree(h->h_theta);
  if (h->h_flags) hipHostFree(h->h_flags);
  if (h->h_rr) hipHostFree(h->h_rr);
  if (h->h_free) hipHostFree(h->h_free);
  if (h->h_reduce) hipHostFree(h->h_reduce);
  if (h->h_sck) hipHostFree(h->h_sck);
  if (h->sync_ev) hipEventDestroy(h->sync_ev);
  for (int b = 0; b < kGroupBanks; ++b) {
    if (h->gbank_ev[b]) hipEventDestroy(h->gbank_ev[b]);
    if (h->gbank_stream[b]) hipStreamDestroy(h->gbank_stream[b]);
  }
  if (h->gchain_stream) hipStreamDestroy(h->gchain_stream);
  if (h->copy_stream) hipStreamDestroy(h->copy_stream);
  if (h->gcheck_ev) hipEventDestroy(h->gcheck_ev);
  for (sc_handle lane : h->glanes) sc_destroy(lane);
  h->glanes.clear();
  delete h->gpool;
  if (h->h_gpack) hipHostFree(h->h_gpack);
  if (h->h_gypack) hipHostFree(h->h_gypack);
  if (h->h_gjtab) hipHostFree(h->h_gjtab);
  if (h->h_gsftab) hipHostFree(h->h_gsftab);
  if (h->h_gswtab) hipHostFree(h->h_gswtab);
  if (h->gsftab_ev) hipEventDestroy(h->gsftab_ev);
  if (h->h_ginfo) hipHostFree(h->h_ginfo);
  if (h->h_glabels) hipHostFree(h->h_glabels);
  hipStreamDestroy(h->stream);
  delete h;
  return SC_OK;
}

extern "C" const char* sc_last_error(sc_handle h) { return h ? h->err.c_str() : ""; }

extern "C" int sc_synchronize(sc_handle h) {
  if (!h) return SC_ERR_INVALID;
  SC_HIP(h, hipStreamSynchronize(h->stream));
  return SC_OK;
}

extern "C" int sc_reserve(sc_handle h, int n_max, int d_max) {
  if (!h || n_max <= 0 || d_max < 0) return SC_ERR_INVALID;
  SC_HIP(h, hipSetDevice(h->device));
  SC_TRY(ensure_matrices(h, n_max, d_max));
  SC_TRY(ensure_eig(h, n_max));
  SC_TRY(ensure_kmeans(h, n_max));
  return SC_OK;
}

// numpy pairwise sum for short arrays (n < 128): 8 running sums, then the tail
static double numpy_sum_short(const double* a, int n) {
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

extern "C" int sc_gaussian_weights(double sigma, int32_t* radius, double* weights) {
  if (!radius || !weights || !(sigma >= 0.0)) return SC_ERR_INVALID;
  if (sigma <= 1e-15) {  // gaussian_filter skips the axis: plain copy
    *radius = 0;
    weights[0] = 1.0;
    return SC_OK;
  }
  const int r = (int)(4.0 * sigma + 0.5);  // truncate = 4.0
  if (r > SC_MAX_BLUR_RADIUS) return SC_ERR_UNSUPPORTED;
  const double s2 = sigma * sigma;
  for (int x = -r; x <= r; ++x) weights[x + r] = std::exp(-0.5 / s2 * (double)(x * x));
  const double sum = numpy_sum_short(weights, 2 * r + 1);
  for (int i = 0; i < 2 * r + 1; ++i) weights[i] /= sum;
  *radius = r;
  return SC_OK;
}

// Weights of a Gaussian blur whose radius does not fit sc_config (sigma > 8: radius =
// int(4 sigma + .5) > SC_MAX_BLUR_RADIUS; the reference has no limit, refinement.py:154-162).
// They stay resident in the handle; a config with blur_radius == radius then uses them.
extern "C" int sc_set_blur_weights(sc_handle h, int radius, const double* weights) {
  if (!h) return SC_ERR_INVALID;
  if (radius <= SC_MAX_BLUR_RADIUS || radius > (1 << 20) || !weights)
    return fail(h, SC_ERR_INVALID, "sc_set_blur_weights: radius must exceed 32; weights 2 r + 1");
  h->blur_ext.assign(weights, weights + 2 * (size_t)radius + 1);
  return SC_OK;
}

extern "C" int sc_config_default(sc_config* cfg) {
  if (!cfg) return SC_ERR_INVALID;
  memset(cfg, 0, sizeof(*cfg));
  sc_gaussian_weights(1.0, &cfg->blur_radius, cfg->blur_weights);
  cfg->p_percentile = 0.95;
  cfg->soft_multiplier = 0.01;
  cfg->threshold_type = SC_THRESHOLD_ROW_MAX;
  cfg->symmetrize_type = SC_SYMMETRIZE_MAX;
  cfg->laplacian_type = SC_LAPLACIAN_NONE;
  cfg->stop_eigenvalue = 1e-2;
  cfg->eigengap_type = SC_EIGENGAP_RATIO;
  cfg->max_iter = 300;
  cfg->constraint_name = SC_CONSTRAINT_NONE;
  cfg->integration_type = SC_INTEGRATION_MAX;
  cfg->constraint_alpha = 0.6;  // constraint.py:41
  return SC_OK;
}

// ------------------------------------------------------------------------------
// E2: eigengap (reference utils.py:74-130)
// ------------------------------------------------------------------------------
void eigengap_core(const double* w, int count, int max_clusters,
                          double stop_eigenvalue, int eigengap_type, int descend,
                          double wmax, int* n_clusters, double* max_delta) {
  const double eps = 1e-10;  // utils.py:7
  double best = 0.0;
  int best_k = 0;
  int end = count;
  if (max_clusters > 0 && max_clusters + 1 < end) end = max_clusters + 1;
  if (descend) {
    for (int i = 1; i < end; ++i) {
      if (w[i - 1] < stop_eigenvalue) break;
      const double d = eigengap_type == SC_EIGENGAP_RATIO ? w[i - 1] / (w[i] + eps)
                                                          : (w[i - 1] - w[i]) / wmax;
      if (d > best) { best = d; best_k = i; }
    }
  } else {
    for (int i = 1; i < end - 1; ++i) {
      const double d = eigengap_type == SC_EIGENGAP_RATIO ? w[i + 1] / (w[i] + eps)
                                                          : (w[i + 1] - w[i]) / wmax;
      if (d > best) { best = d; best_k = i + 1; }
    }
  }
  *n_clusters = best_k;
  *max_delta = best;
}

extern "C" int sc_eigengap(const double* w, int count, int max_clusters,
                           double stop_eigenvalue, int eigengap_type, int descend,
                           int* n_clusters, double* max_delta) {
  if (!w || count < 0 || !n_clusters || !max_delta) return SC_ERR_INVALID;
  if (eigengap_type != SC_EIGENGAP_RATIO && eigengap_type != SC_EIGENGAP_NORMALIZED_DIFF)
    return SC_ERR_INVALID;
  double wmax = 0.0;
  if (count > 0) {
    wmax = w[0];
    for (int i = 1; i < count; ++i) wmax = w[i] > wmax ? w[i] : wmax;  // np.max(eigenvalues)
  }
  eigengap_core(w, count, max_clusters, stop_eigenvalue, eigengap_type, descend, wmax,
                n_clusters, max_delta);
  return SC_OK;
}

// ------------------------------------------------------------------------------
// MT19937 as numpy's legacy RandomState(seed) drives it (k-means++ seeding)
// ------------------------------------------------------------------------------
namespace {
struct Mt19937 {
  uint32_t mt[624];
  int pos;
  explicit Mt19937(uint32_t seed) {
    mt[0] = seed;
    for (int i = 1; i < 624; ++i)
      mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    pos = 624;
  }
  void twist() {
    for (int k = 0; k < 624; ++k) {
      const uint32_t y = (mt[k] & 0x80000000u) | (mt[(k + 1) % 624] & 0x7fffffffu);
      uint32_t v = mt[(k + 397) % 624] ^ (y >> 1);
      if (y & 1u) v ^= 0x9908b0dfu;
      mt[k] = v;
    }
    pos = 0;
  }
  uint32_t next_u32() {
    if (pos >= 624) twist();
    uint32_t y = mt[pos++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
  }
  double next_double() {
    const uint32_t a = next_u32() >> 5, b = next_u32() >> 6;
    return (a * 67108864.0 + b) / 9007199254740992.0;
  }
};
}  // namespace

extern "C" int sc_random_state_doubles(uint32_t seed, int count, double* out) {
  if (!out || count < 0) return SC_ERR_INVALID;
  Mt19937 rng(seed);
  for (int i = 0; i < count; ++i) out[i] = rng.next_double();
  return SC_OK;
}

extern "C" int sc_uniform_choice(int n, double u) {
  if (n <= 0) return SC_ERR_INVALID;
  // cdf = cumsum(p) in order, normalised by its last entry: the same running sums twice
  // instead of an n-element array
  const double p = 1.0 / (double)n;
  double last = 0.0;
  for (int i = 0; i < n; ++i) last += p;
  double run = 0.0;
  for (int i = 0; i < n; ++i) {
    run += p;
    if (run / last > u) return i;  // searchsorted(..., side="right")
  }
  return n - 1;
}

// ------------------------------------------------------------------------------
// data movement helpers
// ------------------------------------------------------------------------------
int h2d_matrix(sc_handle h, const double* src, int rows, int cols, double* dst,
                      int ld) {
  SC_HIP(h, hipMemcpy2DAsync(dst, (size_t)ld * sizeof(double), src,
                             (size_t)cols * sizeof(double), (size_t)cols * sizeof(double),
                             rows, hipMemcpyHostToDevice, h->stream));
  return SC_OK;
}
int d2h_matrix(sc_handle h, const double* src, int ld, int rows, int cols,
                      double* dst) {
  SC_HIP(h, hipMemcpy2DAsync(dst, (size_t)cols * sizeof(double), src,
                             (size_t)ld * sizeof(double), (size_t)cols * sizeof(double),
                             rows, hipMemcpyDeviceToHost, h->stream));
  SC_HIP(h, hipStreamSynchronize(h->stream));
  return SC_OK;
}

int validate_config(sc_handle h, const sc_config* cfg) {
  if (!cfg) return fail(h, SC_ERR_INVALID, "config is NULL");
  if (cfg->n_ops < 0 || cfg->n_ops > SC_MAX_OPS)
    return fail(h, SC_ERR_INVALID, "n_ops out of range");
  for (int i = 0; i < cfg->n_ops; ++i)
    if (cfg->ops[i] < SC_OP_CROP_DIAGONAL || cfg->ops[i] > SC_OP_ROW_WISE_NORMALIZE)
      return fail(h, SC_ERR_INVALID, "Unknown refinement operation");
  if (cfg->blur_radius < 0) return fail(h, SC_ERR_INVALID, "gaussian blur radius < 0");
  if (cfg->blur_radius > SC_MAX_BLUR_RADIUS) {
    if (!h || (int)h->blur_ext.size() != 2 * cfg->blur_radius + 1)
      return fail(h, SC_ERR_UNSUPPORTED,
                  "gaussian blur radius > 32: upload its weights with sc_set_blur_weights first");
    // the radius travels in the config, the weights live in the handle: the config names WHICH
    // weights it means by their central 2 * 32 + 1 entries (two sigmas can share a radius)
    const double* centre = h->blur_ext.data() + (cfg->blur_radius - SC_MAX_BLUR_RADIUS);
    if (memcmp(centre, cfg->blur_weights, (2 * SC_MAX_BLUR_RADIUS + 1) * sizeof(double)) != 0)
      return fail(h, SC_ERR_UNSUPPORTED,
                  "gaussian blur radius > 32: the weights resident in the handle are not the "
                  "ones this config was built with (sc_set_blur_weights them again)");
  }
  if (cfg->laplacian_type < SC_LAPLACIAN_NONE || cfg->laplacian_type > SC_LAPLACIAN_GRAPH_CUT)
    return fail(h, SC_ERR_INVALID, "laplacian_type must be a LaplacianType");
  if (cfg->eigengap_type != SC_EIGENGAP_RATIO &&
      cfg->eigengap_type != SC_EIGENGAP_NORMALIZED_DIFF)
    return fail(h, SC_ERR_INVALID, "eigengap_type must be a EigenGapType");
  if (cfg->symmetrize_type != SC_SYMMETRIZE_MAX &&
      cfg->symmetrize_type != SC_SYMMETRIZE_AVERAGE)
    return fail(h, SC_ERR_INVALID, "Unsupported symmetrize_type.");
  if (cfg->threshold_type != SC_THRESHOLD_ROW_MAX &&
      cfg->threshold_type != SC_THRESHOLD_PERCENTILE)
    return fail(h, SC_ERR_INVALID, "Unsupported thresholding_type");
  return SC_OK;
}

// device copy of the blur weights; the upload is skipped while they do not change
int upload_blur_weights(sc_handle h, const sc_config* cfg) {
  const int count = 2 * cfg->blur_radius + 1;
  if (cfg->blur_radius > SC_MAX_BLUR_RADIUS) {  // resident weights of sc_set_blur_weights
    SC_TRY(grow(h, h->blurw, (size_t)count * sizeof(double)));
    h->blurw_radius = -1;  // (the small-radius cache no longer describes the buffer)
    SC_HIP(h, hipMemcpyAsync(h->blurw.p, h->blur_ext.data(), count * sizeof(double),
                             hipMemcpyHostToDevice, h->stream));
    return SC_OK;
  }
  if (h->blurw_radius == cfg->blur_radius &&
      memcmp(h->blurw_host, cfg->blur_weights, count * sizeof(double)) == 0)
    return SC_OK;
  memcpy(h->blurw_host, cfg->blur_weights, count * sizeof(double));
  h->blurw_radius = cfg->blur_radius;
  SC_HIP(h, hipMemcpyAsync(h->blurw.p, h->blurw_host, count * sizeof(double),
                           hipMemcpyHostToDevice, h->stream));
  return SC_OK;
}

// run one refinement op `in` -> `out` (distinct buffers)
int run_refine_op(sc_handle h, int op, const sc_config* cfg, const double* in, double* out, int n,
                  int ld) {
  hipStream_t s = h->stream;
  switch (op) {
    case SC_OP_CROP_DIAGONAL:
      launch_crop_diagonal(s, in, out, n, ld);
      break;
    case SC_OP_GAUSSIAN_BLUR:
      if (cfg->blur_radius > 0) SC_TRY(upload_blur_weights(h, cfg));
      if (cfg->blur_radius > SC_MAX_BLUR_RADIUS) {
        SC_TRY(grow(h, h->blur_tmp, (size_t)n * ld * sizeof(double)));
        launch_gaussian_blur_any_radius(s, in, ptr<double>(h->blur_tmp), out, n, ld,
                                        cfg->blur_radius, ptr<double>(h->blurw));
      } else {
        // (launch_gaussian_blur, with the kernel it takes reported)
        launch_gaussian_blur_fused(s, in, out, n, ld, cfg->blur_radius, ptr<double>(h->blurw),
                                   nullptr, nullptr, &h->last_blur);
      }
      break;
    case SC_OP_ROW_WISE_THRESHOLD:
      if (cfg->threshold_type == SC_THRESHOLD_PERCENTILE) {
        launch_cut_percentile(s, in, n, ld, cfg->p_percentile, ptr<double>(h->cut),
                              cfg->preserve_diagonal);
        launch_row_threshold_cut(s, in, out, n, ld, ptr<double>(h->cut), cfg->soft_multiplier,
                                 cfg->binarize, cfg->preserve_diagonal);
      } else {
        launch_row_threshold(s, in, out, n, ld, cfg->p_percentile, cfg->soft_multiplier,
                             cfg->binarize, cfg->preserve_diagonal);
      }
      break;
    case SC_OP_SYMMETRIZE:
      launch_symmetrize(s, in, out, n, ld, cfg->symmetrize_type);
      break;
    case SC_OP_DIFFUSE:
      SC_TRY(ensure_tilemap(h, n));
      launch_gemm_nt(s, in, ld, in, ld, out, ld, n, n, n, kEpiNone, true, ptr<double>(h->splitk),
                     h->tilemap_cur);
      break;
    case SC_OP_ROW_WISE_NORMALIZE:
      launch_row_normalize(s, in, out, n, ld);
      break;
    default:
      return fail(h, SC_ERR_INVALID, "Unknown refinement operation");
  }
  return check_last(h, "refinement kernel launch");
}

// ------------------------------------------------------------------------------
// embeddings / affinity
// ------------------------------------------------------------------------------
// (sc_set_embeddings and the other entry points that take embeddings in: ingest.hip)
extern "C" int sc_compute_affinity(sc_handle h) {
  if (!h) return SC_ERR_INVALID;
  if (!h->have_x) return fail(h, SC_ERR_INVALID, "no embeddings resident");
  SC_HIP(h, hipSetDevice(h->device));
  SC_TRY(ensure_tilemap(h, h->n));
  SC_TRY(grow(h, h->symflag, 16));
  SC_HIP(h, hipMemsetAsync(ptr<int>(h->symflag) + 1, 0, sizeof(int), h->stream));
  launch_normalize_rows(h->stream, ptr<double>(h->X), h->ldx, h->n, h->d,
                        ptr<double>(h->Xn), ptr<int>(h->symflag) + 1);
  h->affinity_from_embeddings = true;
  // CropDiagonal's fill value (max_{j != i} A_ij, >= 0) comes out of the GEMM epilogue
  GemmRowStats rs{2, ptr<double>(h->statp), nullptr, ptr<double>(h->cropval), nullptr};
  h->aff_ev[0] = h->aff_ev[1] = -1;
  // (level 1 too since round 6: with the digit product cut to its surviving tiles this GEMM is
  //  the longest kernel of an ICASSP call, and bench.py's roofline wants its time from the
  //  timed region itself)
  if (h->profile_level >= 1) ev_rec(h, &h->aff_ev[0]);
  launch_gemm_nt(h->stream, ptr<double>(h->Xn), h->ldx, ptr<double>(h->Xn), h->ldx,
                 ptr<double>(h->A0), h->ldn, h->n, h->n, h->d, kEpiAffinity, true,
                 ptr<double>(h->splitk), h->tilemap_cur, &rs);
  if (h->profile_level >= 1) ev_rec(h, &h->aff_ev[1]);
  SC_TRY(check_last(h, "affinity launch"));
  h->have_affinity = true;
  h->have_cropval = true;
  h->affinity_symmetric = true;
  h->constraint_applied = false;
  h->n_vec = 0;
  h->sweep_slot.clear();
  return SC_OK;
}

extern "C" int sc_set_affinity(sc_handle h, const double* a, int n) {
  if (!h) return SC_ERR_INVALID;
  if (!a || n <= 0) return fail(h, SC_ERR_INVALID, "affinity must be (n, n)");
  SC_HIP(h, hipSetDevice(h->device));
  SC_TRY(ensure_matrices(h, n, 0));
  h->n = n;
  h->ldn = matrix_ld(n);
  h->have_x = false;
  h->n_vec = 0;
  h->sweep_slot.clear();
  SC_TRY(h2d_matrix(h, a, n, n, ptr<double>(h->A0), h->ldn));
  SC_TRY(device_is_symmetric(h, ptr<double>(h->A0), n, h->ldn, &h->affinity_symmetric));
  h->have_affinity = true;
  h->have_cropval = false;
  h->constraint_applied = false;
  h->affinity_from_embeddings = false;
  return SC_OK;
}

// ------------------------------------------------------------------------------
// _compute_eigenvectors_ncluster
// ------------------------------------------------------------------------------

EigRequest make_eig_request(const sc_config* cfg) {
  EigRequest rq;
  rq.descend = (cfg->laplacian_type == SC_LAPLACIAN_NONE ||
                cfg->laplacian_type == SC_LAPLACIAN_AFFINITY);
  rq.max_clusters = cfg->max_clusters;
  rq.min_clusters = cfg->min_clusters;
  rq.stop_eigenvalue = cfg->stop_eigenvalue;
  rq.eigengap_type = cfg->eigengap_type;
  rq.use_stop = rq.descend;  // spectral_clusterer.py:163-167: not passed when ascending
  rq.value_tol = cfg->eig_value_tol > 0 ? cfg->eig_value_tol : 1e-6;
  rq.vector_tol = cfg->eig_vector_tol > 0 ? cfg->eig_vector_tol : 1e-10;
  rq.max_cycles = cfg->eig_max_cycles > 0 ? cfg->eig_max_cycles : (cfg->eig_max_cycles < 0 ? 0 : 40);
  rq.fixed_count = 0;
  return rq;
}

// `front_only`: stop after the refinement and the scaling vectors (everything before the
// eigensolver, no host synchronisation) and say where the refined matrix is -- the grouped
// batch (batch_group.hip) solves several such problems in lockstep from there.
// stage timers of a call whose events were still in flight when eig_ncluster_impl returned
static void resolve_stage_times(sc_handle h, sc_diag* diag) {
  StageEvents& t = h->stage_events;
  if (!t.pending) return;
  t.pending = false;
  if (!diag) return;
  float dms = 0.f;
  for (int i = 0; i < t.n_diffuse; ++i) dms += ev_ms(h, t.diffuse[i][0], t.diffuse[i][1]);
  diag->stage_ms[SC_STAGE_DIFFUSE] = dms;
  diag->stage_ms[SC_STAGE_REFINE] = ev_ms(h, t.begin, t.after_refine) - dms;
  diag->stage_ms[SC_STAGE_SCALING] = ev_ms(h, t.after_refine, t.after_scaling);
  diag->stage_ms[SC_STAGE_EIG] = ev_ms(h, t.after_scaling, t.after_eig);
  if (t.free_path) {
    diag->stage_ms[SC_STAGE_FREE_QUANTIZE] = ev_ms(h, h->free_ev[0], h->free_ev[1]);
    diag->stage_ms[SC_STAGE_FREE_PRODUCT] = ev_ms(h, h->free_ev[1], h->free_ev[2]);
    diag->stage_ms[SC_STAGE_FREE_SCAN] = ev_ms(h, h->free_ev[2], h->free_ev[3]);
    diag->stage_ms[SC_STAGE_FREE_STATS] = ev_ms(h, h->free_ev[3], h->free_ev[4]);
  }
  if (t.fine) {
    diag->stage_ms[SC_STAGE_BLUR] = ev_ms(h, t.blur[0], t.blur[1]);
    diag->stage_ms[SC_STAGE_THRESHOLD_SYM] = ev_ms(h, t.thr[0], t.thr[1]);
    float mv = 0.f;
    for (int i = 0; i < h->n_mv_ev; ++i) mv += ev_ms(h, h->mv_ev[i][0], h->mv_ev[i][1]);
    diag->stage_ms[SC_STAGE_MATVEC] = mv;
  }
}

// `defer_timing`: return without waiting for the stream (the caller enqueues k-means right
// behind the Ritz vectors and resolves the stage timers after its own synchronisation)
int eig_ncluster_impl(sc_handle h, const sc_config* cfg, sc_diag* diag, FrontResult* front_only,
                      const FrontResult* resume, bool defer_timing,
                      FrontResult* stop_before_solver) {
  const int n = h->n, ld = h->ldn;
  hipStream_t s = h->stream;
  const double* cur = ptr<double>(h->A0);
  double* bufs[2] = {ptr<double>(h->B1), ptr<double>(h->B2)};
  int which = 0;
  bool symmetric = h->affinity_symmetric;  // cosine affinity: always
  const bool constrain_after = constraint_active(h, cfg, false);
  bool folded_rownorm = false;
  int e_begin, e_after_refine;
  const bool fine = h->profile_level >= 2;
  int eb0 = -1, eb1 = -1, et0 = -1, et1 = -1;  // blur / threshold+symmetrize (last of each)
  h->n_mv_ev = 0;
  bool free_path = false;
  const double* amax_of = nullptr;  // matrix whose max|a| h->fscal[0] bounds (matrix-free Diffuse)
  const double* digits_of = nullptr;  // ... whose digits the threshold pass has already written
  float diffuse_ms_events[SC_MAX_OPS][2];
  int n_diffuse = 0;
  ev_rec(h, &e_begin);
  // Fusions (identical arithmetic, fewer passes over the n x n matrix):
  //   CropDiagonal + GaussianBlur      -> crop value vector + blur with diagonal override
  //   GaussianBlur -> RowWiseThreshold -> row maxima come out of the blur epilogue
  //   RowWiseThreshold(RowMax) + Symmetrize -> one tile-pair kernel
  const bool blur_fast = (cfg->blur_radius == 4 || cfg->blur_radius == 8) && n >= 128;
  const double* pending_diag = nullptr;
  bool have_partials = false;
  bool have_row_stats = false;
  int crop_source = 0, cut_kernel = 0;  // (what sc_stage_front reports)
  h->last_blur = BlurLaunch();
  if (resume) {
    cur = resume->matrix;
    symmetric = resume->symmetric;
    folded_rownorm = resume->folded_rownorm;
    which = resume->scratch == bufs[0] ? 0 : 1;
    // resume->free_op: the front left A, not S = A A^T (a matrix-free member of a batch group
    // handed back by the lockstep solve): sym_topk has to apply it twice, and its first host
    // sync looks at the rows the candidate search could not prune (h_free came back behind the
    // group's statistics; free_group_end left free_checked false).  (The stage timers of the
    // statistics belong to the front.)
    if (resume->free_op) h->free_checked = false;
  }
  for (int i = 0; i < (resume ? 0 : cfg->n_ops); ++i) {
    const int op = cfg->ops[i];
    const int next = i + 1 < cfg->n_ops ? cfg->ops[i + 1] : 0;
    const int next2 = i + 2 < cfg->n_ops ? cfg->ops[i + 2] : 0;
    const bool thr_sym_fusable = true;  // RowMax or Percentile, with or without diagonal
    const bool partials_usable = cfg->threshold_type == SC_THRESHOLD_ROW_MAX &&
                                 !cfg->preserve_diagonal;
    if (op == SC_OP_ROW_WISE_NORMALIZE && symmetric && i == cfg->n_ops - 1 &&
        !constrain_after) {
      folded_rownorm = true;  // W = diag(1/rowmax) S is never materialised
      continue;
    }
    if (op == SC_OP_CROP_DIAGONAL && next == SC_OP_GAUSSIAN_BLUR && blur_fast) {
      if (cur == ptr<double>(h->A0) && h->have_cropval) {
        pending_diag = ptr<double>(h->cropval);
        crop_source = 1;
      } else {
        launch_crop_value(s, cur, n, ld, ptr<double>(h->dvec));
        pending_diag = ptr<double>(h->dvec);
        crop_source = 2;
      }
      have_partials = false;
      continue;  // symmetry unchanged; the blur applies the new diagonal on load
    }
    double* out = bufs[which];
    which ^= 1;
    int e0 = -1, e1 = -1;
    bool keep_cur = false;
    if (op == SC_OP_DIFFUSE) ev_rec(h, &e0);
    if (op == SC_OP_GAUSSIAN_BLUR && blur_fast) {
      const bool want = next == SC_OP_ROW_WISE_THRESHOLD && next2 == SC_OP_SYMMETRIZE &&
                        partials_usable;
      SC_TRY(upload_blur_weights(h, cfg));
      if (fine) ev_rec(h, &eb0);
      have_partials = launch_gaussian_blur_fused(s, cur, out, n, ld, cfg->blur_radius,
                                                 ptr<double>(h->blurw), pending_diag,
                                                 want ? ptr<double>(h->rmpart) : nullptr,
                                                 &h->last_blur);
      if (fine) ev_rec(h, &eb1);
      pending_diag = nullptr;
      SC_TRY(check_last(h, "blur launch"));
    } else if (op == SC_OP_ROW_WISE_THRESHOLD && next == SC_OP_SYMMETRIZE && thr_sym_fusable) {
      if (cfg->threshold_type == SC_THRESHOLD_PERCENTILE)
        launch_cut_percentile(s, cur, n, ld, cfg->p_percentile, ptr<double>(h->cut),
                              cfg->preserve_diagonal);
      else if (have_partials && partials_usable)
        launch_cut_from_partials(s, ptr<double>(h->rmpart), n,
                                 blur_tile_columns(n, cfg->blur_radius),
                                 cfg->p_percentile, ptr<double>(h->cut));
      else
        launch_cut_from_rows(s, cur, n, ld, cfg->p_percentile, ptr<double>(h->cut),
                             cfg->preserve_diagonal);
      cut_kernel = cfg->threshold_type == SC_THRESHOLD_PERCENTILE
                       ? 3 : (have_partials && partials_usable ? 1 : 2);
      // the matrix-free Diffuse quantises this pass's result: when it is non-negative by
      // construction (cosine affinity, no constraint applied to it) and thresholded by RowMax
      // with a multiplier in [0, 1], its maximum is known from the cut vector ...
      const bool amax_known =
          cfg->threshold_type == SC_THRESHOLD_ROW_MAX && h->affinity_from_embeddings &&
          !h->constraint_applied && cfg->p_percentile > 0.0 && cfg->soft_multiplier >= 0.0 &&
          cfg->soft_multiplier <= 1.0 && i + 2 < cfg->n_ops && cfg->ops[i + 2] == SC_OP_DIFFUSE &&
          free_diffuse_wanted(h, cfg, n, make_eig_request(cfg));
      // ... and when that Diffuse will take the matrix-free route (the conditions of its branch
      // below), this pass writes the digits and row partials too: no quantiser pass
      const bool fuse_digits =
          amax_known && !constrain_after && !front_only &&
          (i + 2 == cfg->n_ops - 1 ||
           (i + 2 == cfg->n_ops - 2 && cfg->ops[i + 3] == SC_OP_ROW_WISE_NORMALIZE));
      const double amax_floor = (cfg->binarize || cfg->preserve_diagonal) ? 1.0 : 0.0;
      if (fuse_digits)
        SC_TRY(free_fused_prepare(h, s, n, ptr<double>(h->cut), cfg->p_percentile, amax_floor));
      if (fine) ev_rec(h, &et0);
      if (fuse_digits)
        launch_threshold_symmetrize_digits(s, cur, out, n, ld, ptr<double>(h->cut),
                                           cfg->soft_multiplier, cfg->binarize,
                                           cfg->symmetrize_type, cfg->preserve_diagonal,
                                           ptr<signed char>(h->fq), ptr<double>(h->fscal),
                                           ptr<double>(h->fypart), ptr<int>(h->frpart),
                                           ptr<double>(h->fq2part), ptr<double>(h->fmx64));
      else
        launch_threshold_symmetrize(s, cur, out, n, ld, ptr<double>(h->cut),
                                    cfg->soft_multiplier, cfg->binarize, cfg->symmetrize_type,
                                    cfg->preserve_diagonal);
      if (fine) ev_rec(h, &et1);
      SC_TRY(check_last(h, "threshold+symmetrize launch"));
      if (fuse_digits) {
        amax_of = out;
        digits_of = out;
      } else if (amax_known) {
        SC_TRY(ensure_free(h, n));
        launch_free_amax_from_cut(s, ptr<double>(h->cut), n, cfg->p_percentile, amax_floor,
                                  ptr<double>(h->fscal));
        amax_of = out;
      }
      have_partials = false;
      cur = out;
      symmetric = true;
      ++i;  // Symmetrize consumed
      continue;
    } else if (op == SC_OP_DIFFUSE && symmetric && !constrain_after && !front_only &&
               cur != ptr<double>(h->A0) &&
               (i == cfg->n_ops - 1 || (i == cfg->n_ops - 2 && next == SC_OP_ROW_WISE_NORMALIZE)) &&
               free_diffuse_wanted(h, cfg, n, make_eig_request(cfg))) {
      // Matrix-free Diffuse (free_api.hip): nothing after this op reads an entry of
      // S = A A^T -- only rowmax(S) (the RowWiseNormalize fold), rowsum(S) (the Laplacian) and
      // S V (the eigensolver).  `cur` stays the symmetric A; `out` stays free.
      SC_TRY(ensure_eig(h, n));
      SC_TRY(free_diffuse_stats(h, cur, ld, n, amax_of == cur, digits_of == cur));
      free_path = true;
      have_row_stats = true;
      have_partials = false;
      keep_cur = true;
      which ^= 1;
    } else if (op == SC_OP_DIFFUSE) {
      // when Diffuse is the last materialised matrix its row max / row sum (for the
      // RowWiseNormalize fold and the Laplacian scaling) come out of the GEMM epilogue
      const bool last = i == cfg->n_ops - 1 ||
                        (i == cfg->n_ops - 2 && next == SC_OP_ROW_WISE_NORMALIZE);
      GemmRowStats rs{1, ptr<double>(h->statp), ptr<double>(h->statp) + (size_t)n * gemm_tile_dim(n),
                      ptr<double>(h->rowmax), ptr<double>(h->rowsum)};
      SC_TRY(ensure_tilemap(h, n));
      launch_gemm_nt(s, cur, ld, cur, ld, out, ld, n, n, n, kEpiNone, true,
                     ptr<double>(h->splitk), h->tilemap_cur, last ? &rs : nullptr);
      SC_TRY(check_last(h, "diffuse launch"));
      have_row_stats = last;
      have_partials = false;
    } else {
      SC_TRY(run_refine_op(h, op, cfg, cur, out, n, ld));
      have_partials = false;
    }
    if (op == SC_OP_DIFFUSE) {
      ev_rec(h, &e1);
      diffuse_ms_events[n_diffuse][0] = (float)e0;
      diffuse_ms_events[n_diffuse][1] = (float)e1;
      ++n_diffuse;
    }
    if (!keep_cur) cur = out;
    switch (op) {
      case SC_OP_CROP_DIAGONAL:
      case SC_OP_GAUSSIAN_BLUR:
        break;  // symmetry preserved (blur: up to rounding)
      case SC_OP_ROW_WISE_THRESHOLD:
      case SC_OP_ROW_WISE_NORMALIZE:
        symmetric = false;
        break;
      case SC_OP_SYMMETRIZE:
      case SC_OP_DIFFUSE:
        symmetric = true;
        break;
    }
  }
  if (constrain_after && !resume) {  // spectral_clusterer.py:137-142
    if (h->qn != n)
      return fail(h, SC_ERR_INVALID,
                  "affinity and constraint matrix must have the same shape");
    double* out = bufs[which];
    which ^= 1;
    SC_TRY(adjust_affinity(h, cfg, cur, symmetric, out, n, ld));
    cur = out;
    symmetric = symmetric && h->constraint_symmetric;
    have_row_stats = false;
  }
  ev_rec(h, &e_after_refine);
  // ---- scaling vectors (RowWiseNormalize fold + Laplacian)
  bool flags_by_kernel = false;
  if (resume) {
    SC_TRY(ensure_eig(h, n));  // (scaling vectors and the finite-ness flag are resident)
  } else if (!symmetric) {
    // general matrix (e.g. RowWiseThreshold without a later Symmetrize / Diffuse):
    // Op x = p .* x + cl .* (M (cr .* x)), no similarity transform
    SC_TRY(ensure_gen(h, n));
    launch_row_stats(s, cur, n, ld, ptr<double>(h->rowmax), ptr<double>(h->deg));
    launch_scaling_general(s, ptr<double>(h->deg), n, cfg->laplacian_type,
                           ptr<double>(h->cvec), ptr<double>(h->crvec), ptr<double>(h->pvec));
  } else {
    if (!have_row_stats)
      launch_row_stats(s, cur, n, ld, ptr<double>(h->rowmax), ptr<double>(h->rowsum));
    // (the kernel's first thread also sets up the solver's flag words: see rowops.hip)
    SC_TRY(ensure_eig(h, n));
    launch_scaling_vectors(s, ptr<double>(h->rowmax), ptr<double>(h->rowsum), n,
                           cfg->laplacian_type, folded_rownorm ? 1 : 0, ptr<double>(h->cvec),
                           ptr<double>(h->pvec), ptr<double>(h->tvec), ptr<int>(h->flags),
                           h->affinity_from_embeddings ? ptr<int>(h->symflag) : nullptr);
    flags_by_kernel = true;
  }
  // a NaN / inf anywhere in the refined matrix (zero embedding rows, an all-zero refined row
  // under RowWiseNormalize, ...) reaches its row sums, hence c / p: np.linalg.eig raises on
  // such input; the flag is read with the solver's first host sync
  SC_TRY(ensure_eig(h, n));
  if (flags_by_kernel) {
  } else if (h->affinity_from_embeddings)  // a zero embedding row: its NaNs may have been dropped
    SC_HIP(h, hipMemcpyAsync(ptr<int>(h->flags) + 12, ptr<int>(h->symflag) + 1, sizeof(int),
                             hipMemcpyDeviceToDevice, s));
  else
    SC_HIP(h, hipMemsetAsync(ptr<int>(h->flags) + 12, 0, sizeof(int), s));
  launch_check_finite(s, ptr<double>(h->cvec), ptr<double>(h->pvec), n, ptr<int>(h->flags) + 12);
  if (front_only && !flags_by_kernel)  // the lockstep group solve starts from clean chain flags
    SC_HIP(h, hipMemsetAsync(ptr<int>(h->flags) + 13, 0, 3 * sizeof(int), s));
  SC_TRY(check_last(h, "scaling launch"));
  if (sw::eig_trace() > 2 && symmetric) {
    std::vector<double> rm(n), rs(n);
    hipMemcpyAsync(rm.data(), h->rowmax.p, n * sizeof(double), hipMemcpyDeviceToHost, s);
    hipMemcpyAsync(rs.data(), h->rowsum.p, n * sizeof(double), hipMemcpyDeviceToHost, s);
    hipStreamSynchronize(s);
    int imin = 0, imax = 0;
    for (int i = 0; i < n; ++i) {
      if (rm[i] < rm[imin]) imin = i;
      if (rm[i] > rm[imax]) imax = i;
    }
    fprintf(stderr, "[sc] scaling: fused stats %d; rowmax min %.6g at %d, max %.6g at %d; "
            "rowsum[%d] %.6g\n", (int)have_row_stats, rm[imin], imin, rm[imax], imax, imin,
            rs[imin]);
  }
  int e_after_scaling;
  ev_rec(h, &e_after_scaling);
  // the refined matrix, and the operator a symmetric solve of it works on
  FrontResult op;
  op.matrix = cur;
  op.scratch = bufs[which];
  op.ld = ld;
  op.symmetric = symmetric;
  op.folded_rownorm = folded_rownorm;
  op.free_op = free_path || (resume && resume->free_op);
  op.laplacian_type = cfg->laplacian_type;
  op.chain_flags_cleared = flags_by_kernel;  // (never on a resume: the group solve ran the chain)
  op.skip_fused = resume && resume->skip_fused;
  op.digits_fused = free_path && digits_of == cur;
  op.diffuse_explicit = !free_path && n_diffuse > 0;
  op.crop_source = crop_source;
  op.cut_kernel = cut_kernel;
  if (stop_before_solver) {
    *stop_before_solver = op;
    return SC_OK;
  }
  if (front_only) {
    *front_only = op;
    return SC_OK;
  }
  // ---- eigen + eigengap
  EigRequest rq = make_eig_request(cfg);
  EigDecision dc;
  std::vector<double> w;
  if (symmetric) {
    SC_TRY(sym_topk(h, op, n, rq, diag, &dc, &w));
  } else {
    rq.decision_aware = 1;
    SC_TRY(gen_topk(h, cur, ld, n, cfg->laplacian_type, rq, diag, &dc, &w, bufs[which]));
  }
  int e_after_eig;
  ev_rec(h, &e_after_eig);
  h->last_w = w;
  if (diag) {
    diag->n = n;
    diag->n_clusters_raw = dc.n_clusters_raw;
    diag->max_delta = dc.max_delta;
    diag->eig_descending = rq.descend;
    diag->n_eigenvalues = std::min((int)w.size(), SC_MAX_EIG);
    for (int i = 0; i < diag->n_eigenvalues; ++i) diag->eigenvalues[i] = w[i];
    diag->symmetry_state = !symmetric ? 3 : (folded_rownorm ? 2 : 1);
    if (!free_path && n_diffuse > 0) diag->diffuse_path = SC_DIFFUSE_PATH_EXPLICIT;
  }
  StageEvents& t = h->stage_events;
  t.pending = true;
  t.begin = e_begin;
  t.after_refine = e_after_refine;
  t.after_scaling = e_after_scaling;
  t.after_eig = e_after_eig;
  t.n_diffuse = n_diffuse;
  for (int i = 0; i < n_diffuse; ++i) {
    t.diffuse[i][0] = (int)diffuse_ms_events[i][0];
    t.diffuse[i][1] = (int)diffuse_ms_events[i][1];
  }
  t.fine = fine;
  t.free_path = free_path;
  t.blur[0] = eb0;
  t.blur[1] = eb1;
  t.thr[0] = et0;
  t.thr[1] = et1;
  if (defer_timing) return SC_OK;
  SC_HIP(h, hipStreamSynchronize(s));
  resolve_stage_times(h, diag);
  return SC_OK;
}

extern "C" int sc_eig_ncluster(sc_handle h, const sc_config* cfg, sc_diag* diag) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_config(h, cfg));
  if (!h->have_affinity) return fail(h, SC_ERR_INVALID, "no affinity resident");
  SC_HIP(h, hipSetDevice(h->device));
  h->nev = 0;
  if (diag) memset(diag, 0, sizeof(*diag));
  return eig_ncluster_impl(h, cfg, diag, nullptr);
}

extern "C" int sc_num_eigenvectors(sc_handle h) { return h ? h->n_vec : 0; }

extern "C" int sc_num_eigenvalues(sc_handle h) { return h ? (int)h->last_w.size() : 0; }

extern "C" int sc_get_eigenvalues(sc_handle h, double* out, int count) {
  if (!h || !out) return SC_ERR_INVALID;
  if (count < 0 || count > (int)h->last_w.size())
    return fail(h, SC_ERR_INVALID, "eigenvalue request out of range");
  for (int i = 0; i < count; ++i) out[i] = h->last_w[i];
  return SC_OK;
}

extern "C" int sc_get_eigenvectors(sc_handle h, double* out, int n, int ncols) {
  if (!h || !out) return SC_ERR_INVALID;
  if (n != h->n || ncols <= 0 || ncols > h->n_vec)
    return fail(h, SC_ERR_INVALID, "eigenvector request out of range");
  SC_HIP(h, hipSetDevice(h->device));
  launch_colmajor_to_rowmajor(h->stream, ptr<double>(h->E), round_up(n, 16), n, ncols,
                              ptr<double>(h->Eio), ncols);
  return d2h_matrix(h, ptr<double>(h->Eio), ncols, n, ncols, out);
}

// ------------------------------------------------------------------------------
// whole path
// ------------------------------------------------------------------------------
extern "C" int sc_run_resident(sc_handle h, const sc_config* cfg, int64_t* labels,
                               sc_diag* diag) {
  return run_resident(h, cfg, labels, diag, true);
}

int run_resident(sc_handle h, const sc_config* cfg, int64_t* labels, sc_diag* diag,
                 bool from_embeddings) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_config(h, cfg));
  if (!labels) return fail(h, SC_ERR_INVALID, "labels is NULL");
  if (from_embeddings && !h->have_x) return fail(h, SC_ERR_INVALID, "no embeddings resident");
  if (!from_embeddings && (!h->have_affinity || h->affinity_from_embeddings))
    return fail(h, SC_ERR_INVALID, "no caller-supplied affinity resident");
  SC_HIP(h, hipSetDevice(h->device));
  sc_diag local;
  sc_diag* dg = diag ? diag : &local;
  memset(dg, 0, sizeof(*dg));
  h->nev = 0;
  int e0, e1, e2;
  ev_rec(h, &e0);
  if (from_embeddings) SC_TRY(sc_compute_affinity(h));
  if (constraint_active(h, cfg, true)) SC_TRY(sc_apply_constraint(h, cfg));  // :259-264
  ev_rec(h, &e1);
  // (no wait between the eigensolver and k-means: its launches queue behind the Ritz vectors)
  SC_TRY(eig_ncluster_impl(h, cfg, dg, nullptr, nullptr, true));
  int k = dg->n_clusters_raw;
  if (cfg->min_clusters > 0 && k < cfg->min_clusters) k = cfg->min_clusters;  // :295-296
  const int rc_cluster = sc_cluster(h, cfg, k, labels, dg);
  if (rc_cluster != SC_OK) {
    h->stage_events.pending = false;
    return rc_cluster;
  }
  ev_rec(h, &e2);
  SC_HIP(h, hipStreamSynchronize(h->stream));
  resolve_stage_times(h, dg);
  dg->stage_ms[SC_STAGE_AFFINITY] = ev_ms(h, e0, e1);
  dg->stage_ms[SC_STAGE_TOTAL] = ev_ms(h, e0, e2);
  if (h->profile_level >= 1 && from_embeddings)
    dg->stage_ms[SC_STAGE_AFFINITY_GEMM] = ev_ms(h, h->aff_ev[0], h->aff_ev[1]);
  return SC_OK;
}

extern "C" int sc_set_profiling(sc_handle h, int level) {
  if (!h || level < 0 || level > 2) return SC_ERR_INVALID;
  h->profile_level = level;
  return SC_OK;
}

// what the double* batch entry points describe: compact host fp64 rows, one per utterance
std::vector<sc_array> host_f64_arrays(const double* const* xs, const int* ns, int d, int count) {
  std::vector<sc_array> arrays(std::max(count, 0));
  for (int i = 0; i < count; ++i) arrays[i] = host_f64_array(xs[i], ns[i], d);
  return arrays;
}

// Independent calls on ONE handle, one after the other -- with the upload of call i + 1 taken
// off the throughput path: a helper thread copies its embeddings (pageable or pinned, as the
// caller holds them) to the handle's SPARE embeddings buffer on a copy stream while call i's
// pipeline runs; the call then adopts the buffer instead of uploading.  A pipeline of n = 8192
// is 2.3 ms of kernels behind 0.30 ms of PCIe transfer (16.8 MB at 55 GB/s): in sequence the
// link idles 89 % of the time and the GPU 11 %.  Two buffers: no call ever waits for a buffer
// its predecessor still reads.  Same kernels, same arguments, same results as sc_predict.
// (Utterances below 256 KB gain nothing from a second thread: plain loop.)
int predict_sequence(sc_handle h, const int* idx, int count, const sc_array* xs,
                     const int* ns, int d, const sc_config* cfg, int64_t* const* labels,
                     sc_diag* diags) {
  auto at = [&](int k) { return idx ? idx[k] : k; };
  // one call that ingests for itself.  A host source is waited for like sc_predict does; a
  // device source needs no wait: it outlives the batch call, and the pipeline behind the ingest
  // kernel synchronises the stream before the next call touches the arena
  auto one_call = [&](int i) -> int {
    SC_TRY(validate_config(h, cfg));
    SC_HIP(h, hipSetDevice(h->device));
    h->sweep_slot.clear();
    SC_TRY(ingest_embeddings(h, xs[i], xs[i].location == SC_MEM_HOST));
    return sc_run_resident(h, cfg, labels[i], diags ? diags + i : nullptr);
  };
  int nmax = 0;
  size_t smallest = ~(size_t)0;
  bool prefetchable = true;  // the helper thread's copy is for host fp64 rows
  for (int k = 0; k < count; ++k) {
    const int i = at(k);
    if (!xs[i].data || ns[i] <= 0 || d <= 0) { smallest = 0; continue; }
    nmax = std::max(nmax, ns[i]);
    smallest = std::min(smallest, (size_t)ns[i] * d * sizeof(double));
    prefetchable = prefetchable && array_is_host_f64_rows(xs[i]);
  }
  if (nmax > 0) SC_TRY(sc_reserve(h, nmax, d));  // one arena sized for the largest member
  if (count < 2 || smallest < ((size_t)256 << 10) || !prefetchable) {
    for (int k = 0; k < count; ++k) SC_TRY(one_call(at(k)));
    return SC_OK;
  }
  SC_TRY(validate_config(h, cfg));
  SC_HIP(h, hipSetDevice(h->device));
  const size_t ldx = round_up(d, 16);
  SC_TRY(grow(h, h->Xalt, (size_t)nmax * ldx * sizeof(double)));
  SC_TRY(grow(h, h->X, (size_t)nmax * ldx * sizeof(double)));
  if (!h->copy_stream)
    SC_HIP(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
  const DevBuf slot[2] = {h->X, h->Xalt};
  std::mutex mu;
  std::condition_variable cv;
  int uploaded = 0;   // calls [0, uploaded) have their embeddings on the device
  int finished = 0;   // calls [0, finished) are done with their buffer
  bool stop = false;
  hipError_t upload_err = hipSuccess;
  auto upload_loop = [&]() {
    hipSetDevice(h->device);
    for (int k = 0; k < count; ++k) {
      {
        std::unique_lock<std::mutex> lock(mu);
        cv.wait(lock, [&] { return stop || finished >= k - 1; });  // slot k % 2 is free
        if (stop) return;
      }
      const int i = at(k);
      hipError_t e = hipMemcpy2DAsync(slot[k & 1].p, ldx * sizeof(double), xs[i].data,
                                      (size_t)(ns[i] == 1 ? d : xs[i].row_stride) * sizeof(double),
                                      (size_t)d * sizeof(double), ns[i], hipMemcpyHostToDevice,
                                      h->copy_stream);
      if (e == hipSuccess) e = hipStreamSynchronize(h->copy_stream);
      std::lock_guard<std::mutex> lock(mu);
      if (e != hipSuccess) {
        upload_err = e;
        stop = true;
        cv.notify_all();
        return;
      }
      uploaded = k + 1;
      cv.notify_all();
    }
  };
  std::thread helper;
  try {
    helper = std::thread(upload_loop);
  } catch (...) {  // (no thread to be had: every call uploads for itself)
    for (int k = 0; k < count; ++k) SC_TRY(one_call(at(k)));
    return SC_OK;
  }
  int rc = SC_OK;
  for (int k = 0; k < count && rc == SC_OK; ++k) {
    const int i = at(k);
    {
      std::unique_lock<std::mutex> lock(mu);
      cv.wait(lock, [&] { return stop || uploaded > k; });
      if (stop) break;
    }
    // adopt the buffer: sc_set_embeddings without the copy
    h->X = slot[k & 1];
    h->Xalt = slot[(k & 1) ^ 1];
    h->n = ns[i];
    h->d = d;
    h->ldn = matrix_ld(ns[i]);
    h->ldx = (int)ldx;
    h->have_affinity = h->have_cropval = false;
    h->n_vec = 0;
    h->sweep_slot.clear();
    h->have_x = true;
    rc = sc_run_resident(h, cfg, labels[i], diags ? diags + i : nullptr);
    std::lock_guard<std::mutex> lock(mu);
    finished = k + 1;
    cv.notify_all();
  }
  {
    std::lock_guard<std::mutex> lock(mu);
    stop = true;
    cv.notify_all();
  }
  helper.join();  // (h->X stays the buffer of the last call that ran: its embeddings are resident)
  if (rc != SC_OK) return rc;
  if (upload_err != hipSuccess)
    return fail(h, SC_ERR_HIP, (std::string("embedding upload: ") + hipGetErrorString(upload_err)).c_str());
  return SC_OK;
}

extern "C" int sc_predict_batch(sc_handle h, const double* const* xs, const int* ns, int d,
                                int count, const sc_config* cfg, int64_t* const* labels,
                                sc_diag* diags) {
  if (!h) return SC_ERR_INVALID;
  if (!xs || !ns || !labels || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  h->last_routes.assign(count, SC_BATCH_ROUTE_SINGLE);
  const std::vector<sc_array> arrays = host_f64_arrays(xs, ns, d, count);
  return predict_sequence(h, nullptr, count, arrays.data(), ns, d, cfg, labels, diags);
}

extern "C" int sc_last_batch_routes(sc_handle h, int32_t* routes, int count) {
  if (!h) return SC_ERR_INVALID;
  if (!routes) return fail(h, SC_ERR_INVALID, "routes is NULL");
  if (count != (int)h->last_routes.size())
    return fail(h, SC_ERR_INVALID, "count is not the last batch's");
  for (int i = 0; i < count; ++i) routes[i] = h->last_routes[i];
  return SC_OK;
}

// The batch over `streams` HIP streams of the handle's device: handle h plus streams - 1
// pooled handles (one arena + one stream each), one host thread per stream inside this call.
// Small utterances cannot fill 256 CUs and their pipeline is a chain of short, dependent
// launches with two host synchronisations: several in flight hide each other's latencies.
// Utterances are dealt longest-processing-time first (cost n^3 + 64 n^2).
extern "C" int sc_predict_batch_streams(sc_handle h, const double* const* xs, const int* ns,
                                        int d, int count, const sc_config* cfg,
                                        int64_t* const* labels, sc_diag* diags, int streams) {
  if (!h) return SC_ERR_INVALID;
  if (!xs || !ns || !labels || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  const std::vector<sc_array> arrays = host_f64_arrays(xs, ns, d, count);
  return predict_batch_streams_impl(h, arrays.data(), ns, d, count, cfg, labels, diags, streams);
}

int predict_batch_streams_impl(sc_handle h, const sc_array* xs, const int* ns, int d, int count,
                               const sc_config* cfg, int64_t* const* labels, sc_diag* diags,
                               int streams) {
  streams = std::max(1, std::min(streams, std::min(count, 32)));
  h->last_routes.assign(count, SC_BATCH_ROUTE_SINGLE);
  if (streams == 1) return predict_sequence(h, nullptr, count, xs, ns, d, cfg, labels, diags);
  while ((int)h->pool.size() < streams - 1) {
    sc_handle sub = nullptr;
    const int rc = sc_create(h->device, &sub);
    if (rc != SC_OK) return fail(h, rc, "could not create a stream handle for the batch");
    sub->profile_level = h->profile_level;
    h->pool.push_back(sub);
  }
  // longest-processing-time-first assignment (ties: lower index, lower stream)
  std::vector<int> order(count);
  for (int i = 0; i < count; ++i) order[i] = i;
  auto cost = [&](int i) { const double n = ns[i]; return n * n * n + 64.0 * n * n; };
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost(a) > cost(b); });
  std::vector<std::vector<int>> share(streams);
  std::vector<double> load(streams, 0.0);
  for (int i : order) {
    int best = 0;
    for (int q = 1; q < streams; ++q)
      if (load[q] < load[best]) best = q;
    share[best].push_back(i);
    load[best] += cost(i);
  }
  std::vector<int> rcs(streams, SC_OK);
  auto work = [&](int q) {
    sc_handle hq = q == 0 ? h : h->pool[q - 1];
    if (q > 0) hq->blur_ext = h->blur_ext;  // (weights of a blur radius above 32 live in the handle)
    int nmax = 0;
    for (int i : share[q]) nmax = std::max(nmax, ns[i]);
    int rc = nmax > 0 ? sc_reserve(hq, nmax, d) : SC_OK;
    if (rc == SC_OK) rc = sc_clear_constraint(hq);
    // (the stream's calls one after the other, each upload under its predecessor's pipeline)
    if (rc == SC_OK)
      rc = predict_sequence(hq, share[q].data(), (int)share[q].size(), xs, ns, d, cfg, labels,
                            diags);
    rcs[q] = rc;
  };
  std::vector<std::thread> threads;
  for (int q = 1; q < streams; ++q) threads.emplace_back(work, q);
  work(0);
  for (std::thread& t : threads) t.join();
  for (int q = 0; q < streams; ++q)
    if (rcs[q] != SC_OK) {
      if (q > 0) h->err = h->pool[q - 1]->err;
      return rcs[q];
    }
  return SC_OK;
}

// ------------------------------------------------------------------------------
// single stages
// ------------------------------------------------------------------------------
extern "C" int sc_stage_affinity(sc_handle h, const double* x, int n, int d, double* out) {
  if (!h) return SC_ERR_INVALID;
  if (!out) return fail(h, SC_ERR_INVALID, "out is NULL");
  SC_TRY(sc_set_embeddings(h, x, n, d));
  SC_TRY(sc_compute_affinity(h));
  return d2h_matrix(h, ptr<double>(h->A0), h->ldn, n, n, out);
}

extern "C" int sc_stage_refine(sc_handle h, int op, const sc_config* cfg, const double* in,
                               int n, double* out) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_config(h, cfg));
  if (!in || !out || n <= 0) return fail(h, SC_ERR_INVALID, "affinity must be (n, n)");
  SC_HIP(h, hipSetDevice(h->device));
  SC_TRY(ensure_matrices(h, n, 0));
  const int ld = matrix_ld(n);
  h->have_affinity = h->have_cropval = false;
  h->have_x = false;
  h->n_vec = 0;
  SC_TRY(h2d_matrix(h, in, n, n, ptr<double>(h->B1), ld));
  SC_TRY(run_refine_op(h, op, cfg, ptr<double>(h->B1), ptr<double>(h->B2), n, ld));
  return d2h_matrix(h, ptr<double>(h->B2), ld, n, n, out);
}

extern "C" int sc_stage_laplacian(sc_handle h, int laplacian_type, const double* in, int n,
                                  double* out) {
  if (!h) return SC_ERR_INVALID;
  if (!in || !out || n <= 0) return fail(h, SC_ERR_INVALID, "affinity must be (n, n)");
  if (laplacian_type < SC_LAPLACIAN_AFFINITY || laplacian_type > SC_LAPLACIAN_GRAPH_CUT)
    return fail(h, SC_ERR_INVALID, "laplacian_type must be a LaplacianType");
  SC_HIP(h, hipSetDevice(h->device));
  SC_TRY(ensure_matrices(h, n, 0));
  const int ld = matrix_ld(n);
  h->have_affinity = h->have_cropval = false;
  h->have_x = false;
  h->n_vec = 0;
  SC_TRY(h2d_matrix(h, in, n, n, ptr<double>(h->B1), ld));
  if (laplacian_type == SC_LAPLACIAN_AFFINITY)
    return d2h_matrix(h, ptr<double>(h->B1), ld, n, n, out);
  launch_laplacian(h->stream, ptr<double>(h->B1), ptr<double>(h->B2), n, ld, laplacian_type,
                   ptr<double>(h->deg));
  SC_TRY(check_last(h, "laplacian launch"));
  return d2h_matrix(h, ptr<double>(h->B2), ld, n, n, out);
}

__global__ void k_negate(const double* in, double* out, size_t total) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (size_t)gridDim.x * blockDim.x)
    out[e] = -in[e];
}

__global__ void k_fill(double* p, int n, double v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// sc_stage_sym_eig behind its upload: the matrix is in B1 (row pitch matrix_ld(n)).  Leaves the
// `count` values in `values` and, with `vectors`, the eigenvectors in E (column-major, pitch
// round_up(n, 16)); returns with the stream drained.
int stage_sym_eig_resident(sc_handle h, int n, int count, int descend, double* values,
                           bool vectors, sc_diag* diag) {
  const int ld = matrix_ld(n);
  if (n > kDenseMax && count > kMaxVectors && !vectors) {
    // values only, more than a Krylov basis holds: the dense full-spectrum path
    // (Householder tridiagonalisation + Sturm bisection, eig_dense.hip)
    SC_TRY(ensure_eig(h, n));
    SC_TRY(grow(h, h->td_d, (size_t)n * sizeof(double)));
    SC_TRY(grow(h, h->td_e, (size_t)n * sizeof(double)));
    SC_TRY(grow(h, h->td_theta, (size_t)n * sizeof(double)));
    SC_TRY(grow(h, h->td_work, (size_t)(5 * (size_t)n + 2048) * sizeof(double)));
    SC_TRY(grow(h, h->td_tau, (size_t)n * sizeof(double)));
    SC_TRY(grow(h, h->td_panel, (size_t)n * 128 * sizeof(double)));
    launch_tridiagonalize_blocked(h->stream, ptr<double>(h->B1), ld, n, ptr<double>(h->td_d),
                                  ptr<double>(h->td_e), ptr<double>(h->td_tau),
                                  ptr<double>(h->td_panel), ptr<double>(h->td_work),
                                  ptr<double>(h->splitk));
    launch_tridiagonal_eigenvalues(h->stream, ptr<double>(h->td_d), ptr<double>(h->td_e), n,
                                   ptr<double>(h->td_theta), ptr<double>(h->td_work));
    SC_TRY(check_last(h, "dense eigenvalue launch"));
    std::vector<double> all(n);
    SC_HIP(h, hipMemcpyAsync(all.data(), h->td_theta.p, (size_t)n * sizeof(double),
                             hipMemcpyDeviceToHost, h->stream));
    SC_HIP(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < count; ++i) values[i] = descend ? all[i] : all[n - 1 - i];
    if (diag) {
      memset(diag, 0, sizeof(*diag));
      diag->n = n;
      diag->eig_path = SC_EIG_PATH_DENSE_TRIDIAG;
    }
    return SC_OK;
  }
  // Op = +M (descend) or -M (ascend): c = 1, p = 0, t = 1; the sign is folded by
  // running on sigma * M through c = 1 and a negated copy when ascending.
  const int nb = (n + 255) / 256;
  hipLaunchKernelGGL(k_fill, dim3(nb), dim3(256), 0, h->stream, ptr<double>(h->cvec), n, 1.0);
  hipLaunchKernelGGL(k_fill, dim3(nb), dim3(256), 0, h->stream, ptr<double>(h->pvec), n, 0.0);
  hipLaunchKernelGGL(k_fill, dim3(nb), dim3(256), 0, h->stream, ptr<double>(h->tvec), n, 1.0);
  const double* S = ptr<double>(h->B1);
  if (!descend) {  // smallest eigenpairs of M = largest of -M
    hipLaunchKernelGGL(k_negate, dim3(2048), dim3(256), 0, h->stream, ptr<double>(h->B1),
                       ptr<double>(h->B2), (size_t)n * ld);
    S = ptr<double>(h->B2);
  }
  EigRequest rq;
  rq.descend = descend ? 1 : 0;
  rq.max_clusters = 0;
  rq.min_clusters = 0;
  rq.stop_eigenvalue = 0.0;
  rq.eigengap_type = SC_EIGENGAP_RATIO;
  rq.use_stop = 0;
  rq.value_tol = 1e-10;
  rq.vector_tol = 1e-11;
  rq.max_cycles = 60;
  rq.fixed_count = count;
  EigDecision dc;
  std::vector<double> w;
  sc_diag local;
  sc_diag* dg = diag ? diag : &local;
  memset(dg, 0, sizeof(*dg));
  h->nev = 0;
  SC_TRY(ensure_eig(h, n));
  SC_HIP(h, hipMemsetAsync(ptr<int>(h->flags) + 12, 0, sizeof(int), h->stream));
  FrontResult op;  // (the matrix it is given, no scaling: c = 1, p = 0)
  op.matrix = S;
  op.scratch = S == ptr<double>(h->B1) ? ptr<double>(h->B2) : ptr<double>(h->B1);
  op.ld = ld;
  op.symmetric = true;
  SC_TRY(sym_topk(h, op, n, rq, dg, &dc, &w));
  SC_HIP(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < count; ++i) values[i] = w[i];
  return SC_OK;
}

extern "C" int sc_stage_sym_eig(sc_handle h, const double* m, int n, int count, int descend,
                                double* values, double* vectors, sc_diag* diag) {
  if (!h) return SC_ERR_INVALID;
  if (!m || n <= 0 || count <= 0 || count > n || !values)
    return fail(h, SC_ERR_INVALID, "bad eigen request");
  SC_HIP(h, hipSetDevice(h->device));
  SC_TRY(ensure_matrices(h, n, 0));
  const int ld = matrix_ld(n);
  h->n = n;
  h->ldn = ld;
  h->have_affinity = h->have_cropval = false;
  h->have_x = false;
  SC_TRY(h2d_matrix(h, m, n, n, ptr<double>(h->B1), ld));
  SC_TRY(stage_sym_eig_resident(h, n, count, descend, values, vectors != nullptr, diag));
  if (vectors) {
    launch_colmajor_to_rowmajor(h->stream, ptr<double>(h->E), round_up(n, 16), n, count,
                                ptr<double>(h->Eio), count);
    SC_TRY(d2h_matrix(h, ptr<double>(h->Eio), count, n, count, vectors));
  }
  return SC_OK;
}

// sc_stage_eig behind its upload, as stage_sym_eig_resident (ensure_gen has run)
int stage_eig_resident(sc_handle h, int n, int count, int descend, double* values,
                       sc_diag* diag) {
  const int ld = matrix_ld(n);
  const int nb = (n + 255) / 256;
  hipLaunchKernelGGL(k_fill, dim3(nb), dim3(256), 0, h->stream, ptr<double>(h->cvec), n, 1.0);
  hipLaunchKernelGGL(k_fill, dim3(nb), dim3(256), 0, h->stream, ptr<double>(h->crvec), n, 1.0);
  hipLaunchKernelGGL(k_fill, dim3(nb), dim3(256), 0, h->stream, ptr<double>(h->pvec), n, 0.0);
  const double* S = ptr<double>(h->B1);
  if (!descend) {  // smallest real parts of M = largest of -M
    hipLaunchKernelGGL(k_negate, dim3(2048), dim3(256), 0, h->stream, ptr<double>(h->B1),
                       ptr<double>(h->B2), (size_t)n * ld);
    S = ptr<double>(h->B2);
  }
  EigRequest rq;
  rq.descend = descend ? 1 : 0;
  rq.max_clusters = 0;
  rq.min_clusters = 0;
  rq.stop_eigenvalue = 0.0;
  rq.eigengap_type = SC_EIGENGAP_RATIO;
  rq.use_stop = 0;
  rq.value_tol = 1e-10;
  rq.vector_tol = 1e-11;
  rq.max_cycles = 100;
  rq.fixed_count = count;
  EigDecision dc;
  std::vector<double> w;
  sc_diag local;
  sc_diag* dg = diag ? diag : &local;
  memset(dg, 0, sizeof(*dg));
  h->nev = 0;
  SC_TRY(ensure_eig(h, n));
  SC_HIP(h, hipMemsetAsync(ptr<int>(h->flags) + 12, 0, sizeof(int), h->stream));
  SC_TRY(gen_topk(h, S, ld, n, SC_LAPLACIAN_NONE, rq, dg, &dc, &w,
                  S == ptr<double>(h->B1) ? ptr<double>(h->B2) : ptr<double>(h->B1)));
  SC_HIP(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < count; ++i) values[i] = w[i];
  return SC_OK;
}

extern "C" int sc_stage_eig(sc_handle h, const double* m, int n, int count, int descend,
                            double* values, double* vectors, sc_diag* diag) {
  if (!h) return SC_ERR_INVALID;
  if (!m || n <= 0 || count <= 0 || count > n || !values)
    return fail(h, SC_ERR_INVALID, "bad eigen request");
  SC_HIP(h, hipSetDevice(h->device));
  SC_TRY(ensure_matrices(h, n, 0));
  SC_TRY(ensure_gen(h, n));
  const int ld = matrix_ld(n);
  h->n = n;
  h->ldn = ld;
  h->have_affinity = h->have_cropval = false;
  h->have_x = false;
  SC_TRY(h2d_matrix(h, m, n, n, ptr<double>(h->B1), ld));
  SC_TRY(stage_eig_resident(h, n, count, descend, values, diag));
  if (vectors) {
    launch_colmajor_to_rowmajor(h->stream, ptr<double>(h->E), round_up(n, 16), n, count,
                                ptr<double>(h->Eio), count);
    SC_TRY(d2h_matrix(h, ptr<double>(h->Eio), count, n, count, vectors));
  }
  return SC_OK;
}
