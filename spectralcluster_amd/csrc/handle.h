// Internal to the host side of the library (api.hip, eig_driver.hip, constraint_api.hip,
// callers_api.hip, kmeans_api.hip): the handle with its device arena, error plumbing, and the helpers those
// translation units share.  Not installed; the public surface is
// include/spectralcluster_amd.h.
#ifndef SPECTRALCLUSTER_AMD_HANDLE_H_
#define SPECTRALCLUSTER_AMD_HANDLE_H_

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sc_internal.h"

using namespace sc;

// ------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

constexpr int kKgenBufs = 12;   // workspace buffers of sc_stage_kmeans_general
constexpr int kGroupBanks = 2;  // banks of member arenas of the grouped batch (groups in flight)
constexpr int kGroupLanes = 3;  // leads of the grouped batch (host threads, each with its banks)

// event slots of the stage timers of the current call (resolved once the stream has drained)
struct StageEvents {
  bool pending = false, fine = false, free_path = false;
  int begin = -1, after_refine = -1, after_scaling = -1, after_eig = -1;
  int diffuse[SC_MAX_OPS][2];
  int n_diffuse = 0;
  int blur[2] = {-1, -1}, thr[2] = {-1, -1};
};

struct sc_handle_s {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  // current problem
  int n = 0, d = 0, ldn = 0, ldx = 0;
  bool have_x = false, have_affinity = false;
  bool have_cropval = false;  // cropval = CropDiagonal fill values of A0 (affinity GEMM epilogue)
  int n_vec = 0;          // eigenvector columns resident in E
  // matrices
  DevBuf X, Xn, A0, B1, B2;
  DevBuf Xalt;                       // second embeddings buffer: the NEXT call's upload lands here
  hipStream_t copy_stream = nullptr; // ... on this stream (predict_sequence, api.hip)
  DevBuf Xstage;                     // host fp32 / fp16 / bf16 rows at their own width (ingest.hip)
  // n-vectors
  DevBuf rowmax, rowsum, cvec, pvec, tvec, deg, dvec, cut, rmpart, splitk, tilemap;
  DevBuf cropval, statp;  // fused GEMM row statistics: result + per-tile partials
  // constraints: Cq (resident constraint matrix), Neumann-product work matrices, flag word
  DevBuf Cq, cp[5], symflag;
  // ... or its banded form (sc_set_constraint_band): the n - 1 values of the first off-diagonals
  DevBuf Cband;
  bool have_constraint = false, constraint_symmetric = false, constraint_applied = false;
  bool constraint_banded = false;  // the resident constraint is Cband, not Cq
  // ... or a list of directed entries (sc_set_constraint_pairs): Cpairs holds vals (pairs_count
  // doubles), then rows, then cols (int32 each); Cporig: pairs_count doubles of scratch
  DevBuf Cpairs, Cporig;
  bool constraint_pairs = false;  // the resident constraint is Cpairs (never with _banded)
  int pairs_count = 0;
  bool affinity_symmetric = true;
  bool affinity_from_embeddings = false;  // symflag[1] then says whether a row was NaN
  int qn = 0;
  int tilemap_nt = 0;     // tile-grid size the resident tilemap was built for
  DevBuf tilemap_table;   // tile orders of every grid size <= kTilemapTableMax (ensure_tilemap)
  int tilemap_off[65] = {0};
  const int2* tilemap_cur = nullptr;  // what ensure_tilemap selected for the current n
  DevBuf blurw;           // device copy of the blur weights
  DevBuf blur_tmp;        // scratch of the two-pass blur of a radius above SC_MAX_BLUR_RADIUS
  std::vector<double> blur_ext;  // weights of such a radius (sc_set_blur_weights): 2 r + 1
  // eigen workspace
  DevBuf Q, Q2, Vs, W, partial, T, Y, Yt, theta, resid, G, Rinv, Hbuf, hsq, colnorm,
      flags;
  DevBuf E, Ek, Eio;      // eigenvectors (col-major), renormed copy, row-major I/O staging
  DevBuf mvsym;           // slabs of the symmetric block matvec
  // dense full-spectrum path (eig_dense.hip): d, e, all eigenvalues, reflector work vectors
  DevBuf td_d, td_e, td_theta, td_work, td_tau, td_panel;
  std::vector<double> spectrum;  // host copy: every eigenvalue of Op, descending
  std::vector<double> last_w;    // eigenvalues the last eig call consumed (reference order)
  // general (non-symmetric) eigen path: right scaling, Im(theta), complex Ritz vectors
  // (column-major), residual partials, restart codes, dense Laplacian scratch
  DevBuf crvec, thetai, Vre, Vim, gpart, gsrc, genL, gneg;
  DevBuf ahc_size, ahc_chain, ahc_Z, ahc_lab, ahc_cent;  // size reduction (AHC) scratch
  // centroids on described arrays (centroids.hip): member table, label extents, packed labels and
  // the upload of host embeddings | the CSRs and the staging of host outputs.  The label egress
  // (egress.hip) keeps its table and the labels in the first.
  DevBuf cen_in, cen_out;
  // batched size reduction (batch_reduce.hip): bytes a wave may take (0: a share of the free
  // memory, sc_set_reduce_wave_bytes), the pinned staging of a wave's tables, merge lists and CSR
  size_t reduce_wave_bytes = 0;
  void* h_reduce = nullptr;
  size_t h_reduce_bytes = 0;
  DevBuf fb_part, fb_small, fb_x, fb_cent, fb_int;      // fallback decisions scratch
  // the single-cluster test of a batch (single_check.hip): slots and row-block partials of the
  // chain form, records of the short form, the matrices of sc_batch_single_check, and the pinned
  // twin of the slots / records
  DevBuf sck_slots, sck_part, sck_rec, sck_mats;
  void* h_sck = nullptr;
  // k-means workspace
  DevBuf kXc, kxsq, kclosest, kcand, kenorm, krnd, kcent, klab32, klab64, kinfo, kchain;
  DevBuf kbig, kbigw;     // more than kMaxVectors clusters: per-cluster arrays of k_kmeans<true>
  DevBuf kgen[kKgenBufs];  // sc_stage_kmeans_general (kmeans_api.hip): any (n, dim, k)
  // pinned host scratch
  double* h_theta = nullptr;  // 3 * kLdq doubles (theta, resid, Im theta)
  int* h_flags = nullptr;
  double* h_rr = nullptr;     // pinned: T (kHostRR^2) | G (64) | Y (kHostRR^2): host Rayleigh-Ritz
  std::vector<sc_handle_s*> pool;  // extra handles (streams) of sc_predict_batch_streams
  // grouped batch (batch_group.hip): member arenas (own stream for the stages before the
  // eigensolver; the lockstep chains run on THIS handle's stream), the RandomState(0) doubles
  // of every k (k-means++ seeding)
  std::vector<sc_handle_s*> gslots;
  // last sc_eig_ncluster_sweep: member arena that holds value i's eigenvectors (-1: none),
  // what it reported, and the problem size it ran on (sc_sweep_adopt)
  std::vector<int> sweep_slot;
  std::vector<sc_diag> sweep_diags;
  std::vector<double> sweep_p;
  sc_config sweep_cfg;
  int sweep_n = 0;
  hipEvent_t sync_ev = nullptr;    // a member arena: "stages before the eigensolver done"
  DevBuf gkrnd;
  bool gkrnd_ready = false;
  // staging of the group's Rayleigh-Ritz checks (device + pinned host twins), the event the
  // host waits on, the k-means info words and labels of a group in one buffer each
  DevBuf gpack, gypack, ginfo, glabels;
  double* h_gpack = nullptr;
  double* h_gypack = nullptr;
  int* h_ginfo = nullptr;
  long long* h_glabels = nullptr;
  size_t h_glabels_count = 0;
  hipEvent_t gcheck_ev = nullptr;
  // short route of a grouped batch (n <= kDenseMax, batch_group.hip): its member arenas
  // (reserved for n = kDenseMax, whatever else the batch holds), the descriptor table of a
  // wide Jacobi launch (device + pinned twin)
  std::vector<sc_handle_s*> gshort;
  DevBuf gjtab;
  JacobiItem* h_gjtab = nullptr;
  // a short AutoTune level (n <= kDenseMax, batch_sweep.hip): the pair table of its front
  DevBuf gsftab;
  ShortFrontItem* h_gsftab = nullptr;
  hipEvent_t gsftab_ev = nullptr;  // "the copy of the pinned table has been made"
  // the wave front of the short route (enqueue_front_short_wave): the member table of a wave,
  // one half per bank (device + pinned twin), and the kernel launches the last wave front enqueued
  DevBuf gswtab;
  ShortWaveItem* h_gswtab = nullptr;
  int gsw_launches = 0;
  // route of every utterance of the last batch call (sc_last_batch_routes); `groutes`: where
  // a lead of the running batch reports (the caller handle's last_routes)
  std::vector<int32_t> last_routes;
  int32_t* groutes = nullptr;
  // sc_set_batch_any_metric: the grouped and short routes of a batch take every device metric
  // (off: cosine alone, every other metric's utterances run as single calls)
  bool batch_any_metric = false;
  std::vector<sc_handle_s*> glanes;  // the leads of lanes 1.. (batch_group.hip: ensure_lanes)
  class HostPool* gpool = nullptr;  // host workers of the group checks (host_pool.h)
  // grouped front: the stages before the eigensolver of a whole group as grouped launches on
  // the stream of the group's bank, handed to this handle's stream through the bank's event
  hipStream_t gbank_stream[kGroupBanks] = {nullptr};
  hipStream_t gchain_stream = nullptr;  // the lockstep chains of a grouped batch (stands in for `stream`)
  hipEvent_t gbank_ev[kGroupBanks] = {nullptr};
  int gconv_hist[16] = {0};  // members of this batch that converged at basis 8 * index ...
  int gconv_seen = 0;        // ... of this many: where a speculative block is likely wasted
  hipEvent_t ev[48];
  int nev = 0;
  StageEvents stage_events;
  int profile_level = 1;  // sc_set_profiling: 0 totals only, 1 stages, 2 per-kernel events
  int mv_ev[16][2];       // event pairs around the block matvec launches (level 2)
  int n_mv_ev = 0;
  int aff_ev[2] = {-1, -1};  // around the affinity GEMM launch (level 2)
  // what the small per-call uploads last carried (skipped when unchanged)
  int blurw_radius = -1;
  double blurw_host[2 * SC_MAX_BLUR_RADIUS + 1];
  int krnd_k = -1, krnd_trials = -1;
  int kfirst_n = -1, kfirst = 0;  // first k-means++ centre of the last n (RandomState(0) draw)
  // ---- matrix-free Diffuse (free_api.hip)
  int diffuse_mode = -1;   // sc_set_diffuse_mode: 0 auto, 1 explicit fp64 product, 2 matrix-free
                           // wherever the sequence allows it; -1: the environment's default
  DevBuf fq, ft32, fy1, fR, fscal, fwords, fcand, fY, fsplit, fypart, frpart;  // digits, T (fp32 tiles), A 1, sum|q|,
                           // scalars, M | count | ovf words, candidate lists, A Vs
  int free_prune = -1;     // sc_set_free_prune: 1 skip list on, 0 every tile, -1 environment
  DevBuf fq2part, fmx64, ftau64, fplan;  // tile skip list of the digit product (diffuse_free.hip):
                           // squared segment norms per (block, row), their maxima per 64-row
                           // group, the groups' thresholds, surviving tiles per tile row
  int* h_free = nullptr;   // pinned copy of the ovf words (80)
  bool free_checked = false;  // the overflow rows of h_free have been dealt with
  int free_ev[5] = {-1, -1, -1, -1, -1};  // event slots: begin | quantised | product | scans | stats
  // What the last block Lanczos solve of sym_topk left in Q / T / G / cvec / pvec, for
  // sc_stage_krylov_state: basis size at exit (0: no such solve, or the arena has moved on), its
  // n, restart cycles, block steps enqueued beyond the basis (run-ahead), two-product operator
  int krylov_m = 0, krylov_n = 0, krylov_cycles = 0, krylov_ahead = 0;
  bool krylov_free = false;
  // The same for the last block Arnoldi solve of gen_topk (Q, Q2 = Op Q, T = H, the scaling
  // vectors), for sc_stage_arnoldi_state: basis size at exit (0: no such solve), its n, restart
  // cycles and block passes of that solve alone, the wide form, the operator with its sign turned
  int arnoldi_m = 0, arnoldi_n = 0, arnoldi_cycles = 0, arnoldi_passes = 0;
  bool arnoldi_wide = false, arnoldi_negate = false;
  // What the last front on this handle launched, for sc_stage_front: the blur kernel (and the
  // rows per wave of the streaming one)
  BlurLaunch last_blur;
};

// hipEvent slots of the current call (reset by the entry points); -1 when exhausted
inline void ev_rec(sc_handle h, int* slot) {
  if (h->nev < 48) {
    hipEventRecord(h->ev[h->nev], h->stream);
    *slot = h->nev++;
  } else {
    *slot = -1;
  }
}
inline float ev_ms(sc_handle h, int a, int b) {
  if (a < 0 || b < 0) return 0.f;
  float ms = 0.f;
  hipEventElapsedTime(&ms, h->ev[a], h->ev[b]);
  return ms;
}

constexpr int kTilemapTableMax = 64;
constexpr int kMaxCols = 128;  // eigenvector columns the arena can hold
// Leading dimension of the n x n matrices.  A row stride that is a multiple of 4 KiB maps
// the 128 rows of an operand panel onto the same few L2 sets (the GEMM reads one 128-byte
// line per row and K-tile): such strides get one extra 128-byte line.
inline int matrix_ld(int n) {
  int ld = round_up(n, 16);
  if (ld % 512 == 0) ld += 16;
  return ld;
}

// eigenvectors are column-major on the device: column j at E + j * lde, lde = round_up(n, 16)

#define SC_HIP(h, call)                                                         \
  do {                                                                          \
    hipError_t e_ = (call);                                                     \
    if (e_ != hipSuccess) {                                                     \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);             \
      return e_ == hipErrorOutOfMemory ? SC_ERR_OOM : SC_ERR_HIP;               \
    }                                                                           \
  } while (0)

#define SC_TRY(expr)                \
  do {                              \
    int rc_ = (expr);               \
    if (rc_ != SC_OK) return rc_;   \
  } while (0)

inline int fail(sc_handle h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

inline int grow(sc_handle h, DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes) return SC_OK;
  if (b.p) {
    SC_HIP(h, hipStreamSynchronize(h->stream));
    SC_HIP(h, hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
  }
  SC_HIP(h, hipMalloc(&b.p, bytes));
  b.bytes = bytes;
  return SC_OK;
}
template <typename T>
inline T* ptr(const DevBuf& b) {
  return reinterpret_cast<T*>(b.p);
}

// `affinity_copy` false: no A0 (a member arena of an AutoTune sweep only holds B1 / B2)
int ensure_matrices(sc_handle h, int n, int d, bool affinity_copy = true);

// (ti, tj) order of the symmetric GEMM tiles for problems of n rows (cached per handle)
int ensure_tilemap(sc_handle h, int n);
// `count` independent calls (indices idx[0..count) into xs / ns / labels / diags; idx == nullptr:
// 0..count-1) one after the other on handle h, each call's upload under its predecessor's pipeline
// (the upload under the predecessor's pipeline is for host fp64 rows; a device source is widened
// by a kernel on the call's stream, a narrow host source copied per call)
int predict_sequence(sc_handle h, const int* idx, int count, const sc_array* xs,
                     const int* ns, int d, const sc_config* cfg, int64_t* const* labels,
                     sc_diag* diags);
// ---- caller memory as described arrays (ingest.hip; the shared rules: array_layout.h) -------
// One descriptor check (ingest.hip's validate_view), one role each; every check comes before any
// launch or copy and answers SC_ERR_INVALID + message:
//   validate_array           embeddings: (n, d) of any positive extents, the four float dtypes
//   validate_kmeans_array    ... and rows * cols <= 2^31 - 1
//   validate_affinity_array  ... and rows == cols (`what` names the matrix in that message)
//   validate_out_array       an output `what` of exactly (rows, cols) whose view is injective
//   validate_label_array     the label array `what` of member i: one row of n entries (rows 1,
//                            cols n, column stride >= 0) of SC_DTYPE_I64 / I32, as an input also
//                            F64 / F32; an `output` has entries that share no address
int validate_array(sc_handle h, const sc_array* a);
int validate_kmeans_array(sc_handle h, const sc_array* a);
int validate_affinity_array(sc_handle h, const sc_array* a, const char* what = "affinity");
int validate_out_array(sc_handle h, const sc_array* a, const char* what, int rows, int cols);
int validate_label_array(sc_handle h, const sc_array* a, const char* what, int i, int64_t n,
                         bool output);
// is p memory of the handle's device?  (the one pointer query of every descriptor check)
bool is_device_memory_of(sc_handle h, const void* p);
// no two indices of a (rows, cols) view of element strides (rs, cs) share an address
bool view_is_injective(long long rows, long long cols, long long rs, long long cs);
// validate_array for every utterance of a batch, and that they share one d: fills ns[i] = rows of
// xs[i], *d (0 for an empty batch) and whether any source lies on the device (the caller then
// waits for its stream before other streams read one).  `labels` (may be null): labels[i] is
// checked too.
int validate_batch_arrays(sc_handle h, const sc_array* xs, int count, std::vector<int>* ns, int* d,
                          bool* device_source, int64_t* const* labels = nullptr);
// what the double* entry points describe: compact host fp64 rows
sc_array host_f64_array(const double* x, int n, int d);
std::vector<sc_array> host_f64_arrays(const double* const* xs, const int* ns, int d, int count);
// host fp64 rows that one hipMemcpy2DAsync moves (col_stride 1, rows that do not overlap)
bool array_is_host_f64_rows(const sc_array& a);
// compact host fp64 rows: what the double* k-means entries take (one copy + k_to_colmajor)
bool array_is_compact_host_f64(const sc_array& a);
// ---- one host staging path (ingest.hip) ------------------------------------------------------
// the first `rows` rows of a host view <-> compact rows of the view's width (what hipMemcpy2D
// cannot describe is gathered before the upload and scattered after the download)
void pack_host_rows(const sc_array& a, int64_t rows, unsigned char* out);
void scatter_host_rows(const unsigned char* in, const sc_array& a, int64_t rows);
// h->Xstage holds `bytes`; before it is reallocated under a stream s that is not the handle's, s
// is waited for
int ensure_stage(sc_handle h, size_t bytes, hipStream_t s);
// host rows at their own width -> device memory `stage` of row pitch `pitch` bytes on s: the only
// place that decides between hipMemcpy2DAsync and gather-then-copy (into `packed`; *sync is set
// then: wait for s while `packed` lives)
int stage_host_rows(sc_handle h, const sc_array& a, void* stage, size_t pitch, hipStream_t s,
                    std::vector<unsigned char>* packed, bool* sync);
// ---- ingest: validated sources -> the handle's fp64 buffers (ingest.hip) ---------------------
// sc_set_embeddings for a described source, on `stream` (nullptr: the handle's): sizes the
// arena, sets the problem, widens the rows into h->X; `sync` waits for the stream
int ingest_embeddings(sc_handle h, const sc_array& a, bool sync, hipStream_t stream = nullptr);
// its copy / widening step alone, into any buffer of row pitch ldx doubles (the stream pool's
// staging rows): *sync is set when the caller must wait for s before the source may go
int ingest_rows_into(sc_handle h, const sc_array& a, double* X, int ldx, hipStream_t s,
                     bool* sync);
// the (n, dim) values of a k-means input, widened, into X[j * ld + r], ld = round_up(n, 16) (rows
// n .. ld - 1 of every column zeroed) on stream s; the caller waits for s before the source may go
int ingest_columns_into(sc_handle h, const sc_array& a, double* X, int ld, hipStream_t s);
// the (n, n) values of an affinity or constraint matrix, widened, into dst (row pitch ld, padding
// columns zeroed) on stream s, and the exact-symmetry flag into *flag (device memory); *sync as
// in ingest_rows_into
int ingest_affinity_into(sc_handle h, const sc_array& a, double* dst, int ld, int* flag,
                         hipStream_t s, bool* sync);
// 64 sources per launch (member z: dsts[z] of pitch matrix_ld(n_z), flags[z]); `stage`
// (affinity_group_stage_bytes) takes the host members at their own width, `table`
// (count * affinity_group_table_bytes()) the descriptors; `host_flags` (may be null) receives the
// flags in the same wait; returns with s synchronised
size_t affinity_group_table_bytes();
size_t affinity_group_stage_bytes(const sc_array* as, int count);
int ingest_affinity_group(sc_handle h, const sc_array* as, int count, double* const* dsts,
                          int* flags, void* stage, void* table, hipStream_t s,
                          int* host_flags = nullptr);
// ---- egress: results where the caller wants them (egress.hip) --------------------------------
// The (rows, cols) fp64 values at src -- element (r, c) at src[r * ld + c], or with
// `column_major` at src[c * ld + r] -- narrowed into the validated `out` on the handle's stream.
// Returns with the stream drained (a host destination is complete, a device one as well).
int egress_matrix(sc_handle h, const double* src, int ld, int rows, int cols, bool column_major,
                  const sc_array& out);
// sc_stage_sym_eig / sc_stage_eig behind their upload (api.hip): the matrix is in B1, the values
// land in `values` and the eigenvectors in E (column-major, pitch round_up(n, 16))
int stage_sym_eig_resident(sc_handle h, int n, int count, int descend, double* values,
                           bool vectors, sc_diag* diag);
int stage_eig_resident(sc_handle h, int n, int count, int descend, double* values, sc_diag* diag);
// sc_run_resident; `from_embeddings` false: the resident affinity is the caller's (no GEMM)
int run_resident(sc_handle h, const sc_config* cfg, int64_t* labels, sc_diag* diag,
                 bool from_embeddings);
// the bodies of sc_predict_batch_streams / sc_predict_batch_grouped on described sources
int predict_batch_streams_impl(sc_handle h, const sc_array* xs, const int* ns, int d, int count,
                               const sc_config* cfg, int64_t* const* labels, sc_diag* diags,
                               int streams);
int predict_batch_grouped_impl(sc_handle h, const sc_array* xs, const int* ns, int d, int count,
                               const sc_config* cfg, int64_t* const* labels, sc_diag* diags,
                               int group);
// the body of sc_predict_batch_single behind its checks (check may be null: the grouped batch;
// single may be null); the caller has synchronised h->stream when a source is on the device
int predict_batch_single_impl(sc_handle h, const sc_array* xs, const int* ns, int d, int count,
                              const sc_config* cfg, const sc_single_check* check,
                              int64_t* const* labels, sc_diag* diags, int group,
                              int32_t* single);

// sc_ahc on the embeddings resident in h->X (ingest_embeddings): callers_api.hip.  max_height
// (may be null): the largest merge height of the tree.
int ahc_resident(sc_handle h, int linkage, int n_clusters, double distance_threshold,
                 int64_t* labels, int* n_clusters_out, double* max_height = nullptr);

int ensure_eig(sc_handle h, int n);

int ensure_gen(sc_handle h, int n);

// k: clusters the k-means stage will be asked for (buffers grow past the 64-cluster default)
int ensure_kmeans(sc_handle h, int n, int k = kMaxVectors);
int ensure_vectors(sc_handle h, int n, int cols);

inline int check_last(sc_handle h, const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    h->err = std::string(what) + ": " + hipGetErrorString(e);
    return SC_ERR_HIP;
  }
  return SC_OK;
}


// ---- shared between the translation units -------------------------------------------
int h2d_matrix(sc_handle h, const double* src, int rows, int cols, double* dst, int ld);
int d2h_matrix(sc_handle h, const double* src, int ld, int rows, int cols, double* dst);
int validate_config(sc_handle h, const sc_config* cfg);
// utils.compute_number_of_clusters on a host array (api.hip)
void eigengap_core(const double* w, int count, int max_clusters, double stop_eigenvalue,
                   int eigengap_type, int descend, double wmax, int* n_clusters,
                   double* max_delta);

// eigen drivers (eig_driver.hip)
struct EigRequest {
  int descend;          // 1: report largest first (w = theta); 0: w = -theta ascending
  int max_clusters;     // 0 = None
  int min_clusters;     // 0 = None
  double stop_eigenvalue;
  int eigengap_type;
  int use_stop;         // stop_eigenvalue only on the descending branch
  double value_tol, vector_tol;
  int max_cycles;
  int fixed_count;      // > 0: plain "count extreme eigenpairs" request (stage API)
  // General path only.  Consumed eigenvalues deep in a dense bulk converge arbitrarily
  // slowly in a small Krylov basis, yet cannot influence the result: only the two values
  // that form the maximum gap (and the normaliser of NormalizedDiff) are held to value_tol;
  // the others must be accurate enough that, with their residual intervals, no other gap
  // can reach the maximum and no comparison with stop_eigenvalue can flip.
  int decision_aware = 0;
  // General path, internal (gen_topk's far-end solve, eig_driver.hip): the operator with the
  // opposite sign -- the eigenvalues of largest real part of +L instead of -L; give up with
  // SC_ERR_NOT_CONVERGED instead of landing on the dense route; and, for the main solve that
  // follows, np.max(eigenvalues) of the ascending NormalizedDiff rule as that solve found it.
  int negate = 0;
  int no_dense = 0;
  int have_far = 0;
  double far_value = 0.0;
};

struct EigDecision {
  bool enough = false;     // basis large enough to take a decision
  bool converged = false;
  int kw = 0;              // eigenvalues reported
  int kvec = 0;            // vectors that must be accurate
  int n_clusters_raw = 0;
  double max_delta = 0.0;
  double max_resid = 0.0;
  bool unsupported = false;
  int fail_kind = 0;       // 1 consumed value, 2 far-end value, 3 vector, 4 decision (trace)
  int fail_index = -1;
};

// Where eig_ncluster_impl(front_only) left the refined matrix -- and the operator a symmetric
// solve works on: Op = diag(p) + diag(c) S diag(c), S = `matrix`, the scaling vectors c, p in
// the handle (sym_topk).
struct FrontResult {
  const double* matrix = nullptr;
  double* scratch = nullptr;  // a free n x ld matrix (the dense routes materialise Op there)
  int ld = 0;
  bool symmetric = false, folded_rownorm = false;
  // matrix-free Diffuse: `matrix` is the symmetric A BEFORE Diffuse (the operator applies it
  // twice), the row statistics of S = A A^T are in the handle, its overflow record in h_free;
  // the scaling vectors were built for this Laplacian and folded_rownorm
  bool free_op = false;
  int laplacian_type = 0;
  // flags[13..15] were cleared by the scaling kernel: the first start of the fused chain skips
  // its fill
  bool chain_flags_cleared = false;
  // the lockstep group solve saw this problem latch the fused chain: the host-driven chain
  bool skip_fused = false;
  // which branches the front took (sc_stage_front reports them; nothing else reads them):
  // the threshold pass wrote the digits of the matrix-free Diffuse; S = A A^T was formed by the
  // fp64 product (then `scratch` still holds A); where the CropDiagonal value came from (0: no
  // value vector -- the op ran unfused or not at all, 1: the affinity epilogue, 2: k_crop_value);
  // which kernel made the cut vector (0: none, 1: k_cut_from_partials, 2: k_cut_from_rows,
  // 3: k_row_percentile_cut)
  bool digits_fused = false, diffuse_explicit = false;
  int crop_source = 0, cut_kernel = 0;
};
EigRequest make_eig_request(const sc_config* cfg);
int upload_blur_weights(sc_handle h, const sc_config* cfg);  // into h->blurw, on h->stream
// one refinement op `in` -> `out` (distinct buffers) with the single call's unfused kernel
int run_refine_op(sc_handle h, int op, const sc_config* cfg, const double* in, double* out, int n,
                  int ld);
// `resume`: the stages before the eigensolver already ran (a FrontResult of this handle)
// `stop_before_solver`: run the front exactly as a full call does -- every routing decision as
// it is, unlike `front_only` -- then report where it left things and return before the solver
int eig_ncluster_impl(sc_handle h, const sc_config* cfg, sc_diag* diag, FrontResult* front_only,
                      const FrontResult* resume = nullptr, bool defer_timing = false,
                      FrontResult* stop_before_solver = nullptr);
// RandomState(0) stream of the k-means seeding: the uniform that picks the first centre, the
// trial count 2 + int(log k), and the (k - 1) * trials doubles after it (kmeans_api.hip)
void kmeans_seed_constants(int k, double* u_first, int* trials, std::vector<double>* rnd);
KmeansWorkspace kmeans_workspace(sc_handle h);

// One member of a lockstep group solve (eig_driver.hip: sym_topk_group).
struct GroupEigMember {
  sc_handle h = nullptr;      // arena of the member (its matrix ready on lead->stream)
  const double* S = nullptr;  // refined symmetric matrix, scaling vectors resident in h
  int ld = 0, n = 0;
  EigRequest rq;
  // results
  int status = 0;             // 0 solved; 1 needs the single-call path (rare branch taken)
  EigDecision dc;
  std::vector<double> w;      // consumed eigenvalues (reference order)
  int basis = 0, passes = 0;
  bool skip_fused = false;    // (status 1) the fused chain latched: a re-solve takes the host chain
  // matrix-free Diffuse: S is the symmetric A before Diffuse, the operator is
  // diag(p) + diag(c) A A diag(c) (two block products per step, through h->fY)
  bool free_op = false;
};
// Block Lanczos of up to kGroupMax members in lockstep: one launch per chain link / matvec
// for the whole group, one host synchronisation per Rayleigh-Ritz check for the whole group.
// Leaves Ritz vectors in every solved member's h->E (h->n_vec set).
// `want_vectors` false: eigenvalues and the eigengap decision only (AutoTune sweep).
int sym_topk_group(sc_handle lead, GroupEigMember* mem, int count, bool want_vectors = true);
// The dense Jacobi solve of up to kShortWidth members of n <= kDenseMax in one launch (a
// workgroup each), one synchronisation: every eigenpair of each, eigenvectors in h->E.  Fills
// status, dc, w, basis like sym_topk_group; SC_ERR_NON_FINITE when a member's front flagged it.
int dense_topk_group(sc_handle lead, GroupEigMember* mem, int count);
// `any_size`: also n >= 4096 (the group takes the upper-triangle matvec there)
bool sym_group_eligible(int n, const EigRequest& rq, bool any_size = false);

// the symmetric operator `op` (op.scratch: the dense routes' n x ld matrix)
int sym_topk(sc_handle h, const FrontResult& op, int n, const EigRequest& rq, sc_diag* diag,
             EigDecision* out_dc, std::vector<double>* out_w);
// `scratch`: a free n x ld matrix (the dense Hessenberg route reduces a copy of M there; may be
// null for n <= 64)
int gen_topk(sc_handle h, const double* M, int ld, int n, int laplacian_type,
             const EigRequest& rq, sc_diag* diag, EigDecision* out_dc,
             std::vector<double>* out_w, double* scratch);
// two steps of the general path that its test entries (stage_dense.hip) run as the solver does:
// power-of-two scaling + Hessenberg reduction of B in place, and the explicit residuals of the
// first `count` Ritz pairs, 32 per launch (eig_driver.hip)
int hessenberg_reduce_scaled(sc_handle h, double* B, int ld, int n, double* absmax, double* tau,
                             double* vwork, double* eig_scale);
void gen_residuals(hipStream_t s, const double* Q, const double* OpQ, int m, int n,
                   const double* Yre, const double* Yim, const double* theta_re,
                   const double* theta_im, int count, double* partial, double* resid);

// matrix-free Diffuse (free_api.hip)
// does this call take the matrix-free route for a Diffuse whose output only feeds
// RowWiseNormalize / the Laplacian?  (mode of the handle, problem size, request)
bool free_diffuse_wanted(sc_handle h, const sc_config* cfg, int n, const EigRequest& rq,
                         bool in_group = false);
// the statistics of a group (free_api.hip): prepare before the grouped threshold pass (which
// writes the digits), digits after it, end after the grouped digit product
int free_group_prepare(sc_handle* hs, const double* const* A, const double* const* cuts,
                       const double* ps, int count, const int* lds, const int* ns, hipStream_t s,
                       double floor_value, struct FreeItem* items, struct TsDigits* digits);
int free_group_digits(sc_handle* hs, const struct FreeItem* items, int count, hipStream_t s);
int free_group_end(sc_handle* hs, const struct FreeItem* items, int count, hipStream_t s);
int free_fused_prepare(sc_handle h, hipStream_t s, int n, const double* cut, double p,
                       double floor_value);
// what the statistics left in h->h_free, once their stream has drained (sc_stage_front)
void free_front_info(sc_handle h, int* candidates, int* overflow_rows, int* forms_s);
// enqueue the statistics of S = A A^T (h->rowmax, h->rowsum) on h->stream; no synchronisation.
// The overflow words travel to h->h_free behind them.
// `have_amax`: h->fscal[0] already holds max|a| (or an upper bound of it) for this A
int free_diffuse_stats(sc_handle h, const double* A, int ld, int n, bool have_amax = false,
                       bool digits_ready = false);
int ensure_free(sc_handle h, int n);
// the same pipeline in pieces on a given stream (the AutoTune sweep runs the digit product of
// all its members as one grouped launch between them): max|a| + digits | ... | candidates +
// exact statistics + the overflow words on their way to h->h_free
int free_product(sc_handle h, hipStream_t s, int n);
int free_stats_begin(sc_handle h, hipStream_t s, const double* A, int ld, int n, bool have_amax);
int free_stats_end(sc_handle h, hipStream_t s, const double* A, int ld, int n, bool timed,
                   const int* plan = nullptr);
// after the stream has drained: rows with more candidates than the cap are evaluated in full.
// *changed: rowmax was rewritten (the scaling vectors must be rebuilt); *too_many: more such
// rows than the exact route takes (the caller forms S explicitly).
int free_fix_overflow(sc_handle h, const double* A, int ld, int n, bool* changed, bool* too_many);
// W = p .* V + c .* (A (A Vs)) through h->fY (both halves on h->stream)
void free_apply_operator(sc_handle h, const double* A, int ld, int n, bool sym_mv,
                         const double* V, int ldv);
// ... on explicit buffers (what the form above passes from the handle): fY n x 8 scratch,
// slabs matvec_sym_workspace_doubles(n) doubles when sym_mv
void free_apply_operator(hipStream_t s, const double* A, int ld, int n, bool sym_mv,
                         const double* cvec, const double* pvec, const double* V, int ldv,
                         const double* Vs, double* fY, double* W, double* slabs);
bool wants_full_spectrum(const EigRequest& rq);

// constraints (constraint_api.hip)
int device_is_symmetric(sc_handle h, const double* m, int n, int ld, bool* out);
int adjust_affinity(sc_handle h, const sc_config* cfg, const double* a, bool sym_a, double* out,
                    int n, int ld);
bool constraint_active(sc_handle h, const sc_config* cfg, bool before);
// One member of a grouped ConstraintPropagation chain (constraint_propagation_group): a symmetric
// affinity A (n x ld, adjusted in place), four n x ld work matrices, two n-vectors, the band of
// n - 1 values and the tile order of the symmetric GEMM for n, all on the device.  n = 0: idle.
struct CpGroupMember {
  int n = 0, ld = 0;
  double* A = nullptr;
  double *P = nullptr, *T = nullptr, *Pn = nullptr, *Tn = nullptr;
  double *deg = nullptr, *rowmax = nullptr;
  const double* band = nullptr;
  const int2* tilemap = nullptr;
  // pairs: the constraint is not the band but pk <= n directed entries Q[prows[e], pcols[e]] =
  // pvals[e] on the device (psym: the list is symmetric); pk = 0 leaves A as it is
  bool pairs = false, psym = false;
  int pk = 0;
  const int32_t *prows = nullptr, *pcols = nullptr;
  const double* pvals = nullptr;
  // q: the constraint is neither but a dense SYMMETRIC matrix on the device (n x ld, the arena's
  // Cq); band and the entry fields are not read
  const double* q = nullptr;
};
int constraint_propagation_group(sc_handle lead, hipStream_t s, const CpGroupMember* mem,
                                 int count, double alpha);
// sc_set_constraint_pairs' checks of a host entry list, and whether it is symmetric
int validate_constraint_pairs(sc_handle h, const int32_t* rows, const int32_t* cols,
                              const double* vals, int count, int n, bool* symmetric);
// vals | rows | cols as Cpairs holds them: 16 bytes per entry
std::vector<double> pack_constraint_pairs(const int32_t* rows, const int32_t* cols,
                                          const double* vals, int count);
// the body of sc_predict_batch_constraints (batch_group.hip); cons == nullptr: no constraints
int predict_batch_constrained_impl(sc_handle h, const sc_array* xs, const sc_constraint_desc* cons,
                                   const int* ns, int d, int count, const sc_config* cfg,
                                   int64_t* const* labels, sc_diag* diags, int group,
                                   bool affinities = false,  // (xs are the callers' affinities)
                                   // per utterance, data != nullptr: its dense constraint source
                                   const sc_array* dense = nullptr);

// ---- the single-cluster test (callers_api.hip: the single call's; single_check.hip: a batch's)
// the bodies of sc_affinity_stats / sc_affinity_gmm_bic on the affinity resident in h
int affinity_stats_impl(sc_handle h, double* out);
int affinity_gmm_bic_impl(sc_handle h, int diagonal_offset, double* bic1, double* bic2);
struct SingleMember {
  const double* a;  // device memory, n x ld
  int n, ld;
};
int validate_single_check(sc_handle h, const sc_single_check* opt);
// AffinityGmmBic needs diagonal_offset < n - 1: sc_affinity_gmm_bic's message with the index
int check_single_offset(sc_handle h, const sc_single_check* opt, int n, int index);
// The decision of `count` members on stream `s` (synchronised on return): values (may be NULL):
// 8 doubles per member {min, neighbour min, mean, std, bic1, bic2, lloyd steps, em steps}; single:
// the verdicts.  _wave: members of n <= kDenseMax, kScShortMax per launch; _group: up to kGroupMax
// members of kDenseMax < n < kScChainMaxN; _resident: the affinity resident in h, any n, through
// the single call's kernels.
int single_check_wave(sc_handle lead, hipStream_t s, const SingleMember* ms, int count,
                      const sc_single_check* opt, double* values, int32_t* single);
int single_check_group(sc_handle lead, hipStream_t s, const SingleMember* ms, int count,
                       const sc_single_check* opt, double* values, int32_t* single);
int single_check_resident(sc_handle h, const sc_single_check* opt, double* values,
                          int32_t* single);

#endif  // SPECTRALCLUSTER_AMD_HANDLE_H_
