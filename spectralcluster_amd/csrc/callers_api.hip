// Host side of the callers around the spectral path: tree
// bookkeeping of the agglomerative clustering, centroids, fallback decisions, naive
// clusterer; kernels in ahc.hip and fallback.hip.
#include "ahc_tree.h"
#include "gmm_common.h"
#include "handle.h"

// ------------------------------------------------------------------------------
// N4: size reduction -- agglomerative clustering + centroids
// ------------------------------------------------------------------------------
// sklearn.cluster.AgglomerativeClustering(metric="cosine", linkage=complete|average,
// n_clusters=... | distance_threshold=...).fit_predict(X), label numbering included.
extern "C" int sc_ahc(sc_handle h, const double* x, int n, int d, int linkage, int n_clusters,
                      double distance_threshold, int64_t* labels, int* n_clusters_out) {
  if (!h) return SC_ERR_INVALID;
  if (!x || !labels || d <= 0) return fail(h, SC_ERR_INVALID, "embeddings must be (n, d)");
  if (n < 2)
    return fail(h, SC_ERR_INVALID,
                "Found array with " + std::to_string(std::max(n, 0)) +
                    " sample(s) while a minimum of 2 is required by AgglomerativeClustering.");
  if (linkage != SC_LINKAGE_COMPLETE && linkage != SC_LINKAGE_AVERAGE)
    return fail(h, SC_ERR_INVALID, "linkage must be complete or average");
  if (n_clusters < 0 || n_clusters > n)
    return fail(h, SC_ERR_INVALID, "Cannot extract more clusters than samples");
  SC_HIP(h, hipSetDevice(h->device));
  SC_TRY(sc_set_embeddings(h, x, n, d));
  return ahc_resident(h, linkage, n_clusters, distance_threshold, labels, n_clusters_out);
}

// The distance step of sc_ahc on the rows resident in h->X: the affinity stage's normalise +
// symmetric GEMM, then 1 - clip(c), into h->B1 (pitch h->ldn).  *bad_out: the device word behind
// the chain that a zero or non-finite row latches (D would hold NaNs).
static int ahc_resident_distances(sc_handle h, int** bad_out) {
  const int n = h->n, d = h->d;
  SC_TRY(ensure_tilemap(h, n));
  hipStream_t s = h->stream;
  const int ld = h->ldn;
  SC_TRY(grow(h, h->ahc_size, (size_t)n * sizeof(int)));
  SC_TRY(grow(h, h->ahc_chain, ((size_t)n + 1) * sizeof(int)));
  SC_TRY(grow(h, h->ahc_Z, (size_t)n * 4 * sizeof(double)));
  int* bad_d = ptr<int>(h->ahc_chain) + n;
  SC_HIP(h, hipMemsetAsync(bad_d, 0, sizeof(int), s));
  launch_normalize_rows(s, ptr<double>(h->X), h->ldx, n, d, ptr<double>(h->Xn), bad_d);
  // No split-K workspace: every tile takes the whole K, as in the grouped product of a batch.  A
  // split tail (more upper-triangle tiles than workgroup slots: n > 3968 on 256 CUs, d >= 241)
  // sums the columns of its tiles in two chunks and those of the whole tiles in one, so two equal
  // rows got distance columns that differ in the last bit -- scipy's pdist gives them equal
  // ones, and every tie of the chain depends on it.
  launch_gemm_nt(s, ptr<double>(h->Xn), h->ldx, ptr<double>(h->Xn), h->ldx, ptr<double>(h->B1),
                 ld, n, n, d, kEpiNone, true, nullptr, h->tilemap_cur);
  launch_cosine_distance(s, ptr<double>(h->B1), n, ld);
  *bad_out = bad_d;
  return SC_OK;
}

// ... on the n >= 2 rows resident in h->X; the arguments have been checked
int ahc_resident(sc_handle h, int linkage, int n_clusters, double distance_threshold,
                 int64_t* labels, int* n_clusters_out, double* max_height) {
  const int n = h->n;
  hipStream_t s = h->stream;
  const int ld = h->ldn;
  int* bad_d = nullptr;
  SC_TRY(ahc_resident_distances(h, &bad_d));
  launch_ahc_nn_chain(s, ptr<double>(h->B1), ld, n, linkage, ptr<int>(h->ahc_size),
                      ptr<int>(h->ahc_chain), ptr<double>(h->ahc_Z), bad_d);
  SC_TRY(check_last(h, "agglomerative clustering launch"));
  std::vector<double> Z((size_t)(n - 1) * 4);
  int bad = 0;
  SC_HIP(h, hipMemcpyAsync(Z.data(), h->ahc_Z.p, Z.size() * sizeof(double),
                           hipMemcpyDeviceToHost, s));
  SC_HIP(h, hipMemcpyAsync(&bad, bad_d, sizeof(int), hipMemcpyDeviceToHost, s));
  SC_HIP(h, hipStreamSynchronize(s));
  h->have_affinity = h->have_cropval = false;
  if (bad) return fail(h, SC_ERR_INVALID, "embeddings contain a zero or non-finite row");
  // sort, union-find relabelling and the heap cut: ahc_tree.cpp
  const int k = ahc_tree_cut(Z.data(), n, n_clusters, distance_threshold, labels);
  if (n_clusters_out) *n_clusters_out = k;
  if (max_height) {
    double top = Z[2];
    for (int m = 1; m < n - 1; ++m) top = std::max(top, Z[(size_t)m * 4 + 2]);
    *max_height = top;
  }
  return SC_OK;
}

// utils.get_cluster_centroids (reference utils.py:159-176): (k, d) means, k = max(labels)+1
extern "C" int sc_cluster_centroids(sc_handle h, const double* x, int n, int d,
                                    const int64_t* labels, int k, double* out) {
  if (!h) return SC_ERR_INVALID;
  if (!x || !labels || !out || n <= 0 || d <= 0 || k <= 0)
    return fail(h, SC_ERR_INVALID, "embeddings must be (n, d), labels (n,)");
  SC_HIP(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  SC_TRY(grow(h, h->ahc_lab, (size_t)n * sizeof(int)));
  SC_TRY(grow(h, h->ahc_cent, (size_t)(n + k) * d * sizeof(double)));
  std::vector<int> lab32(n);
  for (int i = 0; i < n; ++i) lab32[i] = (int)labels[i];
  double* xd = ptr<double>(h->ahc_cent);
  double* cd_ = xd + (size_t)n * d;
  SC_HIP(h, hipMemcpyAsync(xd, x, (size_t)n * d * sizeof(double), hipMemcpyHostToDevice, s));
  SC_HIP(h, hipMemcpyAsync(h->ahc_lab.p, lab32.data(), (size_t)n * sizeof(int),
                           hipMemcpyHostToDevice, s));
  launch_cluster_centroids(s, xd, d, n, d, ptr<int>(h->ahc_lab), k, cd_);
  SC_TRY(check_last(h, "centroid launch"));
  SC_HIP(h, hipMemcpyAsync(out, cd_, (size_t)k * d * sizeof(double), hipMemcpyDeviceToHost, s));
  SC_HIP(h, hipStreamSynchronize(s));
  return SC_OK;
}

// ------------------------------------------------------------------------------
// stage/test entries of the linkage kernels (ahc.hip): every form on a caller's cosine matrices
// ------------------------------------------------------------------------------
namespace {

struct StageBlock {  // the one device allocation of a call, freed when it returns
  void* p = nullptr;
  ~StageBlock() {
    if (p) (void)hipFree(p);
  }
};

constexpr int kStageGuard = 0x5a5a5a5a;  // the int behind a member's cluster sizes
// What the padding of a matrix holds: the value a scan would take for the smallest distance.  The
// LDS kernels turn cosines into distances while they load them (cosine 1: distance 0); the chain
// kernels scan what their distance kernel left, and that kernel works on the n x n part alone
// (-1: below every distance).
constexpr double kStagePadLds = 1.0, kStagePadChain = -1.0;

}  // namespace

extern "C" int sc_stage_linkage(sc_handle h, int form, int method, int count, const int32_t* ns,
                                const double* cosines, int first, double threshold,
                                const int32_t* bad, double* Z, double* records, int64_t* labels,
                                int n_clusters, double distance_threshold) {
  if (!h) return SC_ERR_INVALID;
  if (!ns || !cosines || count < 1) return fail(h, SC_ERR_INVALID, "bad linkage input");
  if (form < SC_LINKAGE_FORM_SINGLE || form > SC_LINKAGE_FORM_LDS_VERDICT)
    return fail(h, SC_ERR_INVALID, "linkage form: 0 .. 6");
  if (method != SC_LINKAGE_COMPLETE && method != SC_LINKAGE_AVERAGE)
    return fail(h, SC_ERR_INVALID, "linkage must be complete or average");
  const bool lds = form == SC_LINKAGE_FORM_BATCH_LDS || form == SC_LINKAGE_FORM_POOL_LDS ||
                   form == SC_LINKAGE_FORM_LDS_VERDICT;
  const bool verdict = form == SC_LINKAGE_FORM_CHAIN_VERDICT || form == SC_LINKAGE_FORM_LDS_VERDICT;
  const bool pool = form == SC_LINKAGE_FORM_POOL || form == SC_LINKAGE_FORM_POOL_LDS;
  if ((lds || verdict) && method != SC_LINKAGE_AVERAGE)
    return fail(h, SC_ERR_INVALID, "the LDS and the verdict forms take average linkage only");
#if SC_POOL_LDS_LINKAGE_MAX == 0
  if (lds) return fail(h, SC_ERR_UNSUPPORTED, "the library was built without the LDS linkage");
#endif
  if (first < 0 || first >= count) return fail(h, SC_ERR_INVALID, "first must be a member");
  if ((form == SC_LINKAGE_FORM_SINGLE || form == SC_LINKAGE_FORM_POOL) && first != 0)
    return fail(h, SC_ERR_INVALID, "forms 0 and 3 have no table offset: first must be 0");
  if (verdict ? !records : !Z) return fail(h, SC_ERR_INVALID, "the form's output is NULL");
  if (verdict && labels) return fail(h, SC_ERR_INVALID, "a verdict form leaves no tree to cut");
  if (pool && bad) return fail(h, SC_ERR_INVALID, "the pool forms have no bad words");
  int max_all = 0, max_run = 0;  // the largest member; the largest one the launches work on
  for (int i = 0; i < count; ++i) {
    if (ns[i] < 0) return fail(h, SC_ERR_INVALID, "a member has a negative row count");
    if (lds && ns[i] > kPoolLdsLinkageMax)
      return fail(h, SC_ERR_INVALID, "the LDS forms take members of at most " +
                                         std::to_string(kPoolLdsLinkageMax) + " rows");
    max_all = std::max(max_all, ns[i]);
    const bool runs = i >= first && ns[i] >= 2 && !(bad && bad[i] != 0);
    if (runs) max_run = std::max(max_run, ns[i]);
    if (runs && labels && (n_clusters < 0 || n_clusters > ns[i]))
      return fail(h, SC_ERR_INVALID, "Cannot extract more clusters than samples");
  }
  if (max_run < 2) return fail(h, SC_ERR_INVALID, "no member of two or more rows to work on");
  SC_HIP(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;

  // One allocation: table | slots | rows | per member (or per pool slot) D, then size + guard +
  // chain + bad word | Z | records.  Every matrix has padding columns and two padding rows.
  auto align = [](size_t b) { return (b + 255) / 256 * 256; };
  const int pool_ld = round_up(max_all, 16) + 16;
  const int pool_n = max_all + 1;  // ints per position: the last one stays the guard
  const size_t pool_z = 4 * (size_t)std::max(max_all - 1, 1);
  std::vector<size_t> d_at(count), i_at(count), z_at(count), c_at(count), l_at(count);
  std::vector<int> lds_(count);
  size_t at = align((size_t)count * sizeof(AhcBatchItem));
  const size_t slots_at = at;
  at += align(2 * (size_t)count * sizeof(int));
  size_t z_doubles = 0, c_doubles = 0, rows_total = 0;
  for (int i = 0; i < count; ++i) {
    const int n = ns[i];
    lds_[i] = pool ? pool_ld : round_up(n, 16) + 16;
    d_at[i] = at;  // (pool: of SLOT i)
    at += align((size_t)((pool ? max_all : n) + 2) * lds_[i] * sizeof(double));
    z_at[i] = z_doubles;
    z_doubles += 4 * (size_t)std::max(n - 1, 0);
    c_at[i] = c_doubles;
    c_doubles += (size_t)n * n;
    l_at[i] = rows_total;
    rows_total += (size_t)n;
  }
  const size_t ints_at = at;  // pool: sizes of every position, then chains; else per member
  for (int i = 0; i < count; ++i) {
    i_at[i] = at;
    at += pool ? 0 : align((2 * (size_t)ns[i] + 2) * sizeof(int));
  }
  if (pool) at += align(2 * (size_t)count * pool_n * sizeof(int));
  const size_t out_at = at;
  const size_t out_doubles = verdict ? 2 * (size_t)count : (pool ? count * pool_z : z_doubles);
  at += align(out_doubles * sizeof(double));
  const size_t total = at;

  StageBlock block;
  SC_HIP(h, hipMalloc(&block.p, total));
  char* dev = static_cast<char*>(block.p);
  std::vector<char> image(total, 0);
  char* img = image.data();
  AhcBatchItem* table_h = reinterpret_cast<AhcBatchItem*>(img);
  const AhcBatchItem* table_d = reinterpret_cast<const AhcBatchItem*>(dev);
  int* slots_h = reinterpret_cast<int*>(img + slots_at);
  int* rows_h = slots_h + count;
  const int* slots_d = reinterpret_cast<const int*>(dev + slots_at);
  const int* rows_d = slots_d + count;
  double* out_h = reinterpret_cast<double*>(img + out_at);
  double* out_d = reinterpret_cast<double*>(dev + out_at);
  // what the caller's outputs hold goes up first: a member the launches leave alone keeps it
  if (verdict) {
    std::memcpy(out_h, records, 2 * (size_t)count * sizeof(double));
  } else {
    for (int i = 0; i < count; ++i)
      std::memcpy(out_h + (pool ? i * pool_z : z_at[i]), Z + z_at[i],
                  4 * (size_t)std::max(ns[i] - 1, 0) * sizeof(double));
  }
  PoolSlabs p{};
  p.D = reinterpret_cast<double*>(dev + d_at[0]);
  p.stride_d = count > 1 ? (d_at[1] - d_at[0]) / sizeof(double) : 0;
  p.ldd = pool_ld;
  p.size = reinterpret_cast<int*>(dev + ints_at);
  p.chain = p.size + (size_t)count * pool_n;
  p.stride_n = pool_n;
  p.Z = out_d;
  p.stride_z = pool_z;
  for (int i = 0; i < count; ++i) {
    const int n = ns[i];
    slots_h[i] = count - 1 - i;  // position i works in slot count - 1 - i
    rows_h[i] = n;
    const int slot = pool ? slots_h[i] : i;
    const int ld = lds_[i];
    const int rows = (pool ? max_all : n) + 2;
    double* D_h = reinterpret_cast<double*>(img + d_at[slot]);
    std::fill(D_h, D_h + (size_t)rows * ld, lds ? kStagePadLds : kStagePadChain);
    for (int r = 0; r < n; ++r)
      std::memcpy(D_h + (size_t)r * ld, cosines + c_at[i] + (size_t)r * n,
                  (size_t)n * sizeof(double));
    int* ints_h = reinterpret_cast<int*>(img + (pool ? ints_at : i_at[i]));
    if (pool) {
      for (int half = 0; half < 2; ++half)
        std::fill(ints_h + ((size_t)half * count + i) * pool_n,
                  ints_h + ((size_t)half * count + i + 1) * pool_n, kStageGuard);
    } else {
      std::fill(ints_h, ints_h + 2 * n + 1, kStageGuard);
      ints_h[2 * n + 1] = bad ? bad[i] : 0;  // the word sits behind the chain, as in sc_ahc
    }
    AhcBatchItem& it = table_h[i];
    it = AhcBatchItem{};
    it.n = n;
    it.ld = ld;
    it.method = method;
    it.D = reinterpret_cast<double*>(dev + d_at[i]);
    it.size = reinterpret_cast<int*>(dev + i_at[i]);
    it.chain = it.size + n + 1;
    it.bad = it.chain + n;
    it.Z = out_d + (verdict ? 2 * (size_t)i : z_at[i]);
  }
  SC_HIP(h, hipMemcpyAsync(dev, img, total, hipMemcpyHostToDevice, s));
  const int cnt = count - first;
  switch (form) {
    case SC_LINKAGE_FORM_SINGLE:
      for (int i = 0; i < count; ++i) {
        const AhcBatchItem& it = table_h[i];
        if (it.n < 2) continue;  // (sc_ahc refuses them)
        launch_cosine_distance(s, it.D, it.n, it.ld);
        launch_ahc_nn_chain(s, it.D, it.ld, it.n, method, it.size, it.chain, it.Z, it.bad);
      }
      break;
    case SC_LINKAGE_FORM_BATCH:
      launch_batch_cosine_distance(s, table_d, first, cnt, max_run);
      launch_batch_nn_chain(s, table_d, first, cnt);
      break;
    case SC_LINKAGE_FORM_POOL:
      launch_pool_cosine_distance(s, p, slots_d, rows_d, count, max_run);
      launch_pool_nn_chain(s, p, slots_d, rows_d, count, method);
      break;
    case SC_LINKAGE_FORM_CHAIN_VERDICT:
      launch_batch_cosine_distance(s, table_d, first, cnt, max_run);
      launch_batch_nn_chain_verdict(s, table_d, first, cnt, threshold);
      break;
#if SC_POOL_LDS_LINKAGE_MAX > 0
    case SC_LINKAGE_FORM_BATCH_LDS:
      launch_batch_linkage_lds(s, table_d, first, cnt, max_run);
      break;
    case SC_LINKAGE_FORM_POOL_LDS:
      launch_pool_linkage_lds(s, p, slots_d, rows_d, first, cnt, max_run);
      break;
    case SC_LINKAGE_FORM_LDS_VERDICT:
      launch_batch_linkage_lds_verdict(s, table_d, first, cnt, max_run, threshold);
      break;
#endif
    default:
      break;
  }
  SC_TRY(check_last(h, "linkage stage launch"));
  SC_HIP(h, hipMemcpyAsync(img + ints_at, dev + ints_at, total - ints_at, hipMemcpyDeviceToHost,
                           s));
  SC_HIP(h, hipStreamSynchronize(s));
  // nothing wrote behind a member's sizes or its chain
  for (int i = 0; i < count; ++i) {
    const int n = ns[i];
    bool ok = true;
    if (pool) {
      const int* ints_h = reinterpret_cast<const int*>(img + ints_at);
      for (int half = 0; half < 2; ++half)
        for (int e = n; e < pool_n; ++e)
          ok = ok && ints_h[((size_t)half * count + i) * pool_n + e] == kStageGuard;
    } else {
      const int* ints_h = reinterpret_cast<const int*>(img + i_at[i]);
      ok = ints_h[n] == kStageGuard && ints_h[2 * n + 1] == (bad ? bad[i] : 0);
    }
    if (!ok)
      return fail(h, SC_ERR_HIP, "linkage stage: member " + std::to_string(i) +
                                     " wrote behind its cluster sizes or its chain");
  }
  if (verdict) {
    std::memcpy(records, out_h, 2 * (size_t)count * sizeof(double));
    return SC_OK;
  }
  for (int i = 0; i < count; ++i)
    std::memcpy(Z + z_at[i], out_h + (pool ? i * pool_z : z_at[i]),
                4 * (size_t)std::max(ns[i] - 1, 0) * sizeof(double));
  if (labels)
    for (int i = first; i < count; ++i)
      if (ns[i] >= 2 && !(bad && bad[i] != 0))
        ahc_tree_cut(Z + z_at[i], ns[i], n_clusters, distance_threshold, labels + l_at[i]);
  return SC_OK;
}

extern "C" int sc_stage_cosine_distances(sc_handle h, int route, const double* x, int n, int d,
                                         double* out) {
  if (!h) return SC_ERR_INVALID;
  if (!x || !out || n < 2 || d <= 0)
    return fail(h, SC_ERR_INVALID, "embeddings must be (n, d), n >= 2");
  if (route != 0 && route != 1) return fail(h, SC_ERR_INVALID, "route: 0 single call, 1 batch");
  SC_HIP(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  int bad = 0;
  if (route == 0) {  // sc_ahc's own distance step
    SC_TRY(sc_set_embeddings(h, x, n, d));
    int* bad_d = nullptr;
    SC_TRY(ahc_resident_distances(h, &bad_d));
    SC_TRY(check_last(h, "distance launch"));
    SC_HIP(h, hipMemcpyAsync(&bad, bad_d, sizeof(int), hipMemcpyDeviceToHost, s));
    SC_TRY(d2h_matrix(h, ptr<double>(h->B1), h->ldn, n, n, out));
    h->have_affinity = h->have_cropval = false;
  } else {  // a wave of one member, as sc_batch_ahc lays it out (batch_reduce.hip)
    auto align = [](size_t b) { return (b + 255) / 256 * 256; };
    const int ldx = round_up(d, 16), ld = matrix_ld(n);
    const size_t rows = align((size_t)n * ldx * sizeof(double));
    const size_t table_bytes = align(sizeof(AhcBatchItem) + sizeof(int));
    const size_t total = table_bytes + 2 * rows + align((size_t)n * ld * sizeof(double));
    StageBlock block;
    SC_HIP(h, hipMalloc(&block.p, total));
    char* dev = static_cast<char*>(block.p);
    SC_HIP(h, hipMemsetAsync(dev, 0, total, s));
    AhcBatchItem it{};
    it.n = n;
    it.ld = ld;
    it.ldx = ldx;
    it.d = d;
    it.bad = reinterpret_cast<int*>(dev + sizeof(AhcBatchItem));
    double* X = reinterpret_cast<double*>(dev + table_bytes);
    it.X = X;
    it.Xn = reinterpret_cast<double*>(dev + table_bytes + rows);
    it.D = reinterpret_cast<double*>(dev + table_bytes + 2 * rows);
    const AhcBatchItem* table_d = reinterpret_cast<const AhcBatchItem*>(dev);
    SC_HIP(h, hipMemcpyAsync(dev, &it, sizeof(it), hipMemcpyHostToDevice, s));
    SC_TRY(h2d_matrix(h, x, n, d, X, ldx));
    launch_batch_normalize(s, table_d, 1, n);
    GemmGroupItem item;
    item.A = it.Xn;
    item.lda = ldx;
    item.C = it.D;
    item.ldc = ld;
    item.n = n;
    item.K = d;
    launch_gemm_nt_group(s, &item, 1, kEpiNone, 0);
    launch_batch_cosine_distance(s, table_d, 0, 1, n);
    SC_TRY(check_last(h, "batched distance launch"));
    SC_HIP(h, hipMemcpyAsync(&bad, it.bad, sizeof(int), hipMemcpyDeviceToHost, s));
    SC_TRY(d2h_matrix(h, it.D, ld, n, n, out));  // (waits for the stream: `it` is a local)
  }
  if (bad) return fail(h, SC_ERR_INVALID, "embeddings contain a zero or non-finite row");
  return SC_OK;
}

// ------------------------------------------------------------------------------
// N4: fallback decisions (reference fallback_clusterer.py, naive_clusterer.py)
// ------------------------------------------------------------------------------
// out = {affinity.min(), np.diag(affinity, k=1).min(), mean, np.std(affinity)} of the
// resident affinity (single-cluster conditions AllAffinity / NeighborAffinity / AffinityStd)
extern "C" int sc_affinity_stats(sc_handle h, double* out) {
  if (!h) return SC_ERR_INVALID;
  if (!out) return fail(h, SC_ERR_INVALID, "out is NULL");
  return affinity_stats_impl(h, out);
}
// (also what a batch runs for a member of n >= 4096: single_check.hip)
int affinity_stats_impl(sc_handle h, double* out) {
  if (!h->have_affinity) return fail(h, SC_ERR_INVALID, "no affinity resident");
  SC_HIP(h, hipSetDevice(h->device));
  const int n = h->n;
  SC_TRY(grow(h, h->fb_part, (size_t)n * 8 * sizeof(double)));
  SC_TRY(grow(h, h->fb_small, 32 * sizeof(double)));
  launch_affinity_stats(h->stream, ptr<double>(h->A0), n, h->ldn, ptr<double>(h->fb_part),
                        ptr<double>(h->fb_small));
  SC_TRY(check_last(h, "affinity statistics launch"));
  SC_HIP(h, hipMemcpyAsync(out, h->fb_small.p, 4 * sizeof(double), hipMemcpyDeviceToHost,
                           h->stream));
  SC_HIP(h, hipStreamSynchronize(h->stream));
  return SC_OK;
}

// BIC of a 1- and a 2-component Gaussian mixture fitted to affinity[i][j], j >= i + offset
// (fallback_clusterer.py:154-173).  sklearn's GaussianMixture defaults: full covariance,
// reg_covar 1e-6, tol 1e-3 on the mean log-likelihood, max_iter 100, k-means start.  The
// reference's k-means start is randomly seeded; here it is the deterministic 1-D 2-means
// from (min, max), which is the fixed point those seeds reach on separable data.
extern "C" int sc_affinity_gmm_bic(sc_handle h, int diagonal_offset, double* bic1,
                                   double* bic2) {
  if (!h) return SC_ERR_INVALID;
  if (!bic1 || !bic2) return fail(h, SC_ERR_INVALID, "NULL output");
  return affinity_gmm_bic_impl(h, diagonal_offset, bic1, bic2);
}
int affinity_gmm_bic_impl(sc_handle h, int diagonal_offset, double* bic1, double* bic2) {
  if (!h->have_affinity) return fail(h, SC_ERR_INVALID, "no affinity resident");
  const int n = h->n;
  if (diagonal_offset < 0 || diagonal_offset >= n - 1)
    return fail(h, SC_ERR_INVALID,
                "single_cluster_affinity_diagonal_offset must be significantly smaller than "
                "affinity matrix dimension");
  SC_HIP(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  SC_TRY(grow(h, h->fb_part, (size_t)n * 8 * sizeof(double)));
  SC_TRY(grow(h, h->fb_small, 32 * sizeof(double)));
  double* params_d = ptr<double>(h->fb_small);
  double* sums_d = params_d + 8;
  const double* a = ptr<double>(h->A0);
  const int ld = h->ldn;
  const double m = (double)(n - diagonal_offset);
  const double count = m * (m + 1.0) / 2.0;
  double sums[8];
  auto pass = [&](int components, int mode, const double* params) -> int {
    SC_HIP(h, hipMemcpyAsync(params_d, params, 6 * sizeof(double), hipMemcpyHostToDevice, s));
    launch_gmm_pass(s, a, n, ld, diagonal_offset, components, mode, params_d,
                    ptr<double>(h->fb_part), sums_d);
    SC_HIP(h, hipMemcpyAsync(sums, sums_d, 7 * sizeof(double), hipMemcpyDeviceToHost, s));
    SC_HIP(h, hipStreamSynchronize(s));
    return SC_OK;
  };
  // M-step of sklearn's _estimate_gaussian_parameters from the pass sums (gmm_common.h)
  auto m_step = [&](int components, double* params) {
    gmm_m_step(sums, components, count, params);
  };
  auto fit = [&](int components, double* bic) -> int {
    double params[6] = {1.0, 0.0, 1.0, 0.0, 0.0, 1.0};
    if (components == 1) {
      SC_TRY(pass(1, 1, params));  // r0 = 1 everywhere: plain moments
      m_step(1, params);
    } else {
      // 2-means start from the extremes, Lloyd steps until the inertia stops moving
      launch_gmm_range(s, a, n, ld, diagonal_offset, ptr<double>(h->fb_part), sums_d);
      double range[2];
      SC_HIP(h, hipMemcpyAsync(range, sums_d, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
      SC_HIP(h, hipStreamSynchronize(s));
      params[1] = range[0];
      params[4] = range[1];
      double prev_inertia = -1.0;
      for (int it = 0; it < 300; ++it) {
        SC_TRY(pass(2, 0, params));
        const double inertia = sums[6];
        if (sums[0] > 0.0) params[1] = sums[1] / sums[0];
        if (sums[3] > 0.0) params[4] = sums[4] / sums[3];
        if (inertia == prev_inertia) break;
        prev_inertia = inertia;
      }
      SC_TRY(pass(2, 0, params));  // responsibilities = the final hard labels
      m_step(2, params);
    }
    double prev = -__builtin_huge_val();
    for (int it = 0; it < 100; ++it) {
      SC_TRY(pass(components, 1, params));  // E-step under params (+ sums of the M-step)
      const double lower_bound = sums[6] / count;
      m_step(components, params);
      if (std::fabs(lower_bound - prev) < 1e-3) break;
      prev = lower_bound;
    }
    SC_TRY(pass(components, 1, params));
    const double n_params = components == 1 ? 2.0 : 5.0;
    *bic = -2.0 * sums[6] + n_params * std::log(count);
    return SC_OK;
  };
  SC_TRY(fit(1, bic1));
  SC_TRY(fit(2, bic2));
  return SC_OK;
}

// NaiveClusterer.predict (naive_clusterer.py:57-105) continuing from the given state:
// centroids (capacity x d, the first *n_centroids rows valid), counts, labels out.
extern "C" int sc_naive_cluster(sc_handle h, const double* x, int n, int d, double threshold,
                                double adaptation_threshold, double* centroids, int32_t* counts,
                                int32_t* n_centroids, int capacity, int64_t* labels) {
  if (!h) return SC_ERR_INVALID;
  if (!x || !centroids || !counts || !n_centroids || !labels || n <= 0 || d <= 0)
    return fail(h, SC_ERR_INVALID, "embeddings must be (n, d)");
  if (*n_centroids < 0 || *n_centroids + n > capacity)
    return fail(h, SC_ERR_INVALID, "centroid capacity must cover n_centroids + n");
  SC_HIP(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  SC_TRY(grow(h, h->fb_x, (size_t)n * d * sizeof(double)));
  SC_TRY(grow(h, h->fb_cent, (size_t)capacity * d * sizeof(double)));
  SC_TRY(grow(h, h->fb_int, ((size_t)capacity + n + 4) * sizeof(int)));
  int* counts_d = ptr<int>(h->fb_int);
  int* k_d = counts_d + capacity;
  int* labels_d = k_d + 4;
  const int k0 = *n_centroids;
  SC_HIP(h, hipMemcpyAsync(h->fb_x.p, x, (size_t)n * d * sizeof(double), hipMemcpyHostToDevice, s));
  if (k0 > 0) {
    SC_HIP(h, hipMemcpyAsync(h->fb_cent.p, centroids, (size_t)k0 * d * sizeof(double),
                             hipMemcpyHostToDevice, s));
    SC_HIP(h, hipMemcpyAsync(counts_d, counts, (size_t)k0 * sizeof(int), hipMemcpyHostToDevice, s));
  }
  SC_HIP(h, hipMemcpyAsync(k_d, n_centroids, sizeof(int), hipMemcpyHostToDevice, s));
  launch_naive_cluster(s, ptr<double>(h->fb_x), n, d, threshold, adaptation_threshold,
                       ptr<double>(h->fb_cent), counts_d, k_d, labels_d);
  SC_TRY(check_last(h, "naive clusterer launch"));
  std::vector<int> lab(n);
  SC_HIP(h, hipMemcpyAsync(lab.data(), labels_d, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
  SC_HIP(h, hipMemcpyAsync(n_centroids, k_d, sizeof(int), hipMemcpyDeviceToHost, s));
  SC_HIP(h, hipStreamSynchronize(s));
  const int k1 = *n_centroids;
  SC_HIP(h, hipMemcpyAsync(centroids, h->fb_cent.p, (size_t)k1 * d * sizeof(double),
                           hipMemcpyDeviceToHost, s));
  SC_HIP(h, hipMemcpyAsync(counts, counts_d, (size_t)k1 * sizeof(int), hipMemcpyDeviceToHost, s));
  SC_HIP(h, hipStreamSynchronize(s));
  for (int i = 0; i < n; ++i) labels[i] = lab[i];
  return SC_OK;
}

