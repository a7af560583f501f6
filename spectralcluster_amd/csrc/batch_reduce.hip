// Size reduction and the too-few-embeddings fallback for a whole batch (include/
// spectralcluster_amd.h sc_batch_ahc, sc_predict_batch_reduced): the host side of many
// agglomerative clusterings of any size per call.  The members are taken longest first in WAVES:
// a wave is the longest remaining members whose buffers fit the wave budget, in ONE allocation
// carved per member, and runs
//   ingest      every member's rows into its X (ingest_rows_into: host or device, any dtype)
//   table       1 copy (the descriptors, AhcBatchItem) + the members' `bad` words cleared
//   distances   k_batch_normalize_rows + ceil(count / 16) grouped fp64 GEMMs (Xn Xn^T)
//               + k_batch_cosine_distance
//   linkage     k_ahc_nn_chain_batch (grid = members, a workgroup each); average-linkage members
//               of up to SC_POOL_LDS_LINKAGE_MAX rows take k_batch_linkage_lds instead (a
//               wavefront each, the distance pass included)
//   back        1 copy (all merge lists + all `bad` words) + 1 synchronisation
//   cut         ahc_tree_cut + the CSR of rows by cluster on the handle's host workers
//   centroids   1 copy (all CSRs) + k_batch_centroids
// whatever the members' sizes are.  A member of n >= kReduceSingleMin rows, or one that alone
// exceeds the budget, runs sc_ahc's own path (callers_api.hip) inside the call.
// The FallbackClusterer single-cluster test of a batch (sc_batch_fallback_check,
// sc_predict_batch_single_fallback) runs the same waves up to the distances, then the verdict
// forms of the linkage kernels: see VerdictMember below.
// The Naive fallback type (sc_batch_naive_cluster, sc_batch_naive_check and the _naive forms of
// the two predict calls) runs the same waves with one launch between ingest and copy back: see
// NaiveMember below.  The two predict calls and their _naive forms share one body each.
// sc_predict_batch_multi_stage (size reduction, fallback and the single-cluster test of
// min_clusters = 1 together) is the first of those bodies with the test in front of its sub-batch:
// see SingleSpec below.
// Kernels: ahc.hip, rowops.hip, naive_batch.hip.
#include "ahc_tree.h"
#include "handle.h"
#include "host_pool.h"

#include <numeric>
#include <thread>

namespace {

constexpr int kReduceSingleMin = 4096;  // from here on a chain has the device to itself anyway
constexpr double kReduceWaveShare = 0.5;  // of the free memory (the pool and the sweep: <= 0.85)

size_t align256(size_t bytes) { return (bytes + 255) / 256 * 256; }

struct ReduceMember {
  int index = 0;  // into the caller's lists
  int n = 0, linkage = 0, n_clusters = 0;
  double threshold = 0.0;
  bool keep_centroids = false;       // centroids stay on the device: dev_cent
  double* host_centroids = nullptr;  // ... or / and go to the caller
  // results
  int k = 0;
  double* dev_cent = nullptr;

  bool centroids() const { return keep_centroids || host_centroids != nullptr; }
  int kcap() const { return n_clusters > 0 ? n_clusters : n; }
  bool lds() const {
    return kPoolLdsLinkageMax > 0 && linkage == SC_LINKAGE_AVERAGE && n <= kPoolLdsLinkageMax;
  }
  size_t csr_ints() const { return centroids() ? (size_t)kcap() + 2 + (size_t)n : 0; }
  // device bytes of the member's own buffers, and with its share of the wave's slabs
  size_t own_bytes(int d) const {
    const size_t rows = align256((size_t)n * round_up(d, 16) * sizeof(double));
    return 2 * rows + align256((size_t)n * matrix_ld(n) * sizeof(double)) +
           2 * align256((size_t)n * sizeof(int)) +
           (centroids() ? align256((size_t)kcap() * d * sizeof(double)) : 0);
  }
  size_t wave_bytes(int d) const {
    return own_bytes(d) + 4 * (size_t)(n - 1) * sizeof(double) + sizeof(int) +
           sizeof(AhcBatchItem) + csr_ints() * sizeof(int);
  }
};

// device allocations of the call: a wave's block, the centroids of a single-path member
struct DeviceBlocks {
  std::vector<void*> blocks;
  void release() {
    for (void* p : blocks) (void)hipFree(p);
    blocks.clear();
  }
  ~DeviceBlocks() { release(); }
};

std::string bad_rows_message(int index) {
  return "utterance " + std::to_string(index) + ": embeddings contain a zero or non-finite row";
}

// the pinned staging of a wave (the stream is idle: every wave ends drained)
int ensure_wave_staging(sc_handle h, size_t staged) {
  if (h->h_reduce_bytes >= staged) return SC_OK;
  if (h->h_reduce) SC_HIP(h, hipHostFree(h->h_reduce));
  h->h_reduce = nullptr;
  h->h_reduce_bytes = 0;
  SC_HIP(h, hipHostMalloc(&h->h_reduce, staged));
  h->h_reduce_bytes = staged;
  return SC_OK;
}

// one member on sc_ahc's path: the handle's arena, its split-K product, its chain launch
int reduce_single(sc_handle h, const sc_array& a, ReduceMember* m, int64_t* labels,
                  DeviceBlocks* blocks) {
  h->sweep_slot.clear();
  SC_TRY(ingest_embeddings(h, a, true));
  const int n = m->n, d = h->d;
  const int rc = ahc_resident(h, m->linkage, m->n_clusters, m->threshold, labels, &m->k);
  if (rc == SC_ERR_INVALID) return fail(h, rc, "utterance " + std::to_string(m->index) + ": " + h->err);
  SC_TRY(rc);
  if (!m->centroids()) return SC_OK;
  hipStream_t s = h->stream;
  const size_t bytes = (size_t)m->k * d * sizeof(double);
  void* out = nullptr;
  SC_HIP(h, hipMalloc(&out, bytes));
  blocks->blocks.push_back(out);
  SC_TRY(grow(h, h->ahc_lab, (size_t)n * sizeof(int)));
  std::vector<int> lab32(n);
  for (int r = 0; r < n; ++r) lab32[r] = (int)labels[r];
  SC_HIP(h, hipMemcpyAsync(h->ahc_lab.p, lab32.data(), (size_t)n * sizeof(int),
                           hipMemcpyHostToDevice, s));
  launch_cluster_centroids(s, ptr<double>(h->X), h->ldx, n, d, ptr<int>(h->ahc_lab), m->k,
                           static_cast<double*>(out));
  SC_TRY(check_last(h, "centroid launch"));
  if (m->host_centroids)
    SC_HIP(h, hipMemcpyAsync(m->host_centroids, out, bytes, hipMemcpyDeviceToHost, s));
  SC_HIP(h, hipStreamSynchronize(s));  // (lab32 is a local)
  m->dev_cent = static_cast<double*>(out);
  return SC_OK;
}

// One wave: `wave` lists its members, those of the chain kernel first, then those of the LDS
// kernel, each part longest first.  The block joins `blocks`; on return the stream has drained.
int reduce_wave(sc_handle h, const sc_array* xs, int d, const std::vector<ReduceMember*>& wave,
                int64_t* const* labels, DeviceBlocks* blocks) {
  const int count = (int)wave.size();
  const int ldx = round_up(d, 16);
  hipStream_t s = h->stream;
  std::vector<size_t> z_at(count), csr_at(count);
  size_t z_doubles = 0, csr_ints = 0, own = 0;
  int n_chain = 0, chain_rows = 0, lds_rows = 0, max_outputs = 0;
  for (int i = 0; i < count; ++i) {
    const ReduceMember& m = *wave[i];
    z_at[i] = z_doubles;
    z_doubles += 4 * (size_t)(m.n - 1);
    csr_at[i] = csr_ints;
    csr_ints += m.csr_ints();
    own += m.own_bytes(d);
    if (m.lds()) {
      lds_rows = std::max(lds_rows, m.n);
    } else {
      n_chain = i + 1;
      chain_rows = std::max(chain_rows, m.n);
    }
    if (m.centroids()) max_outputs = std::max(max_outputs, m.kcap() * d);
  }
  // the slabs every member has a share of: descriptors | merge lists + bad words | CSRs
  const size_t table_bytes = align256((size_t)count * sizeof(AhcBatchItem));
  const size_t back_bytes = align256(z_doubles * sizeof(double) + (size_t)count * sizeof(int));
  const size_t csr_bytes = align256(csr_ints * sizeof(int));
  const size_t staged = table_bytes + back_bytes + csr_bytes;
  SC_TRY(ensure_wave_staging(h, staged));
  void* block = nullptr;
  SC_HIP(h, hipMalloc(&block, staged + own));
  blocks->blocks.push_back(block);
  char* dev = static_cast<char*>(block);
  char* host = static_cast<char*>(h->h_reduce);
  AhcBatchItem* table_d = reinterpret_cast<AhcBatchItem*>(dev);
  AhcBatchItem* table_h = reinterpret_cast<AhcBatchItem*>(host);
  double* Z_d = reinterpret_cast<double*>(dev + table_bytes);
  double* Z_h = reinterpret_cast<double*>(host + table_bytes);
  int* bad_d = reinterpret_cast<int*>(Z_d + z_doubles);
  const int* bad_h = reinterpret_cast<const int*>(Z_h + z_doubles);
  int* csr_d = reinterpret_cast<int*>(dev + table_bytes + back_bytes);
  int* csr_h = reinterpret_cast<int*>(host + table_bytes + back_bytes);
  char* at = dev + staged;
  auto carve = [&](size_t bytes) {
    void* p = at;
    at += align256(bytes);
    return p;
  };
  for (int i = 0; i < count; ++i) {
    const ReduceMember& m = *wave[i];
    AhcBatchItem& it = table_h[i];
    const size_t rows = (size_t)m.n * ldx * sizeof(double);
    it.n = m.n;
    it.ld = matrix_ld(m.n);
    it.ldx = ldx;
    it.d = d;
    it.kcap = m.kcap();
    it.method = m.linkage;
    it.X = static_cast<double*>(carve(rows));
    it.Xn = static_cast<double*>(carve(rows));
    it.D = static_cast<double*>(carve((size_t)m.n * it.ld * sizeof(double)));
    it.size = static_cast<int*>(carve((size_t)m.n * sizeof(int)));
    it.chain = static_cast<int*>(carve((size_t)m.n * sizeof(int)));
    it.Z = Z_d + z_at[i];
    it.bad = bad_d + i;
    it.csr = m.centroids() ? csr_d + csr_at[i] : nullptr;
    it.cent = m.centroids() ? static_cast<double*>(carve((size_t)it.kcap * d * sizeof(double)))
                            : nullptr;
  }
  SC_HIP(h, hipMemcpyAsync(table_d, table_h, (size_t)count * sizeof(AhcBatchItem),
                           hipMemcpyHostToDevice, s));
  SC_HIP(h, hipMemsetAsync(bad_d, 0, (size_t)count * sizeof(int), s));
  bool sync = false;  // (every wave synchronises before it returns)
  for (int i = 0; i < count; ++i)
    SC_TRY(ingest_rows_into(h, xs[wave[i]->index], const_cast<double*>(table_h[i].X), ldx, s,
                            &sync));
  launch_batch_normalize(s, table_d, count, std::max(chain_rows, lds_rows));
  // sc_ahc's unit rows and symmetric product (whole K per tile), 16 members per launch
  for (int base = 0; base < count; base += kGroupMax) {
    GemmGroupItem items[kGroupMax];
    const int cnt = std::min(kGroupMax, count - base);
    for (int z = 0; z < cnt; ++z) {
      const AhcBatchItem& it = table_h[base + z];
      items[z].A = it.Xn;
      items[z].lda = ldx;
      items[z].C = it.D;
      items[z].ldc = it.ld;
      items[z].n = it.n;
      items[z].K = d;
    }
    launch_gemm_nt_group(s, items, cnt, kEpiNone, 0);
  }
  if (n_chain > 0) {
    launch_batch_cosine_distance(s, table_d, 0, n_chain, chain_rows);
    launch_batch_nn_chain(s, table_d, 0, n_chain);
  }
#if SC_POOL_LDS_LINKAGE_MAX > 0
  if (count > n_chain) launch_batch_linkage_lds(s, table_d, n_chain, count - n_chain, lds_rows);
#endif
  SC_TRY(check_last(h, "batched agglomerative clustering launch"));
  SC_HIP(h, hipMemcpyAsync(Z_h, Z_d, z_doubles * sizeof(double) + (size_t)count * sizeof(int),
                           hipMemcpyDeviceToHost, s));
  SC_HIP(h, hipStreamSynchronize(s));
  int bad_index = -1;  // (the first of the batch, whatever the wave's order)
  for (int i = 0; i < count; ++i)
    if (bad_h[i] != 0 && (bad_index < 0 || wave[i]->index < bad_index)) bad_index = wave[i]->index;
  if (bad_index >= 0) return fail(h, SC_ERR_INVALID, bad_rows_message(bad_index));
  // sort, relabel, heap cut and the rows of every cluster: independent per member
  if (!h->gpool) {
    const unsigned hw = std::thread::hardware_concurrency();
    h->gpool = new HostPool(hw >= 64 ? kGroupMax - 1 : (hw >= 8 ? 6 : (hw >= 4 ? 2 : 0)));
  }
  h->gpool->run(count, [&](int i) {
    ReduceMember& m = *wave[i];
    int64_t* lab = labels[m.index];
    m.k = ahc_tree_cut(Z_h + z_at[i], m.n, m.n_clusters, m.threshold, lab);
    if (!m.centroids()) return;
    int* csr = csr_h + csr_at[i];
    int* offset = csr + 1;  // k + 1 of them
    int* rows = csr + m.kcap() + 2;
    csr[0] = m.k;
    std::fill(offset, offset + m.k + 1, 0);
    for (int r = 0; r < m.n; ++r) ++offset[lab[r] + 1];
    for (int c = 0; c < m.k; ++c) offset[c + 1] += offset[c];
    std::vector<int> next(offset, offset + m.k);
    for (int r = 0; r < m.n; ++r) rows[next[lab[r]]++] = r;  // ascending inside a cluster
  });
  if (max_outputs > 0) {
    SC_HIP(h, hipMemcpyAsync(csr_d, csr_h, csr_ints * sizeof(int), hipMemcpyHostToDevice, s));
    launch_batch_centroids(s, table_d, 0, count, max_outputs);
    SC_TRY(check_last(h, "batched centroid launch"));
    for (int i = 0; i < count; ++i) {
      ReduceMember& m = *wave[i];
      if (!m.centroids()) continue;
      m.dev_cent = table_h[i].cent;
      if (m.host_centroids)
        SC_HIP(h, hipMemcpyAsync(m.host_centroids, m.dev_cent, (size_t)m.k * d * sizeof(double),
                                 hipMemcpyDeviceToHost, s));
    }
    SC_HIP(h, hipStreamSynchronize(s));  // (the staging is the next wave's)
  }
  return SC_OK;
}

// Every member of `members` (checked: n >= 2, n_clusters <= n): labels[m.index], m.k and the
// centroids.  `retain`: the device blocks -- and so every dev_cent -- live as long as `blocks`;
// otherwise a wave's block is freed when the wave is done.
int reduce_members(sc_handle h, const sc_array* xs, int d, std::vector<ReduceMember>* members,
                   int64_t* const* labels, DeviceBlocks* blocks, bool retain) {
  std::vector<int> order(members->size());
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return (*members)[a].n > (*members)[b].n; });
  size_t at = 0;
  while (at < order.size()) {
    size_t budget = h->reduce_wave_bytes;
    if (budget == 0) {
      size_t free_bytes = 0, device_bytes = 0;
      SC_HIP(h, hipMemGetInfo(&free_bytes, &device_bytes));
      budget = (size_t)(kReduceWaveShare * (double)free_bytes);
    }
    ReduceMember* first = &(*members)[order[at]];
    if (first->n >= kReduceSingleMin || first->wave_bytes(d) + 3 * 256 > budget) {
      SC_TRY(reduce_single(h, xs[first->index], first, labels[first->index], blocks));
      if (!retain) blocks->release();
      ++at;
      continue;
    }
    std::vector<ReduceMember*> wave;
    size_t bytes = 3 * 256;  // (the slabs' alignment)
    while (at < order.size()) {
      ReduceMember* m = &(*members)[order[at]];
      if (bytes + m->wave_bytes(d) > budget) break;
      bytes += m->wave_bytes(d);
      wave.push_back(m);
      ++at;
    }
    // the members of the LDS kernel behind those of the chain kernel (both stay longest first)
    std::stable_partition(wave.begin(), wave.end(), [](ReduceMember* m) { return !m->lds(); });
    SC_TRY(reduce_wave(h, xs, d, wave, labels, blocks));
    if (!retain) blocks->release();
  }
  return SC_OK;
}

int too_few_rows(sc_handle h, int index, int n) {
  return fail(h, SC_ERR_INVALID,
              "utterance " + std::to_string(index) + ": Found array with " +
                  std::to_string(std::max(n, 0)) +
                  " sample(s) while a minimum of 2 is required by AgglomerativeClustering.");
}

// ---- the FallbackClusterer single-cluster test of a batch (sc_batch_fallback_check,
//      sc_predict_batch_single_fallback): "does average-linkage cosine AHC, cut at the threshold,
//      leave one cluster?" for every member, in waves as above -- ingest, normalise, grouped
//      GEMM, then the VERDICT forms of the two linkage kernels (ahc.hip): no merge list comes
//      back and no tree is cut, a wave downloads its records {height, verdict} and `bad` words in
//      one copy behind one synchronisation.  A wave's widened rows are a block of their own, which
//      may outlive the wave (the grouped batch of the survivors reads them there).
struct VerdictMember {
  int index = 0;  // into the caller's lists
  int name = -1;  // the utterance a message names, when the lists are a sub-batch (< 0: index)
  int n = 0;
  // results
  double height = 0.0;
  int single = 0;
  const double* dev_rows = nullptr;  // the widened rows (pitch round_up(d, 16)) where they stayed

  int named() const { return name < 0 ? index : name; }
  bool lds() const { return kPoolLdsLinkageMax > 0 && n <= kPoolLdsLinkageMax; }
  size_t rows_bytes(int d) const { return align256((size_t)n * round_up(d, 16) * sizeof(double)); }
  // Xn, D and (chain kernel) size + chain
  size_t scratch_bytes(int d) const {
    return rows_bytes(d) + align256((size_t)n * matrix_ld(n) * sizeof(double)) +
           (lds() ? 0 : 2 * align256((size_t)n * sizeof(int)));
  }
  size_t wave_bytes(int d) const {
    return rows_bytes(d) + scratch_bytes(d) + sizeof(AhcBatchItem) + 2 * sizeof(double) +
           sizeof(int);
  }
};

// one member on sc_ahc's path (reduce_single's): the verdict from its merge heights
int verdict_single(sc_handle h, const sc_array& a, VerdictMember* m, double threshold) {
  h->sweep_slot.clear();
  SC_TRY(ingest_embeddings(h, a, true));
  std::vector<int64_t> lab(m->n);
  const int rc = ahc_resident(h, SC_LINKAGE_AVERAGE, 0, threshold, lab.data(), nullptr, &m->height);
  if (rc == SC_ERR_INVALID)
    return fail(h, rc, "utterance " + std::to_string(m->named()) + ": " + h->err);
  SC_TRY(rc);
  m->single = m->height >= threshold ? 0 : 1;
  return SC_OK;
}

// One wave: the members of the chain kernel first, then those of the LDS kernel, each part
// longest first.  `keep` (may be null): the rows' block joins it and every dev_rows is set;
// otherwise it is freed with the wave's other buffers.  On return the stream has drained.
int verdict_wave(sc_handle h, const sc_array* xs, int d, const std::vector<VerdictMember*>& wave,
                 double threshold, DeviceBlocks* keep) {
  const int count = (int)wave.size();
  const int ldx = round_up(d, 16);
  hipStream_t s = h->stream;
  size_t rows_total = 0, scratch_total = 0;
  int n_chain = 0, chain_rows = 0, lds_rows = 0;
  for (int i = 0; i < count; ++i) {
    const VerdictMember& m = *wave[i];
    rows_total += m.rows_bytes(d);
    scratch_total += m.scratch_bytes(d);
    if (m.lds()) {
      lds_rows = std::max(lds_rows, m.n);
    } else {
      n_chain = i + 1;
      chain_rows = std::max(chain_rows, m.n);
    }
  }
  // descriptors | records + bad words
  const size_t table_bytes = align256((size_t)count * sizeof(AhcBatchItem));
  const size_t back_doubles = 2 * (size_t)count;
  const size_t back_bytes = align256(back_doubles * sizeof(double) + (size_t)count * sizeof(int));
  const size_t staged = table_bytes + back_bytes;
  SC_TRY(ensure_wave_staging(h, staged));
  DeviceBlocks scratch;  // freed when the wave returns
  void* rows_block = nullptr;
  SC_HIP(h, hipMalloc(&rows_block, rows_total));
  (keep ? keep : &scratch)->blocks.push_back(rows_block);
  void* block = nullptr;
  SC_HIP(h, hipMalloc(&block, staged + scratch_total));
  scratch.blocks.push_back(block);
  char* dev = static_cast<char*>(block);
  char* host = static_cast<char*>(h->h_reduce);
  AhcBatchItem* table_d = reinterpret_cast<AhcBatchItem*>(dev);
  AhcBatchItem* table_h = reinterpret_cast<AhcBatchItem*>(host);
  double* rec_d = reinterpret_cast<double*>(dev + table_bytes);
  const double* rec_h = reinterpret_cast<const double*>(host + table_bytes);
  int* bad_d = reinterpret_cast<int*>(rec_d + back_doubles);
  const int* bad_h = reinterpret_cast<const int*>(rec_h + back_doubles);
  char* at = dev + staged;
  char* rows_at = static_cast<char*>(rows_block);
  auto carve = [](char*& from, size_t bytes) {
    void* p = from;
    from += align256(bytes);
    return p;
  };
  for (int i = 0; i < count; ++i) {
    const VerdictMember& m = *wave[i];
    AhcBatchItem& it = table_h[i];
    const size_t rows = (size_t)m.n * ldx * sizeof(double);
    memset(&it, 0, sizeof(it));
    it.n = m.n;
    it.ld = matrix_ld(m.n);
    it.ldx = ldx;
    it.d = d;
    it.kcap = m.n;
    it.method = SC_LINKAGE_AVERAGE;
    it.X = static_cast<double*>(carve(rows_at, rows));
    it.Xn = static_cast<double*>(carve(at, rows));
    it.D = static_cast<double*>(carve(at, (size_t)m.n * it.ld * sizeof(double)));
    if (!m.lds()) {  // (the LDS kernel keeps both in LDS)
      it.size = static_cast<int*>(carve(at, (size_t)m.n * sizeof(int)));
      it.chain = static_cast<int*>(carve(at, (size_t)m.n * sizeof(int)));
    }
    it.Z = rec_d + 2 * (size_t)i;  // the record {height, verdict}
    it.bad = bad_d + i;
  }
  SC_HIP(h, hipMemcpyAsync(table_d, table_h, (size_t)count * sizeof(AhcBatchItem),
                           hipMemcpyHostToDevice, s));
  SC_HIP(h, hipMemsetAsync(rec_d, 0, back_doubles * sizeof(double) + (size_t)count * sizeof(int),
                           s));
  bool sync = false;  // (the wave synchronises before it returns)
  for (int i = 0; i < count; ++i)
    SC_TRY(ingest_rows_into(h, xs[wave[i]->index], const_cast<double*>(table_h[i].X), ldx, s,
                            &sync));
  launch_batch_normalize(s, table_d, count, std::max(chain_rows, lds_rows));
  // sc_batch_ahc's unit rows and symmetric product (whole K per tile), 16 members per launch
  for (int base = 0; base < count; base += kGroupMax) {
    GemmGroupItem items[kGroupMax];
    const int cnt = std::min(kGroupMax, count - base);
    for (int z = 0; z < cnt; ++z) {
      const AhcBatchItem& it = table_h[base + z];
      items[z].A = it.Xn;
      items[z].lda = ldx;
      items[z].C = it.D;
      items[z].ldc = it.ld;
      items[z].n = it.n;
      items[z].K = d;
    }
    launch_gemm_nt_group(s, items, cnt, kEpiNone, 0);
  }
  if (n_chain > 0) {
    launch_batch_cosine_distance(s, table_d, 0, n_chain, chain_rows);
    launch_batch_nn_chain_verdict(s, table_d, 0, n_chain, threshold);
  }
#if SC_POOL_LDS_LINKAGE_MAX > 0
  if (count > n_chain)
    launch_batch_linkage_lds_verdict(s, table_d, n_chain, count - n_chain, lds_rows, threshold);
#endif
  SC_TRY(check_last(h, "batched single-cluster verdict launch"));
  SC_HIP(h, hipMemcpyAsync(const_cast<double*>(rec_h), rec_d,
                           back_doubles * sizeof(double) + (size_t)count * sizeof(int),
                           hipMemcpyDeviceToHost, s));
  SC_HIP(h, hipStreamSynchronize(s));
  int bad_index = -1;  // (the first of the batch, whatever the wave's order)
  for (int i = 0; i < count; ++i)
    if (bad_h[i] != 0 && (bad_index < 0 || wave[i]->named() < bad_index))
      bad_index = wave[i]->named();
  if (bad_index >= 0) return fail(h, SC_ERR_INVALID, bad_rows_message(bad_index));
  for (int i = 0; i < count; ++i) {
    VerdictMember& m = *wave[i];
    m.height = rec_h[2 * (size_t)i];
    m.single = rec_h[2 * (size_t)i + 1] != 0.0;
    m.dev_rows = keep ? table_h[i].X : nullptr;
  }
  return SC_OK;
}

// Every member of `members` (checked: n >= 2): height and single.  `keep` (may be null): the
// rows' blocks of the waves stay there, and every dev_rows with them, while they add up to at
// most half a wave's budget; a member whose rows did not stay has dev_rows == nullptr.
int fallback_verdicts(sc_handle h, const sc_array* xs, int d, std::vector<VerdictMember>* members,
                      double threshold, DeviceBlocks* keep) {
  std::vector<int> order(members->size());
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return (*members)[a].n > (*members)[b].n; });
  size_t at = 0, kept = 0;
  while (at < order.size()) {
    size_t budget = h->reduce_wave_bytes;
    if (budget == 0) {
      size_t free_bytes = 0, device_bytes = 0;
      SC_HIP(h, hipMemGetInfo(&free_bytes, &device_bytes));
      budget = (size_t)(kReduceWaveShare * (double)free_bytes);
    }
    VerdictMember* first = &(*members)[order[at]];
    if (first->n >= kReduceSingleMin || first->wave_bytes(d) + 2 * 256 > budget) {
      SC_TRY(verdict_single(h, xs[first->index], first, threshold));
      ++at;
      continue;
    }
    std::vector<VerdictMember*> wave;
    size_t bytes = 2 * 256, rows = 0;  // (the slabs' alignment)
    while (at < order.size()) {
      VerdictMember* m = &(*members)[order[at]];
      if (bytes + m->wave_bytes(d) > budget) break;
      bytes += m->wave_bytes(d);
      rows += m->rows_bytes(d);
      wave.push_back(m);
      ++at;
    }
    // the members of the LDS kernel behind those of the chain kernel (both stay longest first)
    std::stable_partition(wave.begin(), wave.end(), [](VerdictMember* m) { return !m->lds(); });
    const bool stay = keep && kept + rows <= budget / 2;
    SC_TRY(verdict_wave(h, xs, d, wave, threshold, stay ? keep : nullptr));
    if (stay) kept += rows;
  }
  return SC_OK;
}

// what both entry points check of every utterance before the first launch
int verdict_members(sc_handle h, const std::vector<int>& ns, std::vector<VerdictMember>* members) {
  members->resize(ns.size());
  for (size_t i = 0; i < ns.size(); ++i) {
    if (ns[i] < 2) return too_few_rows(h, (int)i, ns[i]);
    (*members)[i].index = (int)i;
    (*members)[i].n = ns[i];
  }
  return SC_OK;
}

// ---- the naive fallback clusterer of a batch (sc_batch_naive_cluster, sc_batch_naive_check and
//      the _naive forms of the two predict calls): NaiveClusterer.predict from the empty state for
//      every member, in waves as above, with nothing between the ingest and the walk -- one
//      allocation pair, one ingest per member, one table copy, ONE launch (k_naive_cluster_batch,
//      a workgroup per member), one copy back, one synchronisation.  There is no single path: a
//      member that alone exceeds the budget is a wave of its own.
//      labels form   back: [centroids n x d of the members that want them] [labels n | counts n |
//                    n_clusters per member]; the other members' centroids are scratch
//      verdict form  back: {single, stopped_at, bad} per member; scratch: one centroid each.  The
//                    rows are a block of their own, which may outlive the wave (VerdictMember).
struct NaiveMember {
  int index = 0;  // into the caller's lists
  int name = -1;  // the utterance a message names, when the lists are a sub-batch (< 0: index)
  int n = 0;
  bool want_centroids = false;  // labels form: the centroids come back
  // results
  std::vector<int> ints;     // labels form: labels n | counts n | n_clusters
  std::vector<double> cent;  // labels form, wanted: n_clusters x d
  int single = 0, stopped_at = 0;    // verdict form
  const double* dev_rows = nullptr;  // the widened rows (pitch round_up(d, 16)) where they stayed

  int named() const { return name < 0 ? index : name; }
  int k() const { return ints[2 * (size_t)n]; }
  size_t rows_bytes(int d) const { return align256((size_t)n * round_up(d, 16) * sizeof(double)); }
  size_t cent_bytes(int d, bool verdict) const {
    return align256((size_t)(verdict ? 1 : n) * d * sizeof(double));
  }
  size_t back_ints(bool verdict) const { return verdict ? 3 : 2 * (size_t)n + 1; }
  size_t wave_bytes(int d, bool verdict) const {
    return rows_bytes(d) + cent_bytes(d, verdict) + back_ints(verdict) * sizeof(int) +
           sizeof(NaiveBatchItem);
  }
};

struct NaiveRun {
  double threshold = 0.0, adaptation = 0.0;
  bool verdict = false;
  bool check_rows = false;  // verdict form: a zero or non-finite row fails the call
};

// One wave.  `keep` (may be null): the rows' block joins it and every dev_rows is set; otherwise
// it is freed with the wave's other buffers.  On return the stream has drained.
int naive_wave(sc_handle h, const sc_array* xs, int d, const std::vector<NaiveMember*>& wave,
               const NaiveRun& run, DeviceBlocks* keep) {
  const int count = (int)wave.size();
  const int ldx = round_up(d, 16);
  hipStream_t s = h->stream;
  size_t rows_total = 0, back_cent = 0, back_ints = 0, scratch_total = 0;
  for (const NaiveMember* m : wave) {
    rows_total += m->rows_bytes(d);
    back_ints += m->back_ints(run.verdict);
    (m->want_centroids ? back_cent : scratch_total) += m->cent_bytes(d, run.verdict);
  }
  // descriptors | centroids that travel back + the members' ints
  const size_t table_bytes = align256((size_t)count * sizeof(NaiveBatchItem));
  const size_t back_bytes = back_cent + align256(back_ints * sizeof(int));
  const size_t staged = table_bytes + back_bytes;
  SC_TRY(ensure_wave_staging(h, staged));
  DeviceBlocks scratch;  // freed when the wave returns
  void* rows_block = nullptr;
  SC_HIP(h, hipMalloc(&rows_block, rows_total));
  (keep ? keep : &scratch)->blocks.push_back(rows_block);
  void* block = nullptr;
  SC_HIP(h, hipMalloc(&block, staged + scratch_total));
  scratch.blocks.push_back(block);
  char* dev = static_cast<char*>(block);
  char* host = static_cast<char*>(h->h_reduce);
  NaiveBatchItem* table_d = reinterpret_cast<NaiveBatchItem*>(dev);
  NaiveBatchItem* table_h = reinterpret_cast<NaiveBatchItem*>(host);
  char* back_d = dev + table_bytes;
  const char* back_h = host + table_bytes;
  int* ints_d = reinterpret_cast<int*>(back_d + back_cent);
  const int* ints_h = reinterpret_cast<const int*>(back_h + back_cent);
  char* cent_at = back_d;
  char* scratch_at = dev + staged;
  char* rows_at = static_cast<char*>(rows_block);
  auto carve = [](char*& from, size_t bytes) {
    void* p = from;
    from += bytes;  // (a multiple of 256)
    return p;
  };
  std::vector<size_t> ints_of(count), cent_of(count);  // offsets into the back slab
  size_t ints_used = 0;
  for (int i = 0; i < count; ++i) {
    const NaiveMember& m = *wave[i];
    NaiveBatchItem& it = table_h[i];
    memset(&it, 0, sizeof(it));
    it.n = m.n;
    it.ldx = ldx;
    it.d = d;
    it.X = static_cast<double*>(carve(rows_at, m.rows_bytes(d)));
    cent_of[i] = (size_t)(cent_at - back_d);
    it.cent = static_cast<double*>(
        carve(m.want_centroids ? cent_at : scratch_at, m.cent_bytes(d, run.verdict)));
    ints_of[i] = ints_used;
    int* mine = ints_d + ints_used;
    ints_used += m.back_ints(run.verdict);
    if (run.verdict) {
      it.out = mine;
      it.bad = run.check_rows ? mine + 2 : nullptr;
    } else {
      it.labels = mine;
      it.counts = mine + m.n;
      it.out = mine + 2 * (size_t)m.n;
    }
  }
  SC_HIP(h, hipMemcpyAsync(table_d, table_h, (size_t)count * sizeof(NaiveBatchItem),
                           hipMemcpyHostToDevice, s));
  if (run.verdict) SC_HIP(h, hipMemsetAsync(ints_d, 0, back_ints * sizeof(int), s));
  bool sync = false;  // (the wave synchronises before it returns)
  for (int i = 0; i < count; ++i)
    SC_TRY(ingest_rows_into(h, xs[wave[i]->index], const_cast<double*>(table_h[i].X), ldx, s,
                            &sync));
  launch_naive_cluster_batch(s, table_d, count, run.threshold, run.adaptation, run.verdict);
  SC_TRY(check_last(h, "batched naive clusterer launch"));
  SC_HIP(h, hipMemcpyAsync(const_cast<char*>(back_h), back_d,
                           back_cent + back_ints * sizeof(int), hipMemcpyDeviceToHost, s));
  SC_HIP(h, hipStreamSynchronize(s));
  if (run.verdict) {
    int bad_index = -1;  // (the first of the batch, whatever the wave's order)
    for (int i = 0; i < count; ++i)
      if (ints_h[ints_of[i] + 2] != 0 && (bad_index < 0 || wave[i]->named() < bad_index))
        bad_index = wave[i]->named();
    if (bad_index >= 0) return fail(h, SC_ERR_INVALID, bad_rows_message(bad_index));
  }
  for (int i = 0; i < count; ++i) {
    NaiveMember& m = *wave[i];
    const int* mine = ints_h + ints_of[i];
    m.dev_rows = keep ? table_h[i].X : nullptr;
    if (run.verdict) {
      m.single = mine[0];
      m.stopped_at = mine[1];
      continue;
    }
    m.ints.assign(mine, mine + m.back_ints(false));
    if (m.want_centroids) {
      const double* c = reinterpret_cast<const double*>(back_h + cent_of[i]);
      m.cent.assign(c, c + (size_t)m.k() * d);
    }
  }
  return SC_OK;
}

// Every member of `members` (checked: n >= 1).  `keep` (may be null): as fallback_verdicts', the
// rows' blocks of the waves stay there while they add up to at most half a wave's budget.
int naive_members(sc_handle h, const sc_array* xs, int d, std::vector<NaiveMember>* members,
                  const NaiveRun& run, DeviceBlocks* keep) {
  std::vector<int> order(members->size());
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return (*members)[a].n > (*members)[b].n; });
  size_t at = 0, kept = 0;
  while (at < order.size()) {
    size_t budget = h->reduce_wave_bytes;
    if (budget == 0) {
      size_t free_bytes = 0, device_bytes = 0;
      SC_HIP(h, hipMemGetInfo(&free_bytes, &device_bytes));
      budget = (size_t)(kReduceWaveShare * (double)free_bytes);
    }
    std::vector<NaiveMember*> wave;
    size_t bytes = 2 * 256, rows = 0;  // (the slabs' alignment)
    while (at < order.size()) {
      NaiveMember* m = &(*members)[order[at]];
      // (the longest remaining member always goes: alone when it exceeds the budget)
      if (!wave.empty() && bytes + m->wave_bytes(d, run.verdict) > budget) break;
      bytes += m->wave_bytes(d, run.verdict);
      rows += m->rows_bytes(d);
      wave.push_back(m);
      ++at;
    }
    const bool stay = keep && kept + rows <= budget / 2;
    SC_TRY(naive_wave(h, xs, d, wave, run, stay ? keep : nullptr));
    if (stay) kept += rows;
  }
  return SC_OK;
}

// NaiveClusterer.__init__'s check (naive_clusterer.py:36-37)
int validate_naive_thresholds(sc_handle h, double threshold, double adaptation) {
  if (adaptation < threshold)
    return fail(h, SC_ERR_INVALID, "adaptation_threshold cannot be smaller than threshold");
  return SC_OK;
}

// what clusters the fallback utterances (kind 2) of sc_predict_batch_reduced[_naive]
struct FallbackSpec {
  bool naive = false;
  double threshold = 0.0;   // agglomerative: the distance threshold; naive: the similarity one
  double adaptation = 0.0;  // naive only
};

// The single-cluster test of min_clusters = 1 that sc_predict_batch_multi_stage puts in front of
// the spectral run of the sub-batch (the rows of kind 0, the centroids of kind 1)
struct SingleSpec {
  int condition = 0;         // 0 none; 1-4 `check` (the affinity); 5 the fallback clusterer's verdict
  sc_single_check check{};
  int32_t* single = nullptr;  // per utterance 1 / 0, -1 for kind 2 (not tested); may be null
};

// The verdicts of the FallbackClusterer condition for a whole batch, then ONE grouped batch of the
// survivors (defined below, with the two entry points that are nothing else).  `names` (may be
// null): the utterance a message names for xs[z], when xs is a sub-batch.
int predict_batch_fallback_condition(sc_handle h, const sc_array* xs, int count,
                                     const sc_config* cfg, const FallbackSpec& fallback,
                                     const std::vector<int>& ns, int d, int64_t* const* labels,
                                     sc_diag* diags, int group, int32_t* single,
                                     const int* names);

// The body of sc_predict_batch_reduced, sc_predict_batch_reduced_naive (test == nullptr) and
// sc_predict_batch_multi_stage (their arguments are checked by predict_batch_reduced_entry below;
// what is checked per member is checked here, before the first launch).
int predict_batch_reduced_body(sc_handle h, const sc_array* xs, int count, const sc_config* cfg,
                               int max_spectral_size, int spectral_min_embeddings,
                               const FallbackSpec& fallback, const SingleSpec* test,
                               int64_t* const* labels, sc_diag* diags, int group, int32_t* kinds,
                               const std::vector<int>& ns, int d) {
  const int condition = test ? test->condition : 0;
  std::vector<int32_t> kind(count, 0);
  std::vector<ReduceMember> members;
  std::vector<NaiveMember> naive;
  std::vector<std::vector<int64_t>> pre(count);  // kind 1: the rows' pre-cluster labels
  std::vector<int64_t*> ahc_labels(count, nullptr);
  for (int i = 0; i < count; ++i) {
    ReduceMember m;
    m.index = i;
    m.n = ns[i];
    if (ns[i] >= spectral_min_embeddings && condition != 0) {
      // what is tested: the utterance, or the max_spectral_size centroids of kind 1
      const int rows = max_spectral_size > 0 && ns[i] > max_spectral_size ? max_spectral_size
                                                                           : ns[i];
      if (condition <= SC_SINGLE_AFFINITY_STD)
        SC_TRY(check_single_offset(h, &test->check, rows, i));
      else if (!fallback.naive && rows < 2)
        return too_few_rows(h, i, rows);
    }
    if (ns[i] < spectral_min_embeddings) {
      kind[i] = 2;
      if (fallback.naive) {  // (a single row is fine: label 0)
        NaiveMember nm;
        nm.index = i;
        nm.n = ns[i];
        naive.push_back(nm);
        continue;
      }
      if (ns[i] < 2) return too_few_rows(h, i, ns[i]);
      m.linkage = SC_LINKAGE_AVERAGE;
      m.threshold = fallback.threshold;
      ahc_labels[i] = labels[i];
    } else if (max_spectral_size > 0 && ns[i] > max_spectral_size) {
      kind[i] = 1;
      m.linkage = SC_LINKAGE_COMPLETE;
      m.n_clusters = max_spectral_size;
      m.keep_centroids = true;
      pre[i].resize(ns[i]);
      ahc_labels[i] = pre[i].data();
    } else {
      continue;
    }
    members.push_back(m);
  }
  if (kinds) std::copy(kind.begin(), kind.end(), kinds);
  DeviceBlocks blocks;  // the centroids live in them until the spectral batch has returned
  SC_TRY(reduce_members(h, xs, d, &members, ahc_labels.data(), &blocks, true));
  if (!naive.empty()) {
    NaiveRun run;
    run.threshold = fallback.threshold;
    run.adaptation = fallback.adaptation;
    SC_TRY(naive_members(h, xs, d, &naive, run, nullptr));
    for (const NaiveMember& m : naive)
      std::copy(m.ints.begin(), m.ints.begin() + m.n, labels[m.index]);
  }
  // ONE grouped batch: the rows of kind 0, the centroids of kind 1
  std::vector<int> at;  // position in that batch -> utterance
  std::vector<sc_array> sub;
  std::vector<int> sub_ns;
  std::vector<std::vector<int64_t>> main_labels(count);
  std::vector<int64_t*> sub_labels;
  for (int i = 0; i < count; ++i)
    if (kind[i] == 0) {
      at.push_back(i);
      sub.push_back(xs[i]);
      sub_ns.push_back(ns[i]);
      sub_labels.push_back(labels[i]);
    }
  for (const ReduceMember& m : members) {
    if (kind[m.index] != 1) continue;
    sc_array c;
    c.data = m.dev_cent;
    c.dtype = SC_DTYPE_F64;
    c.location = SC_MEM_DEVICE;
    c.rows = m.k;
    c.cols = d;
    c.row_stride = d;
    c.col_stride = 1;
    main_labels[m.index].resize(m.k);
    at.push_back(m.index);
    sub.push_back(c);
    sub_ns.push_back(m.k);
    sub_labels.push_back(main_labels[m.index].data());
  }
  const int sub_count = (int)at.size();
  std::vector<sc_diag> sub_diags(diags ? sub_count : 0);
  std::vector<int32_t> routes(count, SC_BATCH_ROUTE_FALLBACK);
  std::vector<int32_t> sub_single(sub_count, 0);
  if (sub_count > 0) {
    // the centroids are written, and what the caller ordered before this handle's stream is
    // done, before a verdict wave or the streams of the batch read either
    SC_HIP(h, hipStreamSynchronize(h->stream));
    sc_diag* sub_dg = diags ? sub_diags.data() : nullptr;
    if (condition == 0)
      SC_TRY(predict_batch_grouped_impl(h, sub.data(), sub_ns.data(), d, sub_count, cfg,
                                        sub_labels.data(), sub_dg, group));
    else if (condition <= SC_SINGLE_AFFINITY_STD)
      SC_TRY(predict_batch_single_impl(h, sub.data(), sub_ns.data(), d, sub_count, cfg,
                                       &test->check, sub_labels.data(), sub_dg, group,
                                       sub_single.data()));
    else
      SC_TRY(predict_batch_fallback_condition(h, sub.data(), sub_count, cfg, fallback, sub_ns, d,
                                              sub_labels.data(), sub_dg, group,
                                              sub_single.data(), at.data()));
    for (int z = 0; z < sub_count; ++z) routes[at[z]] = h->last_routes[z];
  }
  h->last_routes = routes;
  if (test && test->single) {
    std::fill(test->single, test->single + count, -1);  // kind 2: not tested
    for (int z = 0; z < sub_count; ++z) test->single[at[z]] = sub_single[z];
  }
  for (int z = 0; z < sub_count; ++z) {
    const int i = at[z];
    if (diags) diags[i] = sub_diags[z];
    if (kind[i] != 1) continue;
    for (int r = 0; r < ns[i]; ++r) labels[i][r] = main_labels[i][pre[i][r]];
  }
  if (diags)
    for (int i = 0; i < count; ++i)
      if (kind[i] == 2) memset(&diags[i], 0, sizeof(sc_diag));
  return SC_OK;
}

// the checks of both forms, then the body
int predict_batch_reduced_entry(sc_handle h, const char* name, const sc_array* xs, int count,
                                const sc_config* cfg, int max_spectral_size,
                                int spectral_min_embeddings, const FallbackSpec& fallback,
                                int64_t* const* labels, sc_diag* diags, int group,
                                int32_t* kinds, const SingleSpec* test = nullptr) {
  if (!xs || !labels || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  if (group < 2)
    return fail(h, SC_ERR_INVALID, std::string(name) + " is the grouped form: group >= 2");
  if (max_spectral_size < 0 || max_spectral_size == 1)
    return fail(h, SC_ERR_INVALID, "max_spectral_size should be a relatively big number");
  // (the spectral run of the centroids must not be a fallback member itself)
  if (max_spectral_size > 0 && max_spectral_size < spectral_min_embeddings)
    return fail(h, SC_ERR_INVALID,
                "max_spectral_size must not be below spectral_min_embeddings in a batch");
  if (fallback.naive) SC_TRY(validate_naive_thresholds(h, fallback.threshold, fallback.adaptation));
  if (test && test->condition >= SC_SINGLE_GMM_BIC && test->condition <= SC_SINGLE_AFFINITY_STD)
    SC_TRY(validate_single_check(h, &test->check));
  SC_TRY(validate_config(h, cfg));
  SC_HIP(h, hipSetDevice(h->device));
  bool device_source = false;
  std::vector<int> ns;
  int d = 0;
  SC_TRY(validate_batch_arrays(h, xs, count, &ns, &d, &device_source, labels));
  SC_TRY(sc_clear_constraint(h));  // a batch carries none
  if (count == 0) {
    h->last_routes.clear();
    return SC_OK;
  }
  return predict_batch_reduced_body(h, xs, count, cfg, max_spectral_size, spectral_min_embeddings,
                                    fallback, test, labels, diags, group, kinds, ns, d);
}

// One verdict of the FallbackClusterer condition per utterance, whichever clusterer gave it
struct SingleVerdict {
  int single = 0;
  const double* dev_rows = nullptr;  // the widened rows where a wave left them, or nullptr
};

// The second half of sc_predict_batch_single_fallback and sc_predict_batch_single_naive: zeros
// for the single utterances, ONE grouped batch over the others.
int predict_batch_single_rest(sc_handle h, const sc_array* xs, int count, const sc_config* cfg,
                              const std::vector<SingleVerdict>& verdicts,
                              const std::vector<int>& ns, int d, int64_t* const* labels,
                              sc_diag* diags, int group, int32_t* single) {
  std::vector<int> at;  // position in that batch -> utterance
  std::vector<sc_array> sub;
  std::vector<int> sub_ns;
  std::vector<int64_t*> sub_labels;
  for (int i = 0; i < count; ++i) {
    const SingleVerdict& v = verdicts[i];
    if (single) single[i] = v.single;
    if (v.single) {  // predict(): np.array([0] * n), before the affinity is built
      std::fill(labels[i], labels[i] + ns[i], (int64_t)0);
      continue;
    }
    sc_array a = xs[i];
    if (v.dev_rows) {  // the widened rows (exact: the labels are those of the caller's array)
      a.data = v.dev_rows;
      a.dtype = SC_DTYPE_F64;
      a.location = SC_MEM_DEVICE;
      a.row_stride = round_up(d, 16);
      a.col_stride = 1;
    }
    at.push_back(i);
    sub.push_back(a);
    sub_ns.push_back(ns[i]);
    sub_labels.push_back(labels[i]);
  }
  const int sub_count = (int)at.size();
  std::vector<sc_diag> sub_diags(diags ? sub_count : 0);
  std::vector<int32_t> routes(count, SC_BATCH_ROUTE_FALLBACK);
  if (sub_count > 0) {
    // (every wave ended drained; what the caller ordered before this handle's stream is done
    //  before the streams of the batch read a device source)
    SC_HIP(h, hipStreamSynchronize(h->stream));
    SC_TRY(predict_batch_grouped_impl(h, sub.data(), sub_ns.data(), d, sub_count, cfg,
                                      sub_labels.data(), diags ? sub_diags.data() : nullptr,
                                      group));
    for (int z = 0; z < sub_count; ++z) routes[at[z]] = h->last_routes[z];
  }
  h->last_routes = routes;
  if (diags) {
    for (int i = 0; i < count; ++i) memset(&diags[i], 0, sizeof(sc_diag));
    for (int z = 0; z < sub_count; ++z) diags[at[z]] = sub_diags[z];
  }
  return SC_OK;
}

int predict_batch_fallback_condition(sc_handle h, const sc_array* xs, int count,
                                     const sc_config* cfg, const FallbackSpec& fallback,
                                     const std::vector<int>& ns, int d, int64_t* const* labels,
                                     sc_diag* diags, int group, int32_t* single,
                                     const int* names) {
  // the verdicts of the whole batch first (waves of hundreds of workgroups, not one lockstep
  // group at a time); the rows of the waves stay on the device for the survivors
  DeviceBlocks rows;
  std::vector<SingleVerdict> verdicts(count);
  if (fallback.naive) {
    std::vector<NaiveMember> members(count);
    for (int i = 0; i < count; ++i) {  // (an utterance of one row is single)
      members[i].index = i;
      members[i].name = names ? names[i] : -1;
      members[i].n = ns[i];
    }
    NaiveRun run;
    run.threshold = fallback.threshold;
    run.adaptation = fallback.adaptation;
    run.verdict = true;
    run.check_rows = true;  // predict() builds the affinity of such an utterance and raises
    SC_TRY(naive_members(h, xs, d, &members, run, &rows));
    for (const NaiveMember& m : members) {
      verdicts[m.index].single = m.single;
      verdicts[m.index].dev_rows = m.dev_rows;
    }
  } else {
    std::vector<VerdictMember> members;
    SC_TRY(verdict_members(h, ns, &members));  // (the callers have checked n >= 2)
    for (int i = 0; names && i < count; ++i) members[i].name = names[i];
    SC_TRY(fallback_verdicts(h, xs, d, &members, fallback.threshold, &rows));
    for (const VerdictMember& m : members) {
      verdicts[m.index].single = m.single;
      verdicts[m.index].dev_rows = m.dev_rows;
    }
  }
  return predict_batch_single_rest(h, xs, count, cfg, verdicts, ns, d, labels, diags, group,
                                   single);
}

}  // namespace

extern "C" int sc_set_reduce_wave_bytes(sc_handle h, size_t bytes) {
  if (!h) return SC_ERR_INVALID;
  h->reduce_wave_bytes = bytes;
  return SC_OK;
}

extern "C" int sc_batch_ahc(sc_handle h, const sc_array* xs, int count, int linkage,
                            int n_clusters, double distance_threshold, int64_t* const* labels,
                            double* const* centroids) {
  if (!h) return SC_ERR_INVALID;
  if (!xs || !labels || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  if (linkage != SC_LINKAGE_COMPLETE && linkage != SC_LINKAGE_AVERAGE)
    return fail(h, SC_ERR_INVALID, "linkage must be complete or average");
  SC_HIP(h, hipSetDevice(h->device));
  bool device_source = false;
  std::vector<int> ns;
  int d = 0;
  SC_TRY(validate_batch_arrays(h, xs, count, &ns, &d, &device_source, labels));
  std::vector<ReduceMember> members(count);
  for (int i = 0; i < count; ++i) {
    if (ns[i] < 2) return too_few_rows(h, i, ns[i]);
    if (n_clusters < 0 || n_clusters > ns[i])
      return fail(h, SC_ERR_INVALID, "utterance " + std::to_string(i) +
                                         ": Cannot extract more clusters than samples");
    ReduceMember& m = members[i];
    m.index = i;
    m.n = ns[i];
    m.linkage = linkage;
    m.n_clusters = n_clusters;
    m.threshold = distance_threshold;
    m.host_centroids = centroids ? centroids[i] : nullptr;
  }
  DeviceBlocks blocks;
  return reduce_members(h, xs, d, &members, labels, &blocks, false);
}

extern "C" int sc_predict_batch_reduced(sc_handle h, const sc_array* xs, int count,
                                        const sc_config* cfg, int max_spectral_size,
                                        int spectral_min_embeddings,
                                        double agglomerative_threshold, int64_t* const* labels,
                                        sc_diag* diags, int group, int32_t* kinds) {
  if (!h) return SC_ERR_INVALID;
  FallbackSpec fallback;
  fallback.threshold = agglomerative_threshold;
  return predict_batch_reduced_entry(h, "sc_predict_batch_reduced", xs, count, cfg,
                                     max_spectral_size, spectral_min_embeddings, fallback, labels,
                                     diags, group, kinds);
}

extern "C" int sc_predict_batch_reduced_naive(sc_handle h, const sc_array* xs, int count,
                                              const sc_config* cfg, int max_spectral_size,
                                              int spectral_min_embeddings, double naive_threshold,
                                              double naive_adaptation_threshold,
                                              int64_t* const* labels, sc_diag* diags, int group,
                                              int32_t* kinds) {
  if (!h) return SC_ERR_INVALID;
  FallbackSpec fallback;
  fallback.naive = true;
  fallback.threshold = naive_threshold;
  fallback.adaptation = naive_adaptation_threshold;
  return predict_batch_reduced_entry(h, "sc_predict_batch_reduced_naive", xs, count, cfg,
                                     max_spectral_size, spectral_min_embeddings, fallback, labels,
                                     diags, group, kinds);
}

extern "C" int sc_multi_stage_layout(int* bytes, int* field_offsets) {
  if (bytes) *bytes = (int)sizeof(sc_multi_stage);
  if (field_offsets) {
    field_offsets[0] = (int)offsetof(sc_multi_stage, max_spectral_size);
    field_offsets[1] = (int)offsetof(sc_multi_stage, spectral_min_embeddings);
    field_offsets[2] = (int)offsetof(sc_multi_stage, fallback_type);
    field_offsets[3] = (int)offsetof(sc_multi_stage, agglomerative_threshold);
    field_offsets[4] = (int)offsetof(sc_multi_stage, naive_threshold);
    field_offsets[5] = (int)offsetof(sc_multi_stage, naive_adaptation_threshold);
    field_offsets[6] = (int)offsetof(sc_multi_stage, single_condition);
    field_offsets[7] = (int)offsetof(sc_multi_stage, single_threshold);
    field_offsets[8] = (int)offsetof(sc_multi_stage, diagonal_offset);
  }
  return SC_OK;
}

extern "C" int sc_predict_batch_multi_stage(sc_handle h, const sc_array* xs, int count,
                                            const sc_config* cfg, const sc_multi_stage* stage,
                                            int64_t* const* labels, sc_diag* diags, int group,
                                            int32_t* kinds, int32_t* single) {
  if (!h) return SC_ERR_INVALID;
  if (!stage) return fail(h, SC_ERR_INVALID, "NULL argument");
  constexpr int kAgglomerative = 1, kNaive = 2;  // FallbackClustererType's values
  if (stage->fallback_type != kAgglomerative && stage->fallback_type != kNaive)
    return fail(h, SC_ERR_INVALID, "fallback_type must be 1 (Agglomerative) or 2 (Naive)");
  if (stage->single_condition < 0 || stage->single_condition > SC_SINGLE_BY_FALLBACK)
    return fail(h, SC_ERR_INVALID, "single_condition must be 0 (no test) or 1 .. 5");
  FallbackSpec fallback;
  fallback.naive = stage->fallback_type == kNaive;
  fallback.threshold = fallback.naive ? stage->naive_threshold : stage->agglomerative_threshold;
  fallback.adaptation = stage->naive_adaptation_threshold;
  SingleSpec test;
  test.condition = stage->single_condition;
  test.check.condition = stage->single_condition;
  test.check.diagonal_offset = stage->diagonal_offset;
  test.check.threshold = stage->single_threshold;
  test.single = single;
  return predict_batch_reduced_entry(h, "sc_predict_batch_multi_stage", xs, count, cfg,
                                     stage->max_spectral_size, stage->spectral_min_embeddings,
                                     fallback, labels, diags, group, kinds, &test);
}

extern "C" int sc_batch_naive_cluster(sc_handle h, const sc_array* xs, int count, double threshold,
                                      double adaptation_threshold, int64_t* const* labels,
                                      int32_t* n_clusters, double* const* centroids,
                                      int32_t* const* counts) {
  if (!h) return SC_ERR_INVALID;
  if (!xs || !labels || !n_clusters || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  SC_TRY(validate_naive_thresholds(h, threshold, adaptation_threshold));
  SC_HIP(h, hipSetDevice(h->device));
  bool device_source = false;
  std::vector<int> ns;
  int d = 0;
  SC_TRY(validate_batch_arrays(h, xs, count, &ns, &d, &device_source, labels));
  std::vector<NaiveMember> members(count);
  for (int i = 0; i < count; ++i) {
    members[i].index = i;
    members[i].n = ns[i];
    members[i].want_centroids = centroids && centroids[i];
  }
  NaiveRun run;
  run.threshold = threshold;
  run.adaptation = adaptation_threshold;
  SC_TRY(naive_members(h, xs, d, &members, run, nullptr));
  for (const NaiveMember& m : members) {  // (nothing is written unless every wave succeeded)
    const int i = m.index, k = m.k();
    std::copy(m.ints.begin(), m.ints.begin() + m.n, labels[i]);
    n_clusters[i] = k;
    if (counts && counts[i]) std::copy(m.ints.begin() + m.n, m.ints.begin() + m.n + k, counts[i]);
    if (m.want_centroids) std::copy(m.cent.begin(), m.cent.end(), centroids[i]);
  }
  return SC_OK;
}

extern "C" int sc_batch_naive_check(sc_handle h, const sc_array* xs, int count, double threshold,
                                    double adaptation_threshold, int32_t* single,
                                    int32_t* stopped_at) {
  if (!h) return SC_ERR_INVALID;
  if (!xs || !single || !stopped_at || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  SC_TRY(validate_naive_thresholds(h, threshold, adaptation_threshold));
  SC_HIP(h, hipSetDevice(h->device));
  bool device_source = false;
  std::vector<int> ns;
  int d = 0;
  SC_TRY(validate_batch_arrays(h, xs, count, &ns, &d, &device_source));
  std::vector<NaiveMember> members(count);
  for (int i = 0; i < count; ++i) {
    members[i].index = i;
    members[i].n = ns[i];
  }
  NaiveRun run;
  run.threshold = threshold;
  run.adaptation = adaptation_threshold;
  run.verdict = true;
  SC_TRY(naive_members(h, xs, d, &members, run, nullptr));
  for (const NaiveMember& m : members) {  // (nothing is written unless every wave succeeded)
    single[m.index] = m.single;
    stopped_at[m.index] = m.stopped_at;
  }
  return SC_OK;
}

extern "C" int sc_batch_fallback_check(sc_handle h, const sc_array* xs, int count,
                                       double distance_threshold, double* heights,
                                       int32_t* single) {
  if (!h) return SC_ERR_INVALID;
  if (!xs || !heights || !single || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  SC_HIP(h, hipSetDevice(h->device));
  bool device_source = false;
  std::vector<int> ns;
  int d = 0;
  SC_TRY(validate_batch_arrays(h, xs, count, &ns, &d, &device_source));
  std::vector<VerdictMember> members;
  SC_TRY(verdict_members(h, ns, &members));
  SC_TRY(fallback_verdicts(h, xs, d, &members, distance_threshold, nullptr));
  for (const VerdictMember& m : members) {  // (nothing is written unless every wave succeeded)
    heights[m.index] = m.height;
    single[m.index] = m.single;
  }
  return SC_OK;
}

extern "C" int sc_predict_batch_single_fallback(sc_handle h, const sc_array* xs, int count,
                                                const sc_config* cfg, double distance_threshold,
                                                int64_t* const* labels, sc_diag* diags,
                                                int group, int32_t* single) {
  if (!h) return SC_ERR_INVALID;
  if (!xs || !labels || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  if (group < 2)
    return fail(h, SC_ERR_INVALID,
                "sc_predict_batch_single_fallback is the grouped form: group >= 2");
  SC_TRY(validate_config(h, cfg));
  SC_HIP(h, hipSetDevice(h->device));
  bool device_source = false;
  std::vector<int> ns;
  int d = 0;
  SC_TRY(validate_batch_arrays(h, xs, count, &ns, &d, &device_source, labels));
  std::vector<VerdictMember> members;
  SC_TRY(verdict_members(h, ns, &members));
  SC_TRY(sc_clear_constraint(h));  // a batch carries none
  if (count == 0) {
    h->last_routes.clear();
    return SC_OK;
  }
  FallbackSpec fallback;
  fallback.threshold = distance_threshold;
  return predict_batch_fallback_condition(h, xs, count, cfg, fallback, ns, d, labels, diags, group,
                                          single, nullptr);
}

extern "C" int sc_predict_batch_single_naive(sc_handle h, const sc_array* xs, int count,
                                             const sc_config* cfg, double naive_threshold,
                                             double naive_adaptation_threshold,
                                             int64_t* const* labels, sc_diag* diags, int group,
                                             int32_t* single) {
  if (!h) return SC_ERR_INVALID;
  if (!xs || !labels || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  if (group < 2)
    return fail(h, SC_ERR_INVALID, "sc_predict_batch_single_naive is the grouped form: group >= 2");
  SC_TRY(validate_naive_thresholds(h, naive_threshold, naive_adaptation_threshold));
  SC_TRY(validate_config(h, cfg));
  SC_HIP(h, hipSetDevice(h->device));
  bool device_source = false;
  std::vector<int> ns;
  int d = 0;
  SC_TRY(validate_batch_arrays(h, xs, count, &ns, &d, &device_source, labels));
  SC_TRY(sc_clear_constraint(h));  // a batch carries none
  if (count == 0) {
    h->last_routes.clear();
    return SC_OK;
  }
  FallbackSpec fallback;
  fallback.naive = true;
  fallback.threshold = naive_threshold;
  fallback.adaptation = naive_adaptation_threshold;
  return predict_batch_fallback_condition(h, xs, count, cfg, fallback, ns, d, labels, diags, group,
                                          single, nullptr);
}
