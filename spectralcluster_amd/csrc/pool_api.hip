// Stream pool (include/spectralcluster_amd.h sc_pool_*): the host side of many multi-stage
// streaming sessions advanced per call.  A session's cache, its unit-norm copy, its distance
// matrix and its centroids live in slabs taken once at creation and indexed by slot; one step
// of S sessions is
//   append      1 copy (the new rows) + 1 copy (the entry table) + k_pool_append
//   precluster  1 copy (slot and row lists) + ceil(S / 16) grouped fp64 GEMMs (Xn Xn^T)
//               + k_pool_cosine_distance + k_ahc_nn_chain_pool (grid = S)
//               + 1 copy back (all merge lists) + 1 synchronisation
//               + the tree cuts on the handle's host workers (ahc_tree.cpp)
//               + 1 copy (all labels) + k_pool_centroids
//   fallback    the same copies, GEMMs, synchronisation and tree cuts (average linkage, cut at a
//               distance threshold, no centroids); the linkage of the sessions of up to
//               SC_POOL_LDS_LINKAGE_MAX rows is k_pool_linkage_lds (grid = S, the distance pass
//               included), larger ones take the two kernels of the pre-clusterer
// whatever S is.  Kernels: ahc.hip, rowops.hip.
#include "ahc_tree.h"
#include "handle.h"
#include "host_pool.h"

#include <thread>

struct sc_pool_s {
  sc_handle h = nullptr;
  int capacity = 0, d = 0, u1 = 0, u2 = 0;
  PoolSlabs slabs;
  void* arena = nullptr;         // every slab below, one allocation
  double* stage = nullptr;       // rows on their way into the caches: max(capacity, u2) x ldx
  int stage_rows = 0;
  int* lists = nullptr;          // device: slots (capacity) | rows (capacity)
  PoolAppendItem* items = nullptr;  // device: capacity entries
  // pinned host twins of what travels every step
  int* h_lists = nullptr;
  PoolAppendItem* h_items = nullptr;
  double* h_Z = nullptr;         // capacity x stride_z
  int* h_labels = nullptr;       // capacity x u2
  std::vector<int> rows;         // cached rows per slot
  std::vector<char> have_centroids;
};

namespace {

size_t align256(size_t bytes) { return (bytes + 255) / 256 * 256; }

int check_slot(sc_pool p, int slot) {
  if (slot < 0 || slot >= p->capacity)
    return fail(p->h, SC_ERR_INVALID, "stream pool: slot " + std::to_string(slot) +
                                          " is outside 0 .. capacity - 1");
  return SC_OK;
}

int check_slot_list(sc_pool p, const int32_t* slots, int count) {
  if (!slots || count < 0 || count > p->capacity)
    return fail(p->h, SC_ERR_INVALID, "stream pool: a list of at most `capacity` slots is needed");
  std::vector<char> seen(p->capacity, 0);
  for (int i = 0; i < count; ++i) {
    SC_TRY(check_slot(p, slots[i]));
    if (seen[slots[i]])
      return fail(p->h, SC_ERR_INVALID,
                  "stream pool: slot " + std::to_string(slots[i]) + " is listed twice");
    seen[slots[i]] = 1;
  }
  return SC_OK;
}

void free_pool(sc_pool p) {
  if (p->arena) (void)hipFree(p->arena);
  if (p->h_lists) (void)hipHostFree(p->h_lists);
  if (p->h_items) (void)hipHostFree(p->h_items);
  if (p->h_Z) (void)hipHostFree(p->h_Z);
  if (p->h_labels) (void)hipHostFree(p->h_labels);
  delete p;
}

}  // namespace

extern "C" int sc_pool_create(sc_handle h, int capacity, int d, int u1, int u2, sc_pool* out) {
  if (!h) return SC_ERR_INVALID;
  if (!out) return fail(h, SC_ERR_INVALID, "stream pool: out is NULL");
  *out = nullptr;
  // (u2 rows are a grid dimension of the distance pass)
  if (capacity <= 0 || d <= 0 || u1 < 2 || u2 <= u1 || u2 > 65535 || capacity > 65535)
    return fail(h, SC_ERR_INVALID,
                "stream pool: needs capacity >= 1, d >= 1 and 2 <= u1 < u2 <= 65535");
  SC_HIP(h, hipSetDevice(h->device));
  const int ldx = round_up(d, 16), ldd = matrix_ld(u2);
  const size_t cap = (size_t)capacity;
  const size_t stride_x = (size_t)u2 * ldx, stride_d = (size_t)u2 * ldd;
  const size_t stride_c = (size_t)u1 * d, stride_z = 4 * (size_t)(u2 - 1);
  const int stage_rows = std::max(capacity, u2);
  // the slabs in the order they are carved below
  const size_t bytes[] = {
      align256(cap * stride_x * sizeof(double)),  // X
      align256(cap * stride_x * sizeof(double)),  // Xn
      align256(cap * stride_d * sizeof(double)),  // D
      align256(cap * stride_c * sizeof(double)),  // centroids
      align256(cap * stride_z * sizeof(double)),  // Z
      align256(cap * u2 * sizeof(int)),           // sizes
      align256(cap * u2 * sizeof(int)),           // chain
      align256(cap * u2 * sizeof(int)),           // labels
      align256((size_t)stage_rows * ldx * sizeof(double)),
      align256(2 * cap * sizeof(int)),
      align256(cap * sizeof(PoolAppendItem))};
  size_t total = 0;
  for (size_t b : bytes) total += b;
  size_t free_bytes = 0, device_bytes = 0;
  SC_HIP(h, hipMemGetInfo(&free_bytes, &device_bytes));
  if ((double)total > 0.85 * (double)free_bytes)
    return fail(h, SC_ERR_OOM,
                "stream pool: " + std::to_string(capacity) + " sessions of up to " +
                    std::to_string(u2) + " x " + std::to_string(d) + " rows need " +
                    std::to_string(total >> 20) + " MiB of device memory, 85 % of the free " +
                    "memory is " + std::to_string((size_t)(0.85 * (double)free_bytes) >> 20) +
                    " MiB");
  sc_pool p = new sc_pool_s;
  p->h = h;
  p->capacity = capacity;
  p->d = d;
  p->u1 = u1;
  p->u2 = u2;
  p->stage_rows = stage_rows;
  p->rows.assign(capacity, 0);
  p->have_centroids.assign(capacity, 0);
  auto bail = [&](hipError_t e, const char* what) {
    h->err = std::string(what) + ": " + hipGetErrorString(e);
    free_pool(p);
    return e == hipErrorOutOfMemory ? SC_ERR_OOM : SC_ERR_HIP;
  };
  hipError_t e = hipMalloc(&p->arena, total);
  if (e != hipSuccess) return bail(e, "stream pool slabs");
  char* at = static_cast<char*>(p->arena);
  void* part[sizeof(bytes) / sizeof(bytes[0])];
  for (size_t i = 0; i < sizeof(bytes) / sizeof(bytes[0]); ++i) {
    part[i] = at;
    at += bytes[i];
  }
  PoolSlabs& s = p->slabs;
  s.X = static_cast<double*>(part[0]);
  s.Xn = static_cast<double*>(part[1]);
  s.stride_x = stride_x;
  s.ldx = ldx;
  s.d = d;
  s.D = static_cast<double*>(part[2]);
  s.stride_d = stride_d;
  s.ldd = ldd;
  s.cent = static_cast<double*>(part[3]);
  s.stride_c = stride_c;
  s.Z = static_cast<double*>(part[4]);
  s.stride_z = stride_z;
  s.size = static_cast<int*>(part[5]);
  s.chain = static_cast<int*>(part[6]);
  s.labels = static_cast<int*>(part[7]);
  s.stride_n = u2;
  p->stage = static_cast<double*>(part[8]);
  p->lists = static_cast<int*>(part[9]);
  p->items = static_cast<PoolAppendItem*>(part[10]);
  if ((e = hipHostMalloc(reinterpret_cast<void**>(&p->h_lists), 2 * cap * sizeof(int))) !=
          hipSuccess ||
      (e = hipHostMalloc(reinterpret_cast<void**>(&p->h_items), cap * sizeof(PoolAppendItem))) !=
          hipSuccess ||
      (e = hipHostMalloc(reinterpret_cast<void**>(&p->h_Z), cap * stride_z * sizeof(double))) !=
          hipSuccess ||
      (e = hipHostMalloc(reinterpret_cast<void**>(&p->h_labels), cap * u2 * sizeof(int))) !=
          hipSuccess)
    return bail(e, "stream pool host staging");
  *out = p;
  return SC_OK;
}

extern "C" int sc_pool_destroy(sc_pool pool) {
  if (!pool) return SC_ERR_INVALID;
  (void)hipSetDevice(pool->h->device);
  (void)hipStreamSynchronize(pool->h->stream);
  free_pool(pool);
  return SC_OK;
}

extern "C" int sc_pool_reset(sc_pool pool, int slot) {
  if (!pool) return SC_ERR_INVALID;
  SC_TRY(check_slot(pool, slot));
  pool->rows[slot] = 0;
  pool->have_centroids[slot] = 0;
  return SC_OK;
}

extern "C" int sc_pool_rows(sc_pool pool, int slot) {
  if (!pool) return SC_ERR_INVALID;
  SC_TRY(check_slot(pool, slot));
  return pool->rows[slot];
}

extern "C" int sc_pool_append(sc_pool pool, const int32_t* slots, const int32_t* counts,
                              int count, const sc_array* rows) {
  if (!pool) return SC_ERR_INVALID;
  sc_handle h = pool->h;
  SC_TRY(check_slot_list(pool, slots, count));
  if (!counts) return fail(h, SC_ERR_INVALID, "stream pool: counts is NULL");
  if (count == 0) return SC_OK;
  SC_HIP(h, hipSetDevice(h->device));
  SC_TRY(validate_array(h, rows));
  if (rows->cols != pool->d)
    return fail(h, SC_ERR_INVALID, "stream pool: rows have " + std::to_string(rows->cols) +
                                       " columns, the pool holds " + std::to_string(pool->d));
  long long total = 0;
  int max_rows = 0;
  for (int i = 0; i < count; ++i) {
    if (counts[i] <= 0 || pool->rows[slots[i]] + (long long)counts[i] > pool->u2)
      return fail(h, SC_ERR_INVALID,
                  "stream pool: slot " + std::to_string(slots[i]) + " would hold " +
                      std::to_string(pool->rows[slots[i]] + (long long)counts[i]) +
                      " rows, U2 is " + std::to_string(pool->u2));
    pool->h_items[i] = PoolAppendItem{slots[i], pool->rows[slots[i]], (int)total, counts[i]};
    total += counts[i];
    max_rows = std::max(max_rows, (int)counts[i]);
  }
  if (total != rows->rows || total > pool->stage_rows)
    return fail(h, SC_ERR_INVALID, "stream pool: rows must hold exactly sum(counts) rows");
  hipStream_t s = h->stream;
  bool sync = false;
  SC_TRY(ingest_rows_into(h, *rows, pool->stage, pool->slabs.ldx, s, &sync));
  SC_HIP(h, hipMemcpyAsync(pool->items, pool->h_items, (size_t)count * sizeof(PoolAppendItem),
                           hipMemcpyHostToDevice, s));
  launch_pool_append(s, pool->slabs, pool->stage, pool->items, count, max_rows);
  SC_TRY(check_last(h, "stream pool append launch"));
  // the source (and h_items) may be reused by the caller's next step
  SC_HIP(h, hipStreamSynchronize(s));
  for (int i = 0; i < count; ++i) {
    pool->rows[slots[i]] += counts[i];
    pool->have_centroids[slots[i]] = 0;
  }
  return SC_OK;
}

// What sc_pool_precluster and sc_pool_fallback share: the sessions of the call are the `count`
// (slot, rows) entries of h_lists, position by position.  One copy of the lists, the grouped
// Xn Xn^T products kGroupMax sessions per launch, the linkage of every session, one copy back of
// the merge lists (z_doubles of each session's stride_z), one synchronisation; on return h_Z
// holds them and the handle's host workers exist.  Positions [0, n_chain) (at most chain_rows
// rows) take k_pool_cosine_distance + k_ahc_nn_chain_pool with `method`; positions
// [n_chain, count) (at most lds_rows rows, average linkage) take k_pool_linkage_lds.
static int pool_linkage(sc_pool pool, int count, int n_chain, int chain_rows, int lds_rows,
                        int method, size_t z_doubles, const char* what) {
  sc_handle h = pool->h;
  const PoolSlabs& sl = pool->slabs;
  SC_HIP(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  int* slots_d = pool->lists;
  int* rows_d = pool->lists + pool->capacity;
  SC_HIP(h, hipMemcpyAsync(pool->lists, pool->h_lists, 2 * (size_t)pool->capacity * sizeof(int),
                           hipMemcpyHostToDevice, s));
  // cosine distances: sc_ahc's unit rows and symmetric product (whole K per tile, as its
  // single-call plan runs a product of this size), 16 sessions per launch, then 1 - clip
  for (int base = 0; base < count; base += kGroupMax) {
    GemmGroupItem items[kGroupMax];
    const int cnt = std::min(kGroupMax, count - base);
    for (int z = 0; z < cnt; ++z) {
      const size_t slot = (size_t)pool->h_lists[base + z];
      items[z].A = sl.Xn + slot * sl.stride_x;
      items[z].lda = sl.ldx;
      items[z].C = sl.D + slot * sl.stride_d;
      items[z].ldc = sl.ldd;
      items[z].n = pool->rows[slot];
      items[z].K = pool->d;
    }
    launch_gemm_nt_group(s, items, cnt, kEpiNone, 0);
  }
  if (n_chain > 0) {
    launch_pool_cosine_distance(s, sl, slots_d, rows_d, n_chain, chain_rows);
    launch_pool_nn_chain(s, sl, slots_d, rows_d, n_chain, method);
  }
#if SC_POOL_LDS_LINKAGE_MAX > 0
  if (count > n_chain)
    launch_pool_linkage_lds(s, sl, slots_d, rows_d, n_chain, count - n_chain, lds_rows);
#endif
  SC_TRY(check_last(h, what));
  if (z_doubles == sl.stride_z)
    SC_HIP(h, hipMemcpyAsync(pool->h_Z, sl.Z, (size_t)count * sl.stride_z * sizeof(double),
                             hipMemcpyDeviceToHost, s));
  else  // short sessions: the head of every merge list
    SC_HIP(h, hipMemcpy2DAsync(pool->h_Z, sl.stride_z * sizeof(double), sl.Z,
                               sl.stride_z * sizeof(double), z_doubles * sizeof(double), count,
                               hipMemcpyDeviceToHost, s));
  SC_HIP(h, hipStreamSynchronize(s));
  // sort, relabel, heap cut: independent per session
  if (!h->gpool) {
    const unsigned hw = std::thread::hardware_concurrency();
    h->gpool = new HostPool(hw >= 64 ? kGroupMax - 1 : (hw >= 8 ? 6 : (hw >= 4 ? 2 : 0)));
  }
  return SC_OK;
}

extern "C" int sc_pool_precluster(sc_pool pool, const int32_t* slots, int count,
                                  int64_t* const* labels_out) {
  if (!pool) return SC_ERR_INVALID;
  sc_handle h = pool->h;
  SC_TRY(check_slot_list(pool, slots, count));
  if (!labels_out) return fail(h, SC_ERR_INVALID, "stream pool: labels_out is NULL");
  if (count == 0) return SC_OK;
  const PoolSlabs& sl = pool->slabs;
  int max_rows = 0;
  for (int i = 0; i < count; ++i) {
    const int n = pool->rows[slots[i]];
    if (n <= pool->u1 || !labels_out[i])
      return fail(h, SC_ERR_INVALID,
                  "stream pool: slot " + std::to_string(slots[i]) + " holds " +
                      std::to_string(n) + " rows, the pre-clusterer needs more than U1 = " +
                      std::to_string(pool->u1));
    pool->h_lists[i] = slots[i];
    pool->h_lists[pool->capacity + i] = n;
    max_rows = std::max(max_rows, n);
  }
  SC_TRY(pool_linkage(pool, count, count, max_rows, 0, SC_LINKAGE_COMPLETE, sl.stride_z,
                      "stream pool pre-cluster launch"));
  hipStream_t s = h->stream;
  int* slots_d = pool->lists;
  int* rows_d = pool->lists + pool->capacity;
  h->gpool->run(count, [&](int i) {
    const int n = pool->h_lists[pool->capacity + i];
    ahc_tree_cut(pool->h_Z + (size_t)i * sl.stride_z, n, pool->u1, 0.0, labels_out[i]);
    int* lab32 = pool->h_labels + (size_t)i * sl.stride_n;
    for (int r = 0; r < n; ++r) lab32[r] = (int)labels_out[i][r];
  });
  SC_HIP(h, hipMemcpyAsync(sl.labels, pool->h_labels, (size_t)count * sl.stride_n * sizeof(int),
                           hipMemcpyHostToDevice, s));
  launch_pool_centroids(s, sl, slots_d, rows_d, count, pool->u1);
  SC_TRY(check_last(h, "stream pool centroid launch"));
  // (h_lists / h_labels are rewritten by the next call: it must find them consumed)
  SC_HIP(h, hipStreamSynchronize(s));
  for (int i = 0; i < count; ++i) pool->have_centroids[slots[i]] = 1;
  return SC_OK;
}

extern "C" int sc_pool_fallback(sc_pool pool, const int32_t* slots, int count,
                                double distance_threshold, int64_t* const* labels_out) {
  if (!pool) return SC_ERR_INVALID;
  sc_handle h = pool->h;
  SC_TRY(check_slot_list(pool, slots, count));
  if (!labels_out) return fail(h, SC_ERR_INVALID, "stream pool: labels_out is NULL");
  for (int i = 0; i < count; ++i)
    if (pool->rows[slots[i]] < 1 || !labels_out[i])
      return fail(h, SC_ERR_INVALID, "stream pool: slot " + std::to_string(slots[i]) +
                                         " holds no rows, or its labels_out entry is NULL");
  // positions: the sessions of the global-memory chain first, then those of the LDS kernel;
  // a session of one row is label 0 and takes no position
  std::vector<int> at;  // position -> index into slots
  int chain_rows = 0, lds_rows = 0;
  for (int i = 0; i < count; ++i)
    if (pool->rows[slots[i]] >= 2 && pool->rows[slots[i]] > kPoolLdsLinkageMax) {
      at.push_back(i);
      chain_rows = std::max(chain_rows, pool->rows[slots[i]]);
    }
  const int n_chain = (int)at.size();
  for (int i = 0; i < count; ++i) {
    const int n = pool->rows[slots[i]];
    if (n == 1) labels_out[i][0] = 0;
    if (n < 2 || n > kPoolLdsLinkageMax) continue;
    at.push_back(i);
    lds_rows = std::max(lds_rows, n);
  }
  const int listed = (int)at.size();
  if (listed == 0) return SC_OK;
  for (int z = 0; z < listed; ++z) {
    pool->h_lists[z] = slots[at[z]];
    pool->h_lists[pool->capacity + z] = pool->rows[slots[at[z]]];
  }
  const PoolSlabs& sl = pool->slabs;
  SC_TRY(pool_linkage(pool, listed, n_chain, chain_rows, lds_rows, SC_LINKAGE_AVERAGE,
                      4 * (size_t)(std::max(chain_rows, lds_rows) - 1),
                      "stream pool fallback launch"));
  h->gpool->run(listed, [&](int z) {
    ahc_tree_cut(pool->h_Z + (size_t)z * sl.stride_z, pool->h_lists[pool->capacity + z], 0,
                 distance_threshold, labels_out[at[z]]);
  });
  return SC_OK;
}

extern "C" int sc_pool_centroids(sc_pool pool, int slot, sc_array* out) {
  if (!pool) return SC_ERR_INVALID;
  SC_TRY(check_slot(pool, slot));
  if (!out) return fail(pool->h, SC_ERR_INVALID, "stream pool: out is NULL");
  if (!pool->have_centroids[slot])
    return fail(pool->h, SC_ERR_INVALID, "stream pool: the slot has no centroids");
  out->data = pool->slabs.cent + (size_t)slot * pool->slabs.stride_c;
  out->dtype = SC_DTYPE_F64;
  out->location = SC_MEM_DEVICE;
  out->rows = pool->u1;
  out->cols = pool->d;
  out->row_stride = pool->d;
  out->col_stride = 1;
  return SC_OK;
}

extern "C" int sc_pool_cache(sc_pool pool, int slot, sc_array* out) {
  if (!pool) return SC_ERR_INVALID;
  SC_TRY(check_slot(pool, slot));
  if (!out) return fail(pool->h, SC_ERR_INVALID, "stream pool: out is NULL");
  if (pool->rows[slot] < 1)
    return fail(pool->h, SC_ERR_INVALID, "stream pool: the slot holds no rows");
  out->data = pool->slabs.X + (size_t)slot * pool->slabs.stride_x;
  out->dtype = SC_DTYPE_F64;
  out->location = SC_MEM_DEVICE;
  out->rows = pool->rows[slot];
  out->cols = pool->d;
  out->row_stride = pool->slabs.ldx;
  out->col_stride = 1;
  return SC_OK;
}

extern "C" int sc_pool_get(sc_pool pool, int slot, int what, double* out) {
  if (!pool) return SC_ERR_INVALID;
  sc_handle h = pool->h;
  SC_TRY(check_slot(pool, slot));
  if (!out) return fail(h, SC_ERR_INVALID, "stream pool: out is NULL");
  SC_HIP(h, hipSetDevice(h->device));
  const PoolSlabs& sl = pool->slabs;
  const size_t row = (size_t)pool->d * sizeof(double);
  if (what == SC_POOL_CACHE) {
    if (pool->rows[slot] > 0)
      SC_HIP(h, hipMemcpy2DAsync(out, row, sl.X + (size_t)slot * sl.stride_x,
                                 (size_t)sl.ldx * sizeof(double), row, pool->rows[slot],
                                 hipMemcpyDeviceToHost, h->stream));
  } else if (what == SC_POOL_CENTROIDS) {
    if (!pool->have_centroids[slot])
      return fail(h, SC_ERR_INVALID, "stream pool: the slot has no centroids");
    SC_HIP(h, hipMemcpyAsync(out, sl.cent + (size_t)slot * sl.stride_c,
                             sl.stride_c * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  } else {
    return fail(h, SC_ERR_INVALID, "stream pool: what must be SC_POOL_CACHE or SC_POOL_CENTROIDS");
  }
  SC_HIP(h, hipStreamSynchronize(h->stream));
  return SC_OK;
}

extern "C" int sc_pool_compress(sc_pool pool, int slot) {
  if (!pool) return SC_ERR_INVALID;
  sc_handle h = pool->h;
  SC_TRY(check_slot(pool, slot));
  if (!pool->have_centroids[slot])
    return fail(h, SC_ERR_INVALID, "stream pool: the slot has no centroids");
  SC_HIP(h, hipSetDevice(h->device));
  const PoolSlabs& sl = pool->slabs;
  const size_t row = (size_t)pool->d * sizeof(double);
  double* X = sl.X + (size_t)slot * sl.stride_x;
  // (the padding columns d .. ldx of the cache rows are zero already and stay so)
  SC_HIP(h, hipMemcpy2DAsync(X, (size_t)sl.ldx * sizeof(double),
                             sl.cent + (size_t)slot * sl.stride_c, row, row, pool->u1,
                             hipMemcpyDeviceToDevice, h->stream));
  launch_pool_renormalize(h->stream, sl, slot, pool->u1);
  SC_TRY(check_last(h, "stream pool compression launch"));
  pool->rows[slot] = pool->u1;
  pool->have_centroids[slot] = 0;
  return SC_OK;
}
