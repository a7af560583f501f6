// Cluster centroids where the data is (sc_cluster_centroids_arrays): for every member of a batch
// the means of its embedding rows grouped by label, read from described arrays in place and
// written into described arrays -- utils.get_cluster_centroids without a host round trip.
//
// The arithmetic is cluster_centroid_value's (ahc.hip): out[c][f] adds the widened fp64 values
// X[i][f] of the rows with labels[i] == c from 0.0 in ascending i and divides by their count, the
// bits of np.mean(x[labels == c], axis=0).  That order is a chain of dependent adds, so the
// parallelism is the k * d outputs of a member, not its rows; what is left to gain is to give an
// output its own rows only and to have several of their loads in flight ahead of the adds.
//   k_label_extent   (device labels only) labels of any label dtype and stride -> packed int32,
//                    negative ones as -1; the largest label and a "not a label" flag per member.
//                    Host labels take the same pass on the host.  Every error of the call is known
//                    after this pass, before a byte of any output is written.
//   k_label_sort     a wavefront per member: stable counting sort of its labels into a CSR -- S[c],
//                    S[c + 1] bound the rows of cluster c, ascending.  The rank of a row among the
//                    rows of its label in a group of 64 comes from one ballot per label bit.
//   k_centroid_means a thread per (cluster, feature), adjacent lanes on adjacent features; kAhead
//                    rows are loaded before their adds; the mean is narrowed by the egress's rule.
// Host embeddings are packed at their own width and uploaded in one copy, host outputs come back
// from a staging buffer in one copy: the launches are a fixed number per kBatchGridY members and
// the call synchronises twice (after the extent pass, and at the end) whatever `count` is.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "array_layout.h"
#include "handle.h"

namespace {

constexpr int kBatchGridY = 32768;  // members per launch where the member is blockIdx.y
constexpr int kAhead = 8;           // rows of an output whose loads are issued before their adds
constexpr int kMaxLabel = INT_MAX - 1;  // (k = max + 1 is an int32 as well)

struct CentItem {
  const void* x;      // embeddings: the caller's device memory, or the packed upload
  const void* lab;    // the caller's labels (read by k_label_extent when lab_device)
  void* out;          // the caller's device memory, or compact rows in the output staging
  long long xrs, xcs, lstride, ors, ocs;  // element strides
  long long lab_off;  // this member's labels in the packed int32 array
  long long csr_off;  // ... its CSR in the CSR array: S (k + 2 ints), then n row indices
  int xdtype, ldtype, odtype, lab_device;
  int n, d, k, bits;  // bits: of k - 1 (what the sort's ballots have to tell apart)
};

// a label value -> its cluster (negative: -1, no cluster); false for what is no label
__host__ __device__ inline bool label_of_int(long long v, int* out) {
  if (v > kMaxLabel) return false;
  *out = v < 0 ? -1 : (int)v;
  return true;
}
__host__ __device__ inline bool label_of_float(double v, int* out) {
  // (a NaN fails the first test, an infinity the first or the third)
  if (!(v == trunc(v)) || v > (double)kMaxLabel) return false;
  *out = v < 0.0 ? -1 : (int)v;
  return v >= -1.7976931348623157e308;
}
__host__ __device__ inline bool label_at(const void* p, int dtype, long long at, int* out) {
  switch (dtype) {
    case SC_DTYPE_I64: return label_of_int(static_cast<const long long*>(p)[at], out);
    case SC_DTYPE_I32: return label_of_int(static_cast<const int*>(p)[at], out);
    case SC_DTYPE_F64: return label_of_float(static_cast<const double*>(p)[at], out);
    default: return label_of_float((double)static_cast<const float*>(p)[at], out);
  }
}

// blockIdx.y: the member.  info[2 * member] = largest label (-1: none), [2 * member + 1] = 1 when
// a value is no label.
__global__ __launch_bounds__(256) void k_label_extent(const CentItem* __restrict__ table, int first,
                                                      int* __restrict__ lab32,
                                                      int* __restrict__ info) {
  const int member = first + (int)blockIdx.y;
  const CentItem& it = table[member];
  if (!it.lab_device) return;
  __shared__ int red[2];
  if (threadIdx.x < 2) red[threadIdx.x] = threadIdx.x == 0 ? -1 : 0;
  __syncthreads();
  int top = -1, bad = 0;
  int* out = lab32 + it.lab_off;
  for (int r = (int)threadIdx.x; r < it.n; r += 256) {
    int c = -1;
    if (!label_at(it.lab, it.ldtype, (long long)r * it.lstride, &c)) bad = 1;
    out[r] = c;
    top = max(top, c);
  }
  atomicMax(&red[0], top);
  if (bad) red[1] = 1;
  __syncthreads();
  if (threadIdx.x < 2) info[2 * member + (int)threadIdx.x] = red[threadIdx.x];
}

// blockIdx.y: the member; the workgroup is ONE wavefront, so a group of 64 rows is placed by one
// instruction stream and the groups follow each other in row order.
__global__ __launch_bounds__(64) void k_label_sort(const CentItem* __restrict__ table, int first,
                                                   const int* __restrict__ lab32,
                                                   int* __restrict__ csr) {
  const CentItem it = table[first + (int)blockIdx.y];
  const int n = it.n, k = it.k, lane = (int)threadIdx.x;
  const int* __restrict__ lab = lab32 + it.lab_off;
  int* S = csr + it.csr_off;  // k + 2 ints: the count of cluster c is gathered in S[c + 2]
  int* rows = S + k + 2;
  for (int j = lane; j < k + 2; j += 64) S[j] = 0;
  __syncthreads();
  for (int r = lane; r < n; r += 64) {
    const int c = lab[r];
    if (c >= 0) atomicAdd(&S[c + 2], 1);
  }
  __syncthreads();
  // inclusive sums in place: S[c + 1] becomes the first slot of cluster c
  int carry = 0;
  for (int base = 0; base < k + 2; base += 64) {
    const int j = base + lane;
    // (the counts were added by atomics, which work behind the first-level cache: read there)
    int v = j < k + 2 ? __hip_atomic_load(&S[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
#pragma unroll
    for (int step = 1; step < 64; step <<= 1) {
      const int up = __shfl_up(v, step);
      if (lane >= step) v += up;
    }
    if (j < k + 2) S[j] = carry + v;
    carry += __shfl(v, 63);
  }
  __syncthreads();
  // placement: a row goes to the slot S[c + 1] + its rank among the rows of label c in its group
  // of 64; the last of them moves S[c + 1] on.  Afterwards S[c + 1] is the end of cluster c and
  // the beginning of c + 1, and S[0] = 0: cluster c is rows[S[c] .. S[c + 1]).
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int base = 0; base < n; base += 64) {
    const int r = base + lane;
    const int c = r < n ? lab[r] : -1;
    unsigned long long peers = __ballot(c >= 0);
    for (int b = 0; b < it.bits; ++b) {
      const unsigned long long set = __ballot((c >> b) & 1);
      peers &= ((c >> b) & 1) ? set : ~set;
    }
    int slot = 0;
    if (c >= 0) slot = S[c + 1];
    __syncthreads();
    if (c >= 0) {
      rows[slot + __popcll(peers & below)] = r;
      if ((peers >> lane) == 1ull) S[c + 1] = slot + __popcll(peers);  // the highest lane of them
    }
    __syncthreads();
  }
}

// (the pointers of a CentItem come out of a table, so the compiler takes them for generic ones:
//  they are device memory, say so and the loads and stores are global_*, not flat_*)
template <typename T>
using Global = __attribute__((address_space(1))) T;
// (such a pointer addresses scalars: the 2-byte element types go through their bits)
template <typename T>
struct Scalar {
  using type = T;
  static __device__ __forceinline__ T make(type r) { return r; }
  static __device__ __forceinline__ type of(T v) { return v; }
};
template <>
struct Scalar<F16Bits> {
  using type = unsigned short;
  static __device__ __forceinline__ F16Bits make(type r) { return F16Bits{r}; }
  static __device__ __forceinline__ type of(F16Bits v) { return v.v; }
};
template <>
struct Scalar<BF16Bits> {
  using type = unsigned short;
  static __device__ __forceinline__ BF16Bits make(type r) { return BF16Bits{r}; }
  static __device__ __forceinline__ type of(BF16Bits v) { return v.v; }
};

// One output.  The raw elements of kAhead rows are loaded first and widened afterwards: the fp16
// widening has control flow, and loads that follow it in program order are not issued before it.
template <typename TX, typename TO>
__device__ __forceinline__ void centroid_output(const CentItem& it, const int* __restrict__ rows,
                                                int begin, int end, int c, int f) {
  using RX = typename Scalar<TX>::type;
  using RO = typename Scalar<TO>::type;
  const Global<RX>* x = (const Global<RX>*)it.x + (long long)f * it.xcs;
  const long long xrs = it.xrs;
  double acc = 0.0;
  int r = begin;
  for (; r + kAhead <= end; r += kAhead) {
    int at[kAhead];
    RX raw[kAhead];
#pragma unroll
    for (int a = 0; a < kAhead; ++a) at[a] = rows[r + a];
#pragma unroll
    for (int a = 0; a < kAhead; ++a) raw[a] = x[(long long)at[a] * xrs];
#pragma unroll
    for (int a = 0; a < kAhead; ++a) acc += widen(Scalar<TX>::make(raw[a]));
  }
  for (; r < end; ++r) acc += widen(Scalar<TX>::make(x[(long long)rows[r] * xrs]));
  // empty cluster: 0 / 0 = NaN, as np.mean
  ((Global<RO>*)it.out)[(long long)c * it.ors + (long long)f * it.ocs] =
      Scalar<TO>::of(narrow<TO>(acc / (double)(end - begin)));
}

template <typename TX>
__device__ __forceinline__ void centroid_output_to(const CentItem& it, const int* rows, int begin,
                                                   int end, int c, int f) {
  switch (it.odtype) {
    case SC_DTYPE_F64: centroid_output<TX, double>(it, rows, begin, end, c, f); break;
    case SC_DTYPE_F32: centroid_output<TX, float>(it, rows, begin, end, c, f); break;
    case SC_DTYPE_F16: centroid_output<TX, F16Bits>(it, rows, begin, end, c, f); break;
    default: centroid_output<TX, BF16Bits>(it, rows, begin, end, c, f); break;
  }
}

// blockIdx.y: the member; its (cluster, feature) outputs go round the x-blocks, a thread each.
// (The grid's x extent is bounded whatever the largest member of the launch is: a member with
// fewer outputs leaves at most that many workgroups without work.)
__global__ __launch_bounds__(256) void k_centroid_means(const CentItem* __restrict__ table,
                                                        int first, const int* __restrict__ csr) {
  const CentItem it = table[first + (int)blockIdx.y];
  const long long outputs = (long long)it.k * it.d;
  const int* __restrict__ S = csr + it.csr_off;
  const int* __restrict__ rows = S + it.k + 2;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < outputs;
       t += (long long)gridDim.x * 256) {
    const int c = (int)(t / it.d), f = (int)(t - (long long)c * it.d);
    const int begin = S[c], end = S[c + 1];
    switch (it.xdtype) {
      case SC_DTYPE_F64: centroid_output_to<double>(it, rows, begin, end, c, f); break;
      case SC_DTYPE_F32: centroid_output_to<float>(it, rows, begin, end, c, f); break;
      case SC_DTYPE_F16: centroid_output_to<F16Bits>(it, rows, begin, end, c, f); break;
      default: centroid_output_to<BF16Bits>(it, rows, begin, end, c, f); break;
    }
  }
}

// ---- validation ---------------------------------------------------------------------------
std::string member(const char* what, int i) {
  return std::string(what) + " " + std::to_string(i);
}

size_t label_bytes(int dtype) { return dtype == SC_DTYPE_I32 || dtype == SC_DTYPE_F32 ? 4 : 8; }

// the bytes [lo, hi) that a view touches
struct Range {
  uintptr_t lo, hi;
  int index;
};
Range range_of(const sc_array& a, size_t eb, int index) {
  const uintptr_t lo = reinterpret_cast<uintptr_t>(a.data);
  const unsigned long long last = (unsigned long long)(a.rows - 1) * a.row_stride +
                                  (unsigned long long)(a.cols - 1) * a.col_stride;
  return Range{lo, lo + (uintptr_t)((last + 1) * eb), index};
}

// the host side of the call's asynchronous copies: owned by the entry, which drains the stream
// before they go when the run below fails half way
struct CentroidScratch {
  std::vector<CentItem> table;
  std::vector<int> lab_h, info, info_dev;
  std::vector<unsigned char> xpack, opack;
};
constexpr long long kMeanBlocks = 8192;  // workgroups of a k_centroid_means launch, about

// validated descriptors -> the results; a failure may leave copies from `w` queued on the stream
int centroids_run(sc_handle h, const sc_array* xs, const sc_array* labels, int count,
                  const sc_array* outs, int32_t* ks, int d, int total_n, size_t xstage_bytes,
                  bool device_labels, CentroidScratch& w) {
  hipStream_t s = h->stream;
  // ---- the extent pass: labels -> packed int32, the largest of each member ----
  const size_t tab_bytes = align16((size_t)count * sizeof(CentItem));
  const size_t info_bytes = align16((size_t)count * 2 * sizeof(int));
  const size_t lab_bytes = align16((size_t)total_n * sizeof(int));
  SC_TRY(grow(h, h->cen_in, tab_bytes + info_bytes + lab_bytes + xstage_bytes));
  unsigned char* in_base = ptr<unsigned char>(h->cen_in);
  CentItem* table_d = reinterpret_cast<CentItem*>(in_base);
  int* info_d = reinterpret_cast<int*>(in_base + tab_bytes);
  int* lab_d = reinterpret_cast<int*>(in_base + tab_bytes + info_bytes);
  unsigned char* xstage_d = in_base + tab_bytes + info_bytes + lab_bytes;

  std::vector<CentItem>& table = w.table;
  std::vector<int>&lab_h = w.lab_h, &info = w.info, &info_dev = w.info_dev;
  table.resize(count);
  lab_h.resize((size_t)total_n);
  info.assign(2 * (size_t)count, 0);
  long long lab_off = 0;
  for (int i = 0; i < count; ++i) {
    CentItem& it = table[i];
    memset(&it, 0, sizeof(it));
    const sc_array& l = labels[i];
    it.n = (int)xs[i].rows;
    it.d = d;
    it.lab = l.data;
    it.lstride = l.col_stride;
    it.ldtype = l.dtype;
    it.lab_device = l.location == SC_MEM_DEVICE;
    it.lab_off = lab_off;
    lab_off += it.n;
    if (it.lab_device) continue;
    int top = -1;
    for (int r = 0; r < it.n; ++r) {
      int c = -1;
      if (!label_at(l.data, l.dtype, (long long)r * l.col_stride, &c)) info[2 * i + 1] = 1;
      lab_h[(size_t)it.lab_off + r] = c;
      top = std::max(top, c);
    }
    info[2 * i] = top;
  }
  SC_HIP(h, hipMemcpyAsync(lab_d, lab_h.data(), (size_t)total_n * sizeof(int),
                           hipMemcpyHostToDevice, s));
  if (device_labels) {
    info_dev.resize(info.size());
    SC_HIP(h, hipMemcpyAsync(table_d, table.data(), (size_t)count * sizeof(CentItem),
                             hipMemcpyHostToDevice, s));
    for (int at = 0; at < count; at += kBatchGridY)
      hipLaunchKernelGGL(k_label_extent, dim3(1, std::min(kBatchGridY, count - at)), dim3(256), 0,
                         s, table_d, at, lab_d, info_d);
    SC_TRY(check_last(h, "label extent launch"));
    SC_HIP(h, hipMemcpyAsync(info_dev.data(), info_d, info.size() * sizeof(int),
                             hipMemcpyDeviceToHost, s));
    SC_HIP(h, hipStreamSynchronize(s));
    for (int i = 0; i < count; ++i)
      if (table[i].lab_device) {
        info[2 * i] = info_dev[2 * i];
        info[2 * i + 1] = info_dev[2 * i + 1];
      }
  }
  // ---- what the labels say, still before any output byte ----
  long long csr_ints = 0;
  size_t ostage_bytes = 0;
  long long max_outputs = 0;
  for (int i = 0; i < count; ++i) {
    if (info[2 * i + 1]) {
      return fail(h, SC_ERR_INVALID,
                  member("labels of member", i) + ": every label must be a finite integral value "
                                                  "below 2^31 - 1");
    }
    const int k = info[2 * i] + 1;
    if (outs && outs[i].rows < k) {
      return fail(h, SC_ERR_INVALID, member("out of member", i) + " has " +
                                         std::to_string(outs[i].rows) + " rows, the labels make " +
                                         std::to_string(k) + " clusters");
    }
    table[i].k = k;
    int bits = 0;
    while (bits < 31 && (k - 1) >> bits) ++bits;
    table[i].bits = bits;
    table[i].csr_off = csr_ints;
    csr_ints += (long long)k + 2 + table[i].n;
    max_outputs = std::max(max_outputs, (long long)k * d);
    if (outs && outs[i].location == SC_MEM_HOST)
      ostage_bytes += align16((size_t)k * d * dtype_bytes(outs[i].dtype));
  }
  if (ks)
    for (int i = 0; i < count; ++i) ks[i] = table[i].k;
  if (!outs) {
    SC_HIP(h, hipStreamSynchronize(s));
    return SC_OK;
  }
  if (csr_ints > INT_MAX) {
    return fail(h, SC_ERR_INVALID, "centroids: rows and clusters of one call exceed 2^31 - 1");
  }
  const size_t csr_bytes = align16((size_t)csr_ints * sizeof(int));
  SC_TRY(grow(h, h->cen_out, csr_bytes + ostage_bytes));
  int* csr_d = ptr<int>(h->cen_out);
  unsigned char* ostage_d = ptr<unsigned char>(h->cen_out) + csr_bytes;
  // ---- host embeddings: packed at their own width, one upload ----
  std::vector<unsigned char>&xpack = w.xpack, &opack = w.opack;
  xpack.resize(xstage_bytes);
  opack.resize(ostage_bytes);
  size_t xat = 0, oat = 0;
  for (int i = 0; i < count; ++i) {
    CentItem& it = table[i];
    const sc_array& x = xs[i];
    const size_t eb = dtype_bytes(x.dtype);
    it.xdtype = x.dtype;
    if (x.location == SC_MEM_DEVICE) {
      it.x = x.data;
      it.xrs = x.row_stride;
      it.xcs = x.col_stride;
    } else {
      pack_host_rows(x, x.rows, xpack.data() + xat);
      it.x = xstage_d + xat;
      it.xrs = d;
      it.xcs = 1;
      xat += align16((size_t)x.rows * d * eb);
    }
    const sc_array& o = outs[i];
    it.odtype = o.dtype;
    if (o.location == SC_MEM_DEVICE || it.k == 0) {
      it.out = const_cast<void*>(o.data);
      it.ors = o.row_stride;
      it.ocs = o.col_stride;
    } else {
      it.out = ostage_d + oat;
      it.ors = d;
      it.ocs = 1;
      oat += align16((size_t)it.k * d * dtype_bytes(o.dtype));
    }
  }
  if (xstage_bytes)
    SC_HIP(h, hipMemcpyAsync(xstage_d, xpack.data(), xstage_bytes, hipMemcpyHostToDevice, s));
  SC_HIP(h, hipMemcpyAsync(table_d, table.data(), (size_t)count * sizeof(CentItem),
                           hipMemcpyHostToDevice, s));
  // ---- rows by cluster, then the means ----
  for (int at = 0; at < count; at += kBatchGridY) {
    const int members = std::min(kBatchGridY, count - at);
    hipLaunchKernelGGL(k_label_sort, dim3(1, members), dim3(64), 0, s, table_d, at, lab_d, csr_d);
    // x-blocks per member: what its largest member needs, but no more than spreads kMeanBlocks
    // over the members of the launch (64 at the least): the outputs of a larger member go round
    const long long need = (max_outputs + 255) / 256;
    const long long share = std::max<long long>(64, (kMeanBlocks + members - 1) / members);
    if (max_outputs > 0)
      hipLaunchKernelGGL(k_centroid_means, dim3((unsigned)std::min(need, share), members),
                         dim3(256), 0, s, table_d, at, csr_d);
  }
  const int launched = check_last(h, "centroid launch");
  if (launched == SC_OK && ostage_bytes)
    (void)hipMemcpyAsync(opack.data(), ostage_d, ostage_bytes, hipMemcpyDeviceToHost, s);
  const hipError_t drained = hipStreamSynchronize(s);
  SC_TRY(launched);
  SC_HIP(h, drained);
  oat = 0;
  for (int i = 0; i < count; ++i) {
    if (outs[i].location != SC_MEM_HOST || table[i].k == 0) continue;
    scatter_host_rows(opack.data() + oat, outs[i], table[i].k);
    oat += align16((size_t)table[i].k * d * dtype_bytes(outs[i].dtype));
  }
  return SC_OK;
}

}  // namespace

extern "C" int sc_cluster_centroids_arrays(sc_handle h, const sc_array* xs, const sc_array* labels,
                                           int count, const sc_array* outs, int32_t* ks) {
  if (!h) return SC_ERR_INVALID;
  if (!xs || !labels || count < 1 || (!outs && !ks))
    return fail(h, SC_ERR_INVALID, "centroids: xs, labels, count >= 1, and outs or ks");
  // ---- every descriptor, before anything is launched ----
  std::vector<Range> read;
  long long total_n = 0;
  size_t xstage_bytes = 0;
  bool device_labels = false;
  for (int i = 0; i < count; ++i) {
    if (validate_array(h, xs + i) != SC_OK)
      return fail(h, SC_ERR_INVALID, member("member", i) + ": " + h->err);
    if (xs[i].cols != xs[0].cols)
      return fail(h, SC_ERR_INVALID,
                  member("member", i) + ": all embeddings must be (n_i, d) with the same d");
    SC_TRY(validate_label_array(h, labels + i, "labels of member", i, xs[i].rows, false));
    total_n += xs[i].rows;
    if (xs[i].location == SC_MEM_DEVICE) read.push_back(range_of(xs[i], dtype_bytes(xs[i].dtype), i));
    else xstage_bytes += align16((size_t)xs[i].rows * xs[i].cols * dtype_bytes(xs[i].dtype));
    if (labels[i].location == SC_MEM_DEVICE) {
      read.push_back(range_of(labels[i], label_bytes(labels[i].dtype), i));
      device_labels = true;
    }
  }
  const int d = (int)xs[0].cols;
  if (total_n > INT_MAX)
    return fail(h, SC_ERR_INVALID, "centroids: more than 2^31 - 1 rows in one call");
  if (outs) {
    std::sort(read.begin(), read.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
    std::vector<uintptr_t> reach(read.size());  // the furthest end among the ranges up to here
    for (size_t j = 0; j < read.size(); ++j)
      reach[j] = std::max(read[j].hi, j ? reach[j - 1] : (uintptr_t)0);
    for (int i = 0; i < count; ++i) {
      const sc_array& o = outs[i];
      const std::string w = member("out of member", i);
      if (o.rows < 0 || o.rows > INT_MAX)
        return fail(h, SC_ERR_INVALID, w + " must be (rows >= k, d)");
      if (o.cols != d)
        return fail(h, SC_ERR_INVALID, w + " must have " + std::to_string(d) + " columns, not " +
                                           std::to_string(o.cols));
      if (o.rows == 0) continue;  // (room for no cluster: right when every label is negative)
      if (validate_out_array(h, &o, w.c_str(), (int)o.rows, d) != SC_OK) return SC_ERR_INVALID;
      if (o.location != SC_MEM_DEVICE) continue;
      const Range mine = range_of(o, dtype_bytes(o.dtype), i);
      const size_t before = std::lower_bound(read.begin(), read.end(), mine.hi,
                                             [](const Range& a, uintptr_t hi) { return a.lo < hi; }) -
                            read.begin();
      if (before > 0 && reach[before - 1] > mine.lo)
        return fail(h, SC_ERR_INVALID, w + " overlaps embeddings or labels of the call in device "
                                           "memory: they are read in place");
    }
  }
  SC_HIP(h, hipSetDevice(h->device));
  CentroidScratch w;
  const int rc = centroids_run(h, xs, labels, count, outs, ks, d, (int)total_n, xstage_bytes,
                               device_labels, w);
  // the vectors of w feed asynchronous copies: none of them is still queued when they go
  if (rc != SC_OK) (void)hipStreamSynchronize(h->stream);
  return rc;
}
