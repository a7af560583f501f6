// Results go out where the caller wants them: the fp64 values of a handle buffer are narrowed into
// a described array (sc_array: device or host memory, fp64 / fp32 / fp16 / bf16, any non-negative
// element strides that map no two indices to one address) -- the mirror image of ingest.hip.
//   device destination   k_egress_rows / k_egress_tile write it in place on the handle's stream,
//   host compact fp64    the hipMemcpy2DAsync the double* entry points have always issued,
//   any other host view  narrowed on the device into staging of the destination's width (a half
//                        or a quarter of the fp64 bytes over the link), copied out from there.
// The source is either row-major (element (r, c) at src[r * ld + c]: the n x n matrices) or
// column-major (src[c * ld + r]: the eigenvectors).  Both are "lines" of the source's memory:
// line l, position a at src[l * ld + a]; the destination element of (l, a) lies at
// dst[l * dl + a * da].  Which of dl, da is the smaller says which kernel runs (runs_along_columns,
// the ingest's rule).
// Narrowing is fp64 -> fp32 round to nearest even, then fp32 -> fp16 / bf16 round to nearest even
// (what PyTorch's CPU tensor.to(dtype) computes), done on the bits: no dependence on a denormal
// mode, as the ingest widens.
// Labels leave the same way (sc_labels_egress, k_egress_labels): int64 on the host -> the int64 /
// int32 vector, host or device, of any stride >= 1 that each member of a batch names.
// The stage entries on described arrays (sc_stage_*_array) are at the end: ingest, the launches
// of the double* entry, egress.
// What is shared with the way in lives there: the descriptor checks (validate_out_array and
// view_is_injective), the staging buffer (ensure_stage) and the scatter of host rows are
// ingest.hip's; dispatch_dtype, aligned16 and align16 are array_layout.h's.
#include <climits>
#include <cstring>

#include "array_layout.h"
#include "handle.h"

namespace {

// ---- destination memory along the source's lines ------------------------------------------
// kFast (da == 1, base address and line pitch of the destination multiples of 16 bytes): a work
// item is E = 16 / sizeof(T) positions of a line -- E doubles in (16-byte loads: ld is a multiple
// of 16 doubles), one 16-byte store out; the item that straddles the end of the line writes its
// elements one by one, never past the line.  Otherwise an item is one element, adjacent lanes on
// adjacent destination addresses.
template <typename T, bool kFast>
__global__ __launch_bounds__(256) void k_egress_rows(const double* __restrict__ src, int ld, int L,
                                                     int W, T* __restrict__ dst, long long dl,
                                                     long long da) {
  constexpr int E = kFast ? 16 / (int)sizeof(T) : 1;
  const int per_line = (W + E - 1) / E;
  const long long total = (long long)L * per_line;
  for (long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x; item < total;
       item += (long long)gridDim.x * blockDim.x) {
    const int l = (int)(item / per_line);
    const int a0 = (int)(item - (long long)l * per_line) * E;
    const double* in = src + (size_t)l * ld + a0;
    if constexpr (kFast) {
      T* out = dst + l * dl + a0;
      if (a0 + E <= W) {
        Chunk<T> ch;
#pragma unroll
        for (int e = 0; e < E; e += 2) {
          const double2 p = *reinterpret_cast<const double2*>(in + e);
          ch.v[e] = narrow<T>(p.x);
          ch.v[e + 1] = narrow<T>(p.y);
        }
        *reinterpret_cast<Chunk<T>*>(out) = ch;
      } else {
        for (int e = 0; a0 + e < W; ++e) out[e] = narrow<T>(in[e]);
      }
    } else {
      dst[l * dl + a0 * da] = narrow<T>(*in);
    }
  }
}

// ---- destination memory across the source's lines -----------------------------------------
// A transposed view, or the column-major eigenvectors going out to a row-major (n, count) array:
// a workgroup takes a 64 x 64 tile (64 lines x 64 positions), loads it along the source's memory
// (16-byte loads) into LDS under the ingest's swizzle, and stores it along the destination's:
// an item is E consecutive LINES at one position.  E = 16 / sizeof(T) (dl == 1, base address and
// the pitch da of the destination multiples of 16 bytes): one 16-byte store; the item that
// straddles the last line writes its elements one by one.  E = 1: scalar stores, adjacent lanes on
// adjacent lines.  Elements outside the matrix (and the source's padding) reach LDS at most.
template <typename T, int E>
__global__ __launch_bounds__(256) void k_egress_tile(const double* __restrict__ src, int ld, int L,
                                                     int W, T* __restrict__ dst, long long dl,
                                                     long long da) {
  __shared__ alignas(16) double tile[kAffTile * kAffTile];
  const int tiles_a = (W + kAffTile - 1) / kAffTile;
  const int l0 = (int)(blockIdx.x / tiles_a) * kAffTile, a0 = (int)(blockIdx.x % tiles_a) * kAffTile;
#pragma unroll
  for (int it = 0; it < kAffTile * kAffTile / 2 / 256; ++it) {
    const int item = it * 256 + (int)threadIdx.x;
    const int l = item / (kAffTile / 2), a = (item % (kAffTile / 2)) * 2;
    // (a0 + a and ld are even and W <= ld: a pair that begins inside the line ends inside its pitch)
    double2 p = make_double2(0.0, 0.0);
    if (l0 + l < L && a0 + a < W)
      p = *reinterpret_cast<const double2*>(src + (size_t)(l0 + l) * ld + a0 + a);
    *reinterpret_cast<double2*>(tile + aff_at(l, a)) = p;
  }
  __syncthreads();
  constexpr int kPerPos = kAffTile / E;
#pragma unroll
  for (int it = 0; it < kAffTile * kAffTile / E / 256; ++it) {
    const int item = it * 256 + (int)threadIdx.x;
    const int a = item / kPerPos, l = (item % kPerPos) * E;
    const int ga = a0 + a, gl = l0 + l;
    if (ga >= W || gl >= L) continue;
    if constexpr (E > 1) {
      T* out = dst + ga * da + gl;  // (dl == 1)
      if (gl + E <= L) {
        Chunk<T> ch;
#pragma unroll
        for (int e = 0; e < E; ++e) ch.v[e] = narrow<T>(tile[aff_at(l + e, a)]);
        *reinterpret_cast<Chunk<T>*>(out) = ch;
      } else {
        for (int e = 0; gl + e < L; ++e) out[e] = narrow<T>(tile[aff_at(l + e, a)]);
      }
    } else {
      dst[gl * dl + ga * da] = narrow<T>(tile[aff_at(l, a)]);
    }
  }
}

template <typename T>
void launch_egress_typed(hipStream_t s, const double* src, int ld, int L, int W, void* dst,
                         long long dl, long long da) {
  T* p = static_cast<T*>(dst);
  constexpr int E = 16 / (int)sizeof(T);
  if (!runs_along_columns(dl, da, 0)) {  // the destination runs along the lines (or neither way)
    const bool fast = da == 1 && aligned16(dst, dl, sizeof(T), L);
    const long long total = (long long)L * (fast ? (W + E - 1) / E : W);
    const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 1 << 20);
    if (fast)
      hipLaunchKernelGGL((k_egress_rows<T, true>), dim3(blocks), dim3(256), 0, s, src, ld, L, W, p,
                         dl, da);
    else
      hipLaunchKernelGGL((k_egress_rows<T, false>), dim3(blocks), dim3(256), 0, s, src, ld, L, W,
                         p, dl, da);
    return;
  }
  const unsigned tiles = (unsigned)((L + kAffTile - 1) / kAffTile) *
                         (unsigned)((W + kAffTile - 1) / kAffTile);
  if (dl == 1 && aligned16(dst, da, sizeof(T), W))
    hipLaunchKernelGGL((k_egress_tile<T, E>), dim3(tiles), dim3(256), 0, s, src, ld, L, W, p, dl,
                       da);
  else
    hipLaunchKernelGGL((k_egress_tile<T, 1>), dim3(tiles), dim3(256), 0, s, src, ld, L, W, p, dl,
                       da);
}

// (rows, cols) of the source into device memory `dst` of element strides (rs, cs)
void launch_egress(hipStream_t s, int dtype, const double* src, int ld, int rows, int cols,
                   bool column_major, void* dst, long long rs, long long cs) {
  // the stride of a dimension of extent 1 addresses nothing: make it the larger one
  if (rows == 1) rs = std::max<long long>(cs, 1) * cols;
  if (cols == 1) cs = std::max<long long>(rs, 1) * rows;
  const int L = column_major ? cols : rows, W = column_major ? rows : cols;
  const long long dl = column_major ? cs : rs, da = column_major ? rs : cs;
  dispatch_dtype(dtype, [&](auto t) {
    launch_egress_typed<decltype(t)>(s, src, ld, L, W, dst, dl, da);
  });
}

// ---- labels out ----------------------------------------------------------------------------
// The int64 labels of a batch (one packed array) into the int64 / int32 vector each member names in
// device memory, any stride >= 1: blockIdx.y is the member, its entries go round the x-blocks.
struct LabelEgressItem {
  void* dst;
  long long stride;  // elements
  long long src_off; // this member's labels in the packed array
  int n, dtype;
};
__global__ __launch_bounds__(256) void k_egress_labels(const LabelEgressItem* __restrict__ table,
                                                       int first,
                                                       const long long* __restrict__ packed) {
  const LabelEgressItem it = table[first + (int)blockIdx.y];
  const long long* __restrict__ src = packed + it.src_off;
  for (int r = (int)(blockIdx.x * 256 + threadIdx.x); r < it.n; r += (int)gridDim.x * 256) {
    if (it.dtype == SC_DTYPE_I64) static_cast<long long*>(it.dst)[r * it.stride] = src[r];
    else static_cast<int*>(it.dst)[r * it.stride] = (int)src[r];
  }
}

// ---- symmetric within tolerance, decided on the device --------------------------------------
// One pass over the fp64 matrix in tile pairs (I, J) / (J, I), as k_ingest_affinity walks them:
// stats[0] = max |m| and stats[1] = max |m_ij - m_ji| over the pairs of finite, unequal values
// (non-negative doubles order as their bits do), stats[2] != 0 when an unequal pair has a
// non-finite member -- a NaN anywhere, the diagonal included, or an infinity facing anything else.
__global__ __launch_bounds__(256) void k_symmetry_stats(const double* __restrict__ m, int n, int ld,
                                                        unsigned long long* __restrict__ stats) {
  __shared__ alignas(16) double sp[kAffTile * kAffTile];
  __shared__ alignas(16) double sq[kAffTile * kAffTile];
  __shared__ unsigned long long red[3];
  const int nt = (n + kAffTile - 1) / kAffTile;
  int p = (int)blockIdx.x, ti = 0;
  while (p >= nt - ti) {
    p -= nt - ti;
    ++ti;
  }
  const int tj = ti + p, r0 = ti * kAffTile, c0 = tj * kAffTile;
  const bool diag = ti == tj;
  if (threadIdx.x < 3) red[threadIdx.x] = 0ull;
#pragma unroll
  for (int it = 0; it < kAffTile * kAffTile / 2 / 256; ++it) {
    const int item = it * 256 + (int)threadIdx.x;
    const int r = item / (kAffTile / 2), c = (item % (kAffTile / 2)) * 2;
    // (elements outside the matrix are zeros on both sides; the padding columns are not read)
    double2 u = make_double2(0.0, 0.0), v = u;
    if (r0 + r < n && c0 + c < n) {
      const double* at = m + (size_t)(r0 + r) * ld + c0 + c;
      u.x = at[0];
      if (c0 + c + 1 < n) u.y = at[1];
    }
    *reinterpret_cast<double2*>(sp + aff_at(r, c)) = u;
    if (!diag) {
      if (c0 + r < n && r0 + c < n) {
        const double* at = m + (size_t)(c0 + r) * ld + r0 + c;
        v.x = at[0];
        if (r0 + c + 1 < n) v.y = at[1];
      }
      *reinterpret_cast<double2*>(sq + aff_at(r, c)) = v;
    }
  }
  __syncthreads();
  const double* mir = diag ? sp : sq;
  double amax = 0.0, dmax = 0.0;
  bool bad = false;
#pragma unroll 4
  for (int it = 0; it < kAffTile * kAffTile / 256; ++it) {
    const int item = it * 256 + (int)threadIdx.x;
    const int r = item / kAffTile, c = item % kAffTile;
    const double a = sp[aff_at(r, c)], b = mir[aff_at(c, r)];
    amax = fmax(amax, fmax(fabs(a), fabs(b)));  // (fmax drops a NaN: the flag reports it)
    if (!(a == b)) {
      const double d = fabs(a - b);
      if (isfinite(a) && isfinite(b)) dmax = fmax(dmax, d);
      else bad = true;
    }
  }
  atomicMax(&red[0], (unsigned long long)__double_as_longlong(amax));
  atomicMax(&red[1], (unsigned long long)__double_as_longlong(dmax));
  if (bad) red[2] = 1ull;
  __syncthreads();
  if (threadIdx.x < 2) atomicMax(&stats[threadIdx.x], red[threadIdx.x]);
  if (threadIdx.x == 2 && red[2]) stats[2] = 1ull;
}

// np.allclose(m, m.T, rtol=0, atol=1e-12 * max(max|m|, 1e-300)) on the three statistics
bool symmetric_within_tolerance(const unsigned long long* stats) {
  double amax, dmax;
  memcpy(&amax, stats, sizeof(double));
  memcpy(&dmax, stats + 1, sizeof(double));
  if (stats[2]) return false;
  return dmax <= 1e-12 * std::max(amax, 1e-300);
}

// Before the upload into B1: the union of what the double* stage entries do there.  All of them
// drop the resident embeddings / affinity; the eigen entries also set n and ldn (the solvers read
// them), the refine and Laplacian entries also clear n_vec.  Doing all of it for every entry is
// harmless: each field describes state that the upload into B1 invalidates anyway.
void reset_problem(sc_handle h, int n) {
  h->n = n;
  h->ldn = matrix_ld(n);
  h->have_affinity = h->have_cropval = false;
  h->have_x = false;
  h->n_vec = 0;
}

// an (n, n) source into B1 through the affinity ingest (its exact-symmetry word is not used)
int ingest_into_b1(sc_handle h, const sc_array& in, int n) {
  SC_TRY(ensure_matrices(h, n, 0));
  SC_TRY(grow(h, h->symflag, 64));
  reset_problem(h, n);
  bool sync = false;
  return ingest_affinity_into(h, in, ptr<double>(h->B1), matrix_ld(n), ptr<int>(h->symflag) + 3,
                              h->stream, &sync);
}

}  // namespace

// ------------------------------------------------------------------------------
// the one place results leave
// ------------------------------------------------------------------------------
int egress_matrix(sc_handle h, const double* src, int ld, int rows, int cols, bool column_major,
                  const sc_array& out) {
  hipStream_t s = h->stream;
  void* dst = const_cast<void*>(out.data);
  if (out.location == SC_MEM_DEVICE) {
    launch_egress(s, out.dtype, src, ld, rows, cols, column_major, dst, out.row_stride,
                  out.col_stride);
    SC_TRY(check_last(h, "egress launch"));
    SC_HIP(h, hipStreamSynchronize(s));
    return SC_OK;
  }
  const bool rows_copy = (out.col_stride == 1 || cols == 1) && (out.row_stride >= cols || rows == 1);
  if (!column_major && out.dtype == SC_DTYPE_F64 && rows_copy &&
      (out.row_stride == cols || rows == 1))
    return d2h_matrix(h, src, ld, rows, cols, static_cast<double*>(dst));
  // narrowed (and, for the eigenvectors, transposed) on the device into rows of the destination's
  // width on a 16-byte pitch; hipMemcpy2D moves them when it can describe the view, otherwise they
  // are scattered from a packed temporary on the host (the reverse of the ingest's gather)
  const size_t eb = dtype_bytes(out.dtype), width = (size_t)cols * eb;
  const size_t pitch = align16(width);
  SC_TRY(ensure_stage(h, (size_t)rows * pitch, s));
  launch_egress(s, out.dtype, src, ld, rows, cols, column_major, h->Xstage.p,
                (long long)(pitch / eb), 1);
  SC_TRY(check_last(h, "egress launch"));
  if (rows_copy) {
    SC_HIP(h, hipMemcpy2DAsync(dst, rows == 1 ? width : (size_t)out.row_stride * eb, h->Xstage.p,
                               pitch, width, rows, hipMemcpyDeviceToHost, s));
    SC_HIP(h, hipStreamSynchronize(s));
    return SC_OK;
  }
  std::vector<unsigned char> packed((size_t)rows * width);
  SC_HIP(h, hipMemcpy2DAsync(packed.data(), width, h->Xstage.p, pitch, width, rows,
                             hipMemcpyDeviceToHost, s));
  SC_HIP(h, hipStreamSynchronize(s));
  scatter_host_rows(packed.data(), out, rows);
  return SC_OK;
}

// ------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------
extern "C" int sc_stage_egress(sc_handle h, const double* host_src, int rows, int cols,
                               int column_major, const sc_array* out) {
  if (!h) return SC_ERR_INVALID;
  if (!host_src || rows <= 0 || cols <= 0) return fail(h, SC_ERR_INVALID, "source must be (rows, cols)");
  SC_TRY(validate_out_array(h, out, "out", rows, cols));
  SC_HIP(h, hipSetDevice(h->device));
  // a buffer of the call's own at the library's pitch, NaNs wherever the source does not land
  const int lines = column_major ? cols : rows, width = column_major ? rows : cols;
  const int ld = column_major ? round_up(rows, 16) : matrix_ld(cols);
  const size_t bytes = (size_t)lines * ld * sizeof(double);
  // (host_src is the (rows, cols) matrix in rows; the column-major buffer takes its transpose)
  std::vector<double> turned;
  if (column_major) {
    turned.resize((size_t)rows * cols);
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) turned[(size_t)c * rows + r] = host_src[(size_t)r * cols + c];
    host_src = turned.data();
  }
  double* buf = nullptr;
  SC_HIP(h, hipMalloc(reinterpret_cast<void**>(&buf), bytes));
  auto run = [&]() -> int {
    SC_HIP(h, hipMemsetAsync(buf, 0xff, bytes, h->stream));
    SC_TRY(h2d_matrix(h, host_src, lines, width, buf, ld));
    return egress_matrix(h, buf, ld, rows, cols, column_major != 0, *out);
  };
  const int rc = run();
  hipStreamSynchronize(h->stream);
  hipFree(buf);
  return rc;
}

extern "C" int sc_labels_egress(sc_handle h, const int64_t* const* labels, int count,
                                const sc_array* outs) {
  if (!h) return SC_ERR_INVALID;
  if (!labels || !outs || count < 1) return fail(h, SC_ERR_INVALID, "labels egress: bad arguments");
  long long to_device = 0;
  int device_members = 0, max_n = 0;
  for (int i = 0; i < count; ++i) {  // every descriptor before the first byte is written
    if (!labels[i]) return fail(h, SC_ERR_INVALID, "NULL labels");
    if (outs[i].cols < 0 || outs[i].cols > INT_MAX)
      return fail(h, SC_ERR_INVALID, "out " + std::to_string(i) + ": bad length");
    if (outs[i].cols == 0) continue;
    SC_TRY(validate_label_array(h, outs + i, "out", i, outs[i].cols, true));
    if (outs[i].location != SC_MEM_DEVICE) continue;
    to_device += outs[i].cols;
    ++device_members;
    max_n = std::max(max_n, (int)outs[i].cols);
  }
  for (int i = 0; i < count; ++i) {  // host destinations: written here
    const sc_array& o = outs[i];
    if (o.location != SC_MEM_HOST) continue;
    for (int64_t r = 0; r < o.cols; ++r) {
      if (o.dtype == SC_DTYPE_I64)
        static_cast<int64_t*>(const_cast<void*>(o.data))[r * o.col_stride] = labels[i][r];
      else
        static_cast<int32_t*>(const_cast<void*>(o.data))[r * o.col_stride] = (int32_t)labels[i][r];
    }
  }
  if (!device_members) return SC_OK;
  SC_HIP(h, hipSetDevice(h->device));
  const size_t tab_bytes = align16((size_t)device_members * sizeof(LabelEgressItem));
  SC_TRY(grow(h, h->cen_in, tab_bytes + (size_t)to_device * sizeof(int64_t)));
  LabelEgressItem* table_d = ptr<LabelEgressItem>(h->cen_in);
  long long* packed_d = reinterpret_cast<long long*>(ptr<char>(h->cen_in) + tab_bytes);
  std::vector<LabelEgressItem> table;
  std::vector<long long> packed;
  table.reserve(device_members);
  packed.reserve((size_t)to_device);
  for (int i = 0; i < count; ++i) {
    const sc_array& o = outs[i];
    if (o.location != SC_MEM_DEVICE || o.cols == 0) continue;
    table.push_back(LabelEgressItem{const_cast<void*>(o.data), o.col_stride,
                                    (long long)packed.size(), (int)o.cols, o.dtype});
    packed.insert(packed.end(), labels[i], labels[i] + o.cols);
  }
  hipStream_t s = h->stream;
  SC_HIP(h, hipMemcpyAsync(table_d, table.data(), table.size() * sizeof(LabelEgressItem),
                           hipMemcpyHostToDevice, s));
  SC_HIP(h, hipMemcpyAsync(packed_d, packed.data(), packed.size() * sizeof(long long),
                           hipMemcpyHostToDevice, s));
  constexpr int kGridY = 32768;  // members per launch where the member is blockIdx.y
  for (int at = 0; at < device_members; at += kGridY)
    hipLaunchKernelGGL(k_egress_labels,
                       dim3((unsigned)std::min((max_n + 255) / 256, 64),
                            std::min(kGridY, device_members - at)),
                       dim3(256), 0, s, table_d, at, packed_d);
  const int launched = check_last(h, "label egress launch");
  const hipError_t drained = hipStreamSynchronize(s);  // (table and packed are locals)
  SC_TRY(launched);
  SC_HIP(h, drained);
  return SC_OK;
}

extern "C" int sc_stage_affinity_array(sc_handle h, const sc_array* x, const sc_array* out) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_array(h, x));
  const int n = (int)x->rows;
  SC_TRY(validate_out_array(h, out, "out", n, n));
  SC_TRY(sc_set_embeddings_array(h, x));
  SC_TRY(sc_compute_affinity(h));
  return egress_matrix(h, ptr<double>(h->A0), h->ldn, n, n, false, *out);
}

extern "C" int sc_stage_refine_array(sc_handle h, int op, const sc_config* cfg, const sc_array* in,
                                     const sc_array* out) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_config(h, cfg));
  SC_TRY(validate_affinity_array(h, in));
  const int n = (int)in->rows, ld = matrix_ld(n);
  SC_TRY(validate_out_array(h, out, "out", n, n));
  SC_HIP(h, hipSetDevice(h->device));
  SC_TRY(ingest_into_b1(h, *in, n));
  SC_TRY(run_refine_op(h, op, cfg, ptr<double>(h->B1), ptr<double>(h->B2), n, ld));
  return egress_matrix(h, ptr<double>(h->B2), ld, n, n, false, *out);
}

extern "C" int sc_stage_laplacian_array(sc_handle h, int laplacian_type, const sc_array* in,
                                        const sc_array* out) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_affinity_array(h, in));
  if (laplacian_type < SC_LAPLACIAN_AFFINITY || laplacian_type > SC_LAPLACIAN_GRAPH_CUT)
    return fail(h, SC_ERR_INVALID, "laplacian_type must be a LaplacianType");
  const int n = (int)in->rows, ld = matrix_ld(n);
  SC_TRY(validate_out_array(h, out, "out", n, n));
  SC_HIP(h, hipSetDevice(h->device));
  SC_TRY(ingest_into_b1(h, *in, n));
  if (laplacian_type == SC_LAPLACIAN_AFFINITY)
    return egress_matrix(h, ptr<double>(h->B1), ld, n, n, false, *out);
  launch_laplacian(h->stream, ptr<double>(h->B1), ptr<double>(h->B2), n, ld, laplacian_type,
                   ptr<double>(h->deg));
  SC_TRY(check_last(h, "laplacian launch"));
  return egress_matrix(h, ptr<double>(h->B2), ld, n, n, false, *out);
}

extern "C" int sc_stage_eig_array(sc_handle h, const sc_array* in, int count, int descend,
                                  const sc_array* values, const sc_array* vectors,
                                  int* symmetric) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_affinity_array(h, in));
  const int n = (int)in->rows, ld = matrix_ld(n);
  // count 0: the decision alone.  count -1: the default count, which follows the decision -- the
  // outputs hold the larger default (the symmetric one) and the leading columns are written.
  if (count < -1 || count > n || (count <= 0 && !symmetric))
    return fail(h, SC_ERR_INVALID, "bad eigen request");
  const int room = count == -1 ? (n <= 128 ? n : 64) : count;
  if (count != 0) {
    SC_TRY(validate_out_array(h, values, "out values", 1, room));
    SC_TRY(validate_out_array(h, vectors, "out vectors", n, room));
  }
  SC_HIP(h, hipSetDevice(h->device));
  SC_TRY(ingest_into_b1(h, *in, n));
  // symmetric within tolerance? -- three words of statistics come back, not the matrix
  unsigned long long* stats = reinterpret_cast<unsigned long long*>(ptr<char>(h->symflag) + 32);
  unsigned long long host_stats[3];
  SC_HIP(h, hipMemsetAsync(stats, 0, sizeof(host_stats), h->stream));
  const unsigned nt = (unsigned)((n + kAffTile - 1) / kAffTile);
  hipLaunchKernelGGL(k_symmetry_stats, dim3(nt * (nt + 1) / 2), dim3(256), 0, h->stream,
                     ptr<double>(h->B1), n, ld, stats);
  SC_TRY(check_last(h, "symmetry statistics launch"));
  SC_HIP(h, hipMemcpyAsync(host_stats, stats, sizeof(host_stats), hipMemcpyDeviceToHost,
                           h->stream));
  SC_HIP(h, hipStreamSynchronize(h->stream));
  const bool sym = symmetric_within_tolerance(host_stats);
  if (symmetric) *symmetric = sym ? 1 : 0;
  if (count == 0) return SC_OK;
  if (count == -1) count = sym ? room : (n <= 64 ? n : 32);
  std::vector<double> w(count);
  if (sym) {
    SC_TRY(stage_sym_eig_resident(h, n, count, descend, w.data(), true, nullptr));
  } else {
    SC_TRY(ensure_gen(h, n));
    SC_TRY(stage_eig_resident(h, n, count, descend, w.data(), nullptr));
  }
  // the values as one line of the I/O staging buffer, then both results out
  const int ldw = round_up(count, 16);
  SC_TRY(grow(h, h->Eio, (size_t)ldw * sizeof(double)));
  SC_HIP(h, hipMemcpyAsync(h->Eio.p, w.data(), (size_t)count * sizeof(double),
                           hipMemcpyHostToDevice, h->stream));
  sc_array vals = *values, vecs = *vectors;  // (the leading `count` columns of the room given)
  vals.cols = vecs.cols = count;
  SC_TRY(egress_matrix(h, ptr<double>(h->Eio), ldw, 1, count, false, vals));
  return egress_matrix(h, ptr<double>(h->E), round_up(n, 16), n, count, true, vecs);
}
