// Embeddings come in where they are: a described array (sc_array: device or host memory, fp64 /
// fp32 / fp16 / bf16, any element strides) is widened into the handle's fp64 X buffer.
//   device source        k_ingest_rows reads it in place on the call's stream,
//   host fp64            the hipMemcpy2DAsync the double* entry points have always issued,
//   host fp32/fp16/bf16  copied at their own width into a staging buffer of the handle (a half
//                        or a quarter of the fp64 bytes over the link), then the same kernel.
// All arithmetic after this stays fp64, and widening is exact for every bit pattern, so results
// are bit for bit those of the values converted to double on the host.
// An (n, n) affinity or constraint matrix (k_ingest_affinity) and the (n, dim) input of the
// k-means entries (k_ingest_columns: the column-major layout of the k-means kernels) come in the
// same way, through the same widening and the same LDS tile.
//
// The file in order: the kernels and their launches (element type by dispatch_dtype, wide
// accesses by aligned16: array_layout.h); the one host staging path (pack_host_rows /
// scatter_host_rows, ensure_stage, stage_host_rows), which the egress and the centroids use as
// well; the one descriptor check (validate_view) behind the validate_* roles of every
// translation unit; then the three ways in (rows, columns, affinity) and the entry points.
#include <climits>
#include <cstddef>

#include "array_layout.h"
#include "handle.h"

namespace {

// One work item = 16 bytes of a source row = E elements = E doubles of X (E / 2 stores of 16
// bytes).  A row of X has ldx = round_up(d, 16) doubles and E divides 16, so the items of a row
// tile it exactly: items past column d write the zero padding, the item that straddles d reads
// its elements one by one (never past the row).  kFast: col_stride == 1, base address and row
// pitch in bytes multiples of 16 -- the whole items are one 16-byte load.  Otherwise every
// element is a scalar load at its strided address.
template <typename T, bool kFast>
__global__ __launch_bounds__(256) void k_ingest_rows(const T* __restrict__ src, long long row_stride,
                                                     long long col_stride, int n, int d,
                                                     double* __restrict__ X, int ldx) {
  constexpr int E = 16 / (int)sizeof(T);
  const int per_row = ldx / E;
  const long long total = (long long)n * per_row;
  for (long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x; item < total;
       item += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(item / per_row);
    const int c0 = (int)(item - (long long)r * per_row) * E;
    const T* row = src + (long long)r * row_stride;
    double w[E];
    if (kFast && c0 + E <= d) {
      const Chunk<T> ch = *reinterpret_cast<const Chunk<T>*>(row + c0);
#pragma unroll
      for (int e = 0; e < E; ++e) w[e] = widen(ch.v[e]);
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e)
        w[e] = c0 + e < d ? widen(row[(long long)(c0 + e) * (kFast ? 1 : col_stride)]) : 0.0;
    }
    double2* out = reinterpret_cast<double2*>(X + (size_t)r * ldx + c0);
#pragma unroll
    for (int e = 0; e < E; e += 2) out[e / 2] = make_double2(w[e], w[e + 1]);
  }
}

template <typename T>
void launch_ingest_typed(hipStream_t s, const void* src, long long row_stride, long long col_stride,
                         int n, int d, double* X, int ldx) {
  constexpr int E = 16 / (int)sizeof(T);
  const long long total = (long long)n * (ldx / E);
  const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 1 << 20);
  const bool fast = col_stride == 1 && aligned16(src, row_stride, sizeof(T), n);
  const T* p = static_cast<const T*>(src);
  if (fast)
    hipLaunchKernelGGL((k_ingest_rows<T, true>), dim3(blocks), dim3(256), 0, s, p, row_stride,
                       col_stride, n, d, X, ldx);
  else
    hipLaunchKernelGGL((k_ingest_rows<T, false>), dim3(blocks), dim3(256), 0, s, p, row_stride,
                       col_stride, n, d, X, ldx);
}

void launch_ingest_rows(hipStream_t s, int dtype, const void* src, long long row_stride,
                        long long col_stride, int n, int d, double* X, int ldx) {
  dispatch_dtype(dtype, [&](auto t) {
    launch_ingest_typed<decltype(t)>(s, src, row_stride, col_stride, n, d, X, ldx);
  });
}

// ---- an (n, n) affinity where it is -> fp64 rows of pitch ld, and its symmetry flag ----------
// A workgroup takes the 64 x 64 tile (I, J), I <= J, together with its mirror (J, I): both are
// widened into LDS, stored from there in rows (16-byte stores), and compared element against
// transposed element -- every source byte is read once, the flag costs no second pass.
//   kAffVec   col_stride 1, base and row pitch multiples of 16 bytes: 16-byte loads (the item that
//             straddles column n reads its elements one by one, never past the row)
//   kAffRows  scalar loads, adjacent lanes on adjacent columns (col_stride <= row_stride)
//   kAffCols  scalar loads, adjacent lanes on adjacent ROWS: a transposed view is walked along
//             its memory, LDS does the transposition
//   kAffVecCols  kAffVec for a transposed view: row_stride 1, base and column pitch multiples of
//             16 bytes -- 16-byte loads down the columns
// LDS rows are not padded (two fp64 tiles are the whole 64 KB): the pair index of a row is
// XOR-ed with the row number instead, which keeps 16-byte pairs together and spreads a column
// over all banks.
enum { kAffVec = 0, kAffRows = 1, kAffCols = 2, kAffVecCols = 3 };

// (the source has nr rows and nc columns: an affinity passes n twice, the k-means ingest the
// transposed view of an (n, dim) input)
template <typename T, int E, bool COLWALK>
__device__ __forceinline__ void aff_load_tile(const T* __restrict__ src, long long rs,
                                              long long cs, int nr, int nc, int r0, int c0,
                                              double* __restrict__ lds) {
  // an item is E elements along the walked direction: of a row, or (COLWALK) of a column
  constexpr int kPerLine = kAffTile / E;
  const int nline = COLWALK ? nc : nr, nat = COLWALK ? nr : nc;
#pragma unroll
  for (int it = 0; it < kAffTile * kAffTile / E / 256; ++it) {
    const int item = it * 256 + (int)threadIdx.x;
    const int line = item / kPerLine, at = (item % kPerLine) * E;
    const int r = COLWALK ? at : line, c = COLWALK ? line : at;
    const int gr = r0 + r, gc = c0 + c;
    if constexpr (E > 1) {
      // (the walked stride is 1: kAffVec walks rows, kAffVecCols columns)
      const long long base = COLWALK ? (long long)gc * cs + gr : (long long)gr * rs + gc;
      const int gline = COLWALK ? gc : gr, gat = COLWALK ? gr : gc;
      double w[E];
      if (gline < nline && gat + E <= nat) {
        const Chunk<T> ch = *reinterpret_cast<const Chunk<T>*>(src + base);
#pragma unroll
        for (int e = 0; e < E; ++e) w[e] = widen(ch.v[e]);
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) w[e] = gline < nline && gat + e < nat ? widen(src[base + e]) : 0.0;
      }
      if constexpr (COLWALK) {
#pragma unroll
        for (int e = 0; e < E; ++e) lds[aff_at(r + e, c)] = w[e];
      } else {
#pragma unroll
        for (int e = 0; e < E; e += 2)
          *reinterpret_cast<double2*>(lds + aff_at(r, c + e)) = make_double2(w[e], w[e + 1]);
      }
    } else {
      lds[aff_at(r, c)] =
          gr < nr && gc < nc ? widen(src[(long long)gr * rs + (long long)gc * cs]) : 0.0;
    }
  }
}

// rows of one tile from LDS to dst (only elements inside the matrix)
__device__ __forceinline__ void aff_store_pair(double* __restrict__ dst, int ld, int n, int gr,
                                               int gc, double2 v) {
  if (gr >= n || gc >= n) return;
  double* out = dst + (size_t)gr * ld + gc;
  if (gc + 1 < n) *reinterpret_cast<double2*>(out) = v;
  else *out = v.x;
}

struct AffIngestItem {
  const void* src;
  long long row_stride, col_stride;  // elements
  double* dst;
  int* flag;  // set to 1 before the launch; cleared when an (i, j) differs from (j, i)
  int n, ld, dtype, mode;
};

template <typename T, int E, bool COLWALK>
__device__ __forceinline__ void aff_ingest_tiles(const AffIngestItem& m, int ti, int tj,
                                                 double* __restrict__ sp,
                                                 double* __restrict__ sq) {
  const T* src = static_cast<const T*>(m.src);
  const int n = m.n, ld = m.ld, r0 = ti * kAffTile, c0 = tj * kAffTile;
  const bool diag = ti == tj;
  aff_load_tile<T, E, COLWALK>(src, m.row_stride, m.col_stride, n, n, r0, c0, sp);
  if (!diag) aff_load_tile<T, E, COLWALK>(src, m.row_stride, m.col_stride, n, n, c0, r0, sq);
  __syncthreads();
  const double* mir = diag ? sp : sq;
  bool differs = false;
#pragma unroll
  for (int it = 0; it < kAffTile * kAffTile / 2 / 256; ++it) {
    const int item = it * 256 + (int)threadIdx.x;
    const int r = item / (kAffTile / 2), c = (item % (kAffTile / 2)) * 2;
    const double2 p = *reinterpret_cast<const double2*>(sp + aff_at(r, c));
    // k_symmetry_flag's test, on the pairs above the diagonal (elements outside the matrix are
    // zeros on both sides)
    if (!diag || c > r) differs |= !(p.x == mir[aff_at(c, r)]);
    if (!diag || c + 1 > r) differs |= !(p.y == mir[aff_at(c + 1, r)]);
    aff_store_pair(m.dst, ld, n, r0 + r, c0 + c, p);
    if (!diag)
      aff_store_pair(m.dst, ld, n, c0 + r, r0 + c,
                     *reinterpret_cast<const double2*>(sq + aff_at(r, c)));
  }
  if (differs) *m.flag = 0;
  if (diag) {  // the padding columns of these 64 rows
    const int gr = r0 + ((int)threadIdx.x >> 2);
    if (gr < n)
      for (int c = n + ((int)threadIdx.x & 3); c < ld; c += 4) m.dst[(size_t)gr * ld + c] = 0.0;
  }
}

template <typename T>
__device__ __forceinline__ void aff_ingest_modes(const AffIngestItem& m, int ti, int tj,
                                                 double* sp, double* sq) {
  if (m.mode == kAffVec) aff_ingest_tiles<T, 16 / (int)sizeof(T), false>(m, ti, tj, sp, sq);
  else if (m.mode == kAffRows) aff_ingest_tiles<T, 1, false>(m, ti, tj, sp, sq);
  else if (m.mode == kAffCols) aff_ingest_tiles<T, 1, true>(m, ti, tj, sp, sq);
  else aff_ingest_tiles<T, 16 / (int)sizeof(T), true>(m, ti, tj, sp, sq);
}

// block p of a member: the p-th tile pair of the upper triangle, row by row
__device__ __forceinline__ void aff_ingest_block(const AffIngestItem& m, int p, double* sp,
                                                 double* sq) {
  const int nt = (m.n + kAffTile - 1) / kAffTile;
  if (p >= nt * (nt + 1) / 2) return;  // (a smaller member of a group)
  int ti = 0;
  while (p >= nt - ti) {
    p -= nt - ti;
    ++ti;
  }
  const int tj = ti + p;
  switch (m.dtype) {
    case SC_DTYPE_F64: aff_ingest_modes<double>(m, ti, tj, sp, sq); break;
    case SC_DTYPE_F32: aff_ingest_modes<float>(m, ti, tj, sp, sq); break;
    case SC_DTYPE_F16: aff_ingest_modes<F16Bits>(m, ti, tj, sp, sq); break;
    default: aff_ingest_modes<BF16Bits>(m, ti, tj, sp, sq); break;
  }
}

__global__ __launch_bounds__(256) void k_ingest_affinity(AffIngestItem m) {
  __shared__ alignas(16) double sp[kAffTile * kAffTile];
  __shared__ alignas(16) double sq[kAffTile * kAffTile];
  aff_ingest_block(m, (int)blockIdx.x, sp, sq);
}

// blockIdx.y: the member; its descriptor comes from a table in device memory
__global__ __launch_bounds__(256) void k_ingest_affinity_group(
    const AffIngestItem* __restrict__ members) {
  __shared__ alignas(16) double sp[kAffTile * kAffTile];
  __shared__ alignas(16) double sq[kAffTile * kAffTile];
  const AffIngestItem m = members[blockIdx.y];
  aff_ingest_block(m, (int)blockIdx.x, sp, sq);
}

unsigned aff_blocks(int n) {
  const unsigned nt = (unsigned)((n + kAffTile - 1) / kAffTile);
  return nt * (nt + 1) / 2;
}

AffIngestItem aff_item(int dtype, const void* src, long long row_stride, long long col_stride,
                       int n, double* dst, int ld, int* flag) {
  const size_t eb = dtype_bytes(dtype);
  AffIngestItem m;
  m.src = src;
  m.row_stride = row_stride;
  m.col_stride = col_stride;
  m.dst = dst;
  m.flag = flag;
  m.n = n;
  m.ld = ld;
  m.dtype = dtype;
  if (col_stride == 1 && aligned16(src, row_stride, eb, n))
    m.mode = kAffVec;
  else if (row_stride == 1 && aligned16(src, col_stride, eb, n))
    m.mode = kAffVecCols;
  else
    m.mode = col_stride > row_stride ? kAffCols : kAffRows;
  return m;
}

// ---- an (n, dim) input where it is -> the k-means layout X[j * ld + r], fp64 -----------------
// X has the shape of the source's transposed view ((dim, n), the two strides swapped) in rows of
// pitch ld = round_up(n, 16).  Which way the source's memory runs decides the kernel:
//   along its rows (col_stride 1, or the smaller stride)  k_ingest_columns: a workgroup takes a
//     64 x 64 tile, loads it along the memory with the affinity ingest's column walk of the
//     transposed view (E > 1: 16-byte loads -- col_stride 1, base and row pitch multiples of 16
//     bytes; E = 1: scalar loads, adjacent lanes on adjacent columns), LDS does the transposition
//     (aff_at's swizzle), and the stores run down the columns of X, 16 bytes each;
//   along its columns (row_stride 1: it is column-major already; or the smaller stride)
//     nothing is to be transposed: k_ingest_rows on the transposed view.
// Either way every source byte is read once and every element of X is written once, rows
// n .. ld - 1 of each column as zeros (no k-means kernel reads them; they are defined all the
// same, as the embedding ingest defines its padding columns).
template <typename T, int E>
__global__ __launch_bounds__(256) void k_ingest_columns(const T* __restrict__ src,
                                                        long long row_stride, long long col_stride,
                                                        int n, int dim, double* __restrict__ X,
                                                        int ld) {
  __shared__ alignas(16) double tile[kAffTile * kAffTile];
  const int tiles_r = (n + kAffTile - 1) / kAffTile;
  const int r0 = (int)(blockIdx.x % tiles_r) * kAffTile, j0 = (int)(blockIdx.x / tiles_r) * kAffTile;
  // tile[aff_at(j, r)] = source(r0 + r, j0 + j), zero outside the source
  aff_load_tile<T, E, true>(src, col_stride, row_stride, dim, n, j0, r0, tile);
  __syncthreads();
#pragma unroll
  for (int it = 0; it < kAffTile * kAffTile / 2 / 256; ++it) {
    const int item = it * 256 + (int)threadIdx.x;
    const int j = item / (kAffTile / 2), r = (item % (kAffTile / 2)) * 2;
    // (r0 + r and ld are even: a pair lies inside the column or outside it)
    if (j0 + j < dim && r0 + r < ld)
      *reinterpret_cast<double2*>(X + (size_t)(j0 + j) * ld + r0 + r) =
          *reinterpret_cast<const double2*>(tile + aff_at(j, r));
  }
}

template <typename T>
void launch_ingest_columns_typed(hipStream_t s, const void* src, long long row_stride,
                                 long long col_stride, int n, int dim, double* X, int ld) {
  const unsigned tiles = (unsigned)((n + kAffTile - 1) / kAffTile) *
                         (unsigned)((dim + kAffTile - 1) / kAffTile);
  const bool vec = col_stride == 1 && aligned16(src, row_stride, sizeof(T), n);
  const T* p = static_cast<const T*>(src);
  if (vec)
    hipLaunchKernelGGL((k_ingest_columns<T, 16 / (int)sizeof(T)>), dim3(tiles), dim3(256), 0, s, p,
                       row_stride, col_stride, n, dim, X, ld);
  else
    hipLaunchKernelGGL((k_ingest_columns<T, 1>), dim3(tiles), dim3(256), 0, s, p, row_stride,
                       col_stride, n, dim, X, ld);
}

void launch_ingest_columns(hipStream_t s, int dtype, const void* src, long long row_stride,
                           long long col_stride, int n, int dim, double* X, int ld) {
  if (runs_along_columns(row_stride, col_stride, dim)) {
    launch_ingest_rows(s, dtype, src, col_stride, row_stride, dim, n, X, ld);
    return;
  }
  dispatch_dtype(dtype, [&](auto t) {
    launch_ingest_columns_typed<decltype(t)>(s, src, row_stride, col_stride, n, dim, X, ld);
  });
}

}  // namespace

// ------------------------------------------------------------------------------
// host rows <-> device staging memory
// ------------------------------------------------------------------------------
// The first `rows` rows of a host view, gathered at the view's width into compact rows at `out`
// -- and the way back.  (For what hipMemcpy2D cannot describe: a column stride, rows that overlap.)
void pack_host_rows(const sc_array& a, int64_t rows, unsigned char* out) {
  const size_t eb = dtype_bytes(a.dtype), width = (size_t)a.cols * eb;
  const unsigned char* base = static_cast<const unsigned char*>(a.data);
  for (int64_t r = 0; r < rows; ++r) {
    const unsigned char* row = base + (size_t)(r * a.row_stride) * eb;
    if (a.col_stride == 1) {
      memcpy(out, row, width);
      out += width;
    } else {
      for (int64_t c = 0; c < a.cols; ++c, out += eb) memcpy(out, row + (size_t)(c * a.col_stride) * eb, eb);
    }
  }
}

void scatter_host_rows(const unsigned char* in, const sc_array& a, int64_t rows) {
  const size_t eb = dtype_bytes(a.dtype);
  unsigned char* base = static_cast<unsigned char*>(const_cast<void*>(a.data));
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t c = 0; c < a.cols; ++c, in += eb)
      memcpy(base + (size_t)(r * a.row_stride + c * a.col_stride) * eb, in, eb);
}

// The handle's staging buffer holds `bytes` for work on stream s.  (What is queued on another
// stream than the handle's may still read the buffer that a reallocation frees: waited for.)
int ensure_stage(sc_handle h, size_t bytes, hipStream_t s) {
  if (h->Xstage.bytes >= bytes) return SC_OK;
  if (h->Xstage.p && s != h->stream) SC_HIP(h, hipStreamSynchronize(s));
  return grow(h, h->Xstage, bytes);
}

// Host rows at their own width into device memory `stage` of row pitch `pitch` bytes on stream
// s: one hipMemcpy2DAsync where it can describe them, gathered into `packed` first where it
// cannot.  The one place that decides between the two.  *sync is set when `packed` feeds the
// copy: the caller waits for s while `packed` lives.
int stage_host_rows(sc_handle h, const sc_array& a, void* stage, size_t pitch, hipStream_t s,
                    std::vector<unsigned char>* packed, bool* sync) {
  const int n = (int)a.rows;
  const size_t eb = dtype_bytes(a.dtype), width = (size_t)a.cols * eb;
  const void* src = a.data;
  size_t spitch = (size_t)a.row_stride * eb;
  if (a.col_stride != 1 || (a.row_stride < a.cols && n > 1)) {
    packed->resize((size_t)n * width);
    pack_host_rows(a, n, packed->data());
    src = packed->data();
    spitch = width;
    *sync = true;
  }
  if (n == 1) spitch = width;  // (the pitch of one row addresses nothing)
  SC_HIP(h, hipMemcpy2DAsync(stage, pitch, src, spitch, width, n, hipMemcpyHostToDevice, s));
  return SC_OK;
}

// ------------------------------------------------------------------------------
// validation (no launch, no copy)
// ------------------------------------------------------------------------------
bool is_device_memory_of(sc_handle h, const void* p) {
  hipPointerAttribute_t attr;
  memset(&attr, 0, sizeof(attr));
  const hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) (void)hipGetLastError();  // (the failed query is sticky otherwise)
  return e == hipSuccess && attr.type == hipMemoryTypeDevice && attr.device == h->device;
}

// no two indices of a (rows, cols) view of element strides (rs, cs) share an address: over the
// dimensions of more than one element, ordered by stride, small >= 1 and big >= small * extent
bool view_is_injective(long long rows, long long cols, long long rs, long long cs) {
  if (rows > 1 && cols > 1) {
    const bool rows_small = rs < cs;
    const long long small = rows_small ? rs : cs, big = rows_small ? cs : rs;
    const long long extent = rows_small ? rows : cols;
    return small >= 1 && big / extent >= small;  // (no overflow: big >= small * extent)
  }
  if (rows > 1) return rs >= 1;
  if (cols > 1) return cs >= 1;
  return true;
}

namespace {

// What a role asks of its descriptor beyond the checks every descriptor gets.
struct ViewRule {
  unsigned dtypes;         // bit t: dtype t is taken
  const char* dtype_text;  // the message when it is another one
  int64_t rows, cols;      // the shape; rows < 0: any positive one whose extents fit an int
  bool vector;             // one row of `cols` entries: the row stride addresses nothing
  bool output;             // written: no two indices may share an address
  bool fits_2_31;          // rows * cols <= 2^31 - 1
};
constexpr unsigned kFloatDtypes = 1u << SC_DTYPE_F64 | 1u << SC_DTYPE_F32 | 1u << SC_DTYPE_F16 |
                                  1u << SC_DTYPE_BF16;
constexpr unsigned kLabelDtypes = 1u << SC_DTYPE_I64 | 1u << SC_DTYPE_I32;
constexpr const char* kFloatDtypeText = "unknown dtype (SC_DTYPE_F64 / F32 / F16 / BF16)";

// Every check of the descriptor `what` (SC_ERR_INVALID + message), in the order: present, data
// and shape, dtype, location, strides, injective, really device memory, and what the rule adds
// about the sizes.
int validate_view(sc_handle h, const sc_array* a, const std::string& what, const ViewRule& rule) {
  auto refuse = [&](const std::string& msg) { return fail(h, SC_ERR_INVALID, what + msg); };
  if (!a) return refuse(" descriptor is NULL");
  const bool any = rule.rows < 0;
  if (rule.vector) {
    if (!a->data) return refuse(": data is NULL");
    if (a->rows != 1 || a->cols != rule.cols)
      return refuse(" must hold " + std::to_string(rule.cols) + " entries, not " +
                    std::to_string(a->rows == 1 ? a->cols : a->rows * a->cols));
  } else if (any) {
    if (!a->data || a->rows <= 0 || a->cols <= 0) return refuse(" must be (n, d)");
    if (a->rows > INT_MAX || a->cols > INT_MAX) return refuse(": rows and cols must fit an int");
  } else if (!a->data || a->rows != rule.rows || a->cols != rule.cols) {
    return refuse(" must be (" + std::to_string(rule.rows) + ", " + std::to_string(rule.cols) + ")");
  }
  if (a->dtype < 0 || a->dtype > 31 || !(rule.dtypes >> a->dtype & 1u))
    return refuse(std::string(": ") + rule.dtype_text);
  if (a->location != SC_MEM_HOST && a->location != SC_MEM_DEVICE)
    return refuse(": unknown location (SC_MEM_HOST / SC_MEM_DEVICE)");
  if (a->col_stride < 0 || (!rule.vector && a->row_stride < 0))
    return refuse(rule.vector ? ": the stride must not be negative"
                              : ": strides must not be negative");
  if (rule.output && !view_is_injective(a->rows, a->cols, a->row_stride, a->col_stride))
    return refuse(": the view maps two indices to one address");
  if (a->location == SC_MEM_DEVICE && !is_device_memory_of(h, a->data))
    return refuse(": location is SC_MEM_DEVICE but the pointer is not device memory of the "
                  "handle's device");
  if (rule.fits_2_31 && a->rows * a->cols > 0x7fffffffLL)
    return fail(h, SC_ERR_INVALID, "k-means input larger than 2^31 elements");
  return SC_OK;
}

}  // namespace

// the roles (handle.h says what each is for)
int validate_array(sc_handle h, const sc_array* a) {
  return validate_view(h, a, "embeddings", {kFloatDtypes, kFloatDtypeText, -1, -1});
}
int validate_kmeans_array(sc_handle h, const sc_array* a) {
  return validate_view(h, a, "embeddings",
                       {kFloatDtypes, kFloatDtypeText, -1, -1, false, false, true});
}
int validate_affinity_array(sc_handle h, const sc_array* a, const char* what) {
  SC_TRY(validate_array(h, a));
  if (a->rows != a->cols) return fail(h, SC_ERR_INVALID, std::string(what) + " must be (n, n)");
  return SC_OK;
}
int validate_out_array(sc_handle h, const sc_array* a, const char* what, int rows, int cols) {
  return validate_view(h, a, what, {kFloatDtypes, kFloatDtypeText, rows, cols, false, true});
}
int validate_label_array(sc_handle h, const sc_array* a, const char* what, int i, int64_t n,
                         bool output) {
  const unsigned floats = 1u << SC_DTYPE_F64 | 1u << SC_DTYPE_F32;
  return validate_view(h, a, std::string(what) + " " + std::to_string(i),
                       {output ? kLabelDtypes : kLabelDtypes | floats,
                        output ? "dtype must be SC_DTYPE_I64 or SC_DTYPE_I32"
                               : "dtype must be SC_DTYPE_I64, I32, F64 or F32",
                        1, n, true, output});
}

int validate_batch_arrays(sc_handle h, const sc_array* xs, int count, std::vector<int>* ns, int* d,
                          bool* device_source, int64_t* const* labels) {
  *device_source = false;
  ns->assign(count, 0);
  for (int i = 0; i < count; ++i) {  // every descriptor before the first launch
    SC_TRY(validate_array(h, xs + i));
    if (labels && !labels[i]) return fail(h, SC_ERR_INVALID, "NULL labels");
    if (xs[i].cols != xs[0].cols)
      return fail(h, SC_ERR_INVALID, "all utterances must be (n_i, d) with the same d");
    (*ns)[i] = (int)xs[i].rows;
    *device_source |= xs[i].location == SC_MEM_DEVICE;
  }
  *d = count > 0 ? (int)xs[0].cols : 0;
  return SC_OK;
}

sc_array host_f64_array(const double* x, int n, int d) {
  sc_array a;
  a.data = x;
  a.dtype = SC_DTYPE_F64;
  a.location = SC_MEM_HOST;
  a.rows = n;
  a.cols = d;
  a.row_stride = d;
  a.col_stride = 1;
  return a;
}

bool array_is_host_f64_rows(const sc_array& a) {
  return a.location == SC_MEM_HOST && a.dtype == SC_DTYPE_F64 && a.col_stride == 1 &&
         (a.row_stride >= a.cols || a.rows == 1);
}

// ------------------------------------------------------------------------------
// the one place embeddings enter
// ------------------------------------------------------------------------------
// sc_set_embeddings for a described source: arena, problem size, then the rows into h->X on
// `stream` (default: the handle's).  `sync`: wait for the stream, after which the source may be
// reused (sc_set_embeddings' promise); a batch passes false, its sources outlive the call.
int ingest_embeddings(sc_handle h, const sc_array& a, bool sync, hipStream_t stream) {
  SC_TRY(validate_array(h, &a));
  const int n = (int)a.rows, d = (int)a.cols;
  hipStream_t s = stream ? stream : h->stream;
  SC_TRY(ensure_matrices(h, n, d));
  h->n = n;
  h->d = d;
  h->ldn = matrix_ld(n);
  h->ldx = round_up(d, 16);
  h->have_affinity = h->have_cropval = false;
  h->have_x = false;
  h->n_vec = 0;
  SC_TRY(ingest_rows_into(h, a, ptr<double>(h->X), h->ldx, s, &sync));
  if (sync) SC_HIP(h, hipStreamSynchronize(s));
  h->have_x = true;
  return SC_OK;
}

// The rows of a validated source, widened, into X (row pitch ldx doubles) on stream s; nothing
// else of the handle changes.  *sync is set when the source was packed into a local, so the
// caller must wait for s before it returns.  (A host fp64 source leaves the columns d..ldx of
// X as they were; every other source zeroes them.)
int ingest_rows_into(sc_handle h, const sc_array& a, double* X, int ldx, hipStream_t s,
                     bool* sync) {
  const int n = (int)a.rows, d = (int)a.cols;
  const size_t eb = dtype_bytes(a.dtype);
  std::vector<unsigned char> packed;
  if (a.location == SC_MEM_HOST && a.dtype == SC_DTYPE_F64)  // straight into X, d doubles a row
    return stage_host_rows(h, a, X, (size_t)ldx * sizeof(double), s, &packed, sync);
  const void* src = a.data;
  long long row_stride = a.row_stride, col_stride = a.col_stride;
  if (a.location == SC_MEM_HOST) {
    // staging rows on a 16-byte pitch (the kernel's wide loads); sized with the X buffer, so
    // an arena reserved for the largest member of a batch allocates it once
    const size_t pitch = align16((size_t)d * eb);
    SC_TRY(ensure_stage(h, std::max((size_t)n * pitch, h->X.bytes / sizeof(double) * eb), s));
    SC_TRY(stage_host_rows(h, a, h->Xstage.p, pitch, s, &packed, sync));
    src = h->Xstage.p;
    row_stride = (long long)(pitch / eb);
    col_stride = 1;
  }
  launch_ingest_rows(s, a.dtype, src, row_stride, col_stride, n, d, X, ldx);
  return check_last(h, "ingest launch");
}

// ------------------------------------------------------------------------------
// the one place a described k-means input enters
// ------------------------------------------------------------------------------
bool array_is_compact_host_f64(const sc_array& a) {
  return a.location == SC_MEM_HOST && a.dtype == SC_DTYPE_F64 &&
         (a.col_stride == 1 || a.cols == 1) && (a.row_stride == a.cols || a.rows == 1);
}

// The (n, dim) values of a validated source, widened, into X[j * ld + r] (ld = round_up(n, 16),
// rows n .. ld - 1 zeroed) on stream s.  A device source is read in place; a host source is
// copied at its own width into the handle's staging buffer, in the direction its memory runs (a
// transposed view is staged as the rows it is made of), and read from there.  The caller waits
// for s before it hands the source back (every k-means entry does, for its labels).
int ingest_columns_into(sc_handle h, const sc_array& a, double* X, int ld, hipStream_t s) {
  const int n = (int)a.rows, dim = (int)a.cols;
  if (a.location == SC_MEM_DEVICE) {
    launch_ingest_columns(s, a.dtype, a.data, a.row_stride, a.col_stride, n, dim, X, ld);
    return check_last(h, "k-means ingest launch");
  }
  const size_t eb = dtype_bytes(a.dtype);
  const bool flip = runs_along_columns(a.row_stride, a.col_stride, dim);
  sc_array v = a;  // the view whose rows run along the memory
  if (flip) {
    v.rows = a.cols;
    v.cols = a.rows;
    v.row_stride = a.col_stride;
    v.col_stride = a.row_stride;
  }
  const size_t pitch = align16((size_t)v.cols * eb);
  SC_TRY(ensure_stage(h, (size_t)v.rows * pitch, s));
  std::vector<unsigned char> packed;
  bool sync = false;
  SC_TRY(stage_host_rows(h, v, h->Xstage.p, pitch, s, &packed, &sync));
  const long long step = (long long)(pitch / eb);
  launch_ingest_columns(s, a.dtype, h->Xstage.p, flip ? 1 : step, flip ? step : 1, n, dim, X, ld);
  SC_TRY(check_last(h, "k-means ingest launch"));
  if (sync) SC_HIP(h, hipStreamSynchronize(s));  // (`packed` is a local)
  return SC_OK;
}

// ------------------------------------------------------------------------------
// the one place a caller's affinity enters
// ------------------------------------------------------------------------------
// The (n, n) values of a validated source, widened, into dst (row pitch ld doubles, padding
// columns zeroed) on stream s, and *flag (device memory) = is it exactly symmetric.  *sync as in
// ingest_rows_into.  A host fp64 source takes sc_set_affinity's copy and the separate symmetry
// pass (staging it would cost a second n x n fp64 buffer); everything else is one kernel.
int ingest_affinity_into(sc_handle h, const sc_array& a, double* dst, int ld, int* flag,
                         hipStream_t s, bool* sync_out) {
  static const int kOne = 1;
  const int n = (int)a.rows;
  const size_t eb = dtype_bytes(a.dtype);
  bool sync = false;
  SC_HIP(h, hipMemcpyAsync(flag, &kOne, sizeof(int), hipMemcpyHostToDevice, s));
  if (a.location == SC_MEM_DEVICE) {
    hipLaunchKernelGGL(k_ingest_affinity, dim3(aff_blocks(n)), dim3(256), 0, s,
                       aff_item(a.dtype, a.data, a.row_stride, a.col_stride, n, dst, ld, flag));
    SC_TRY(check_last(h, "affinity ingest launch"));
  } else if (a.dtype == SC_DTYPE_F64) {
    std::vector<unsigned char> packed;
    SC_TRY(stage_host_rows(h, a, dst, (size_t)ld * sizeof(double), s, &packed, &sync));
    if (ld > n)
      SC_HIP(h, hipMemset2DAsync(dst + n, (size_t)ld * sizeof(double), 0,
                                 (size_t)(ld - n) * sizeof(double), n, s));
    launch_symmetry_flag(s, dst, n, ld, flag);
    SC_TRY(check_last(h, "symmetry flag launch"));
    if (sync) SC_HIP(h, hipStreamSynchronize(s));  // (`packed` is a local)
  } else {
    const size_t pitch = align16((size_t)n * eb);
    SC_TRY(ensure_stage(h, (size_t)n * pitch, s));
    std::vector<unsigned char> packed;
    SC_TRY(stage_host_rows(h, a, h->Xstage.p, pitch, s, &packed, &sync));
    hipLaunchKernelGGL(k_ingest_affinity, dim3(aff_blocks(n)), dim3(256), 0, s,
                       aff_item(a.dtype, h->Xstage.p, (long long)(pitch / eb), 1, n, dst, ld, flag));
    SC_TRY(check_last(h, "affinity ingest launch"));
    if (sync) SC_HIP(h, hipStreamSynchronize(s));  // (`packed` is a local)
  }
  if (sync) *sync_out = true;
  return SC_OK;
}

// `count` sources by ONE launch per 64 of them: member z into dsts[z] (pitch matrix_ld(n_z)), its flag
// into flags[z] (device memory).  Host members are copied at their own width into `stage` (device
// memory of affinity_group_stage_bytes bytes) first; `table` holds the descriptors (device memory,
// count * affinity_group_table_bytes()).  The host side of the copies is waited for before return.
size_t affinity_group_table_bytes() { return sizeof(AffIngestItem); }
size_t affinity_group_stage_bytes(const sc_array* as, int count) {
  size_t total = 0;
  for (int z = 0; z < count; ++z)
    if (as[z].location == SC_MEM_HOST)
      total += (size_t)as[z].rows * align16((size_t)as[z].rows * dtype_bytes(as[z].dtype));
  return total;
}
int ingest_affinity_group(sc_handle h, const sc_array* as, int count, double* const* dsts,
                          int* flags, void* stage, void* table, hipStream_t s, int* host_flags) {
  if (count <= 0) return SC_OK;
  std::vector<AffIngestItem> items(count);
  std::vector<int> ones(count, 1);
  std::vector<std::vector<unsigned char>> packed(count);
  unsigned char* at = static_cast<unsigned char*>(stage);
  bool sync = false;
  for (int z = 0; z < count; ++z) {
    const sc_array& a = as[z];
    const int n = (int)a.rows;
    const size_t eb = dtype_bytes(a.dtype);
    if (a.location == SC_MEM_HOST) {
      const size_t pitch = align16((size_t)n * eb);
      SC_TRY(stage_host_rows(h, a, at, pitch, s, &packed[z], &sync));
      items[z] = aff_item(a.dtype, at, (long long)(pitch / eb), 1, n, dsts[z], matrix_ld(n),
                          flags + z);
      at += (size_t)n * pitch;
    } else {
      items[z] = aff_item(a.dtype, a.data, a.row_stride, a.col_stride, n, dsts[z], matrix_ld(n),
                          flags + z);
    }
  }
  SC_HIP(h, hipMemcpyAsync(flags, ones.data(), count * sizeof(int), hipMemcpyHostToDevice, s));
  SC_HIP(h, hipMemcpyAsync(table, items.data(), count * sizeof(AffIngestItem),
                           hipMemcpyHostToDevice, s));
  for (int z0 = 0; z0 < count; z0 += 64) {  // one launch per <= 64 sources, one wait for all
    const int cnt = std::min(64, count - z0);
    unsigned blocks = 0;
    for (int z = z0; z < z0 + cnt; ++z) blocks = std::max(blocks, aff_blocks(items[z].n));
    hipLaunchKernelGGL(k_ingest_affinity_group, dim3(blocks, cnt), dim3(256), 0, s,
                       static_cast<const AffIngestItem*>(table) + z0);
  }
  SC_TRY(check_last(h, "grouped affinity ingest launch"));
  if (host_flags)
    SC_HIP(h, hipMemcpyAsync(host_flags, flags, count * sizeof(int), hipMemcpyDeviceToHost, s));
  SC_HIP(h, hipStreamSynchronize(s));  // (`items`, `ones`, `packed` are locals)
  return SC_OK;
}

// ------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------
extern "C" int sc_array_layout(int* array_bytes, int* field_offsets) {
  if (array_bytes) *array_bytes = (int)sizeof(sc_array);
  if (field_offsets) {
    field_offsets[0] = (int)offsetof(sc_array, data);
    field_offsets[1] = (int)offsetof(sc_array, dtype);
    field_offsets[2] = (int)offsetof(sc_array, location);
    field_offsets[3] = (int)offsetof(sc_array, rows);
    field_offsets[4] = (int)offsetof(sc_array, cols);
    field_offsets[5] = (int)offsetof(sc_array, row_stride);
    field_offsets[6] = (int)offsetof(sc_array, col_stride);
  }
  return SC_OK;
}

extern "C" void* sc_stream(sc_handle h) { return h ? (void*)h->stream : nullptr; }

extern "C" int sc_set_embeddings_array(sc_handle h, const sc_array* x) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_array(h, x));
  SC_HIP(h, hipSetDevice(h->device));
  h->sweep_slot.clear();  // (eigenvectors of a sweep on the previous affinity)
  return ingest_embeddings(h, *x, true);
}

extern "C" int sc_set_embeddings(sc_handle h, const double* x, int n, int d) {
  if (!h) return SC_ERR_INVALID;
  if (!x || n <= 0 || d <= 0) return fail(h, SC_ERR_INVALID, "embeddings must be (n, d)");
  const sc_array a = host_f64_array(x, n, d);
  return sc_set_embeddings_array(h, &a);
}

extern "C" int sc_predict_array(sc_handle h, const sc_array* x, const sc_config* cfg,
                                int64_t* labels, sc_diag* diag) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_config(h, cfg));
  SC_TRY(sc_set_embeddings_array(h, x));
  return sc_run_resident(h, cfg, labels, diag);  // (the ingest is outside stage_ms: it is
                                                 // host-synchronous, time it on the host)
}

extern "C" int sc_predict(sc_handle h, const double* x, int n, int d, const sc_config* cfg,
                          int64_t* labels, sc_diag* diag) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_config(h, cfg));
  SC_TRY(sc_set_embeddings(h, x, n, d));
  return sc_run_resident(h, cfg, labels, diag);
}

extern "C" int sc_stage_ingest(sc_handle h, const sc_array* x, double* out) {
  if (!h) return SC_ERR_INVALID;
  if (!out) return fail(h, SC_ERR_INVALID, "out is NULL");
  SC_TRY(sc_set_embeddings_array(h, x));
  return d2h_matrix(h, ptr<double>(h->X), h->ldx, h->n, h->d, out);
}

extern "C" int sc_predict_batch_arrays(sc_handle h, const sc_array* xs, int count,
                                       const sc_config* cfg, int64_t* const* labels,
                                       sc_diag* diags, int group, int streams) {
  if (!h) return SC_ERR_INVALID;
  if (!xs || !labels || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  SC_TRY(validate_config(h, cfg));
  SC_HIP(h, hipSetDevice(h->device));
  bool device_source = false;
  std::vector<int> ns;
  int d = 0;
  SC_TRY(validate_batch_arrays(h, xs, count, &ns, &d, &device_source));
  if (count == 0) {
    h->last_routes.clear();
    return SC_OK;
  }
  // what the caller ordered before this handle's stream is done before any other stream of the
  // batch (pooled handles, lanes, banks, member arenas) reads a device source
  if (device_source) SC_HIP(h, hipStreamSynchronize(h->stream));
  if (group > 1)
    return predict_batch_grouped_impl(h, xs, ns.data(), d, count, cfg, labels, diags, group);
  return predict_batch_streams_impl(h, xs, ns.data(), d, count, cfg, labels, diags, streams);
}
