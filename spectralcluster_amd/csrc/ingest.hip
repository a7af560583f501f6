// Embeddings come in where they are: a described array (sc_array: device or host memory, fp64 /
// fp32 / fp16 / bf16, any element strides) is widened into the handle's fp64 X buffer.
//   device source        k_ingest_rows reads it in place on the call's stream,
//   host fp64            the hipMemcpy2DAsync the double* entry points have always issued,
//   host fp32/fp16/bf16  copied at their own width into a staging buffer of the handle (a half
//                        or a quarter of the fp64 bytes over the link), then the same kernel.
// All arithmetic after this stays fp64, and widening is exact for every bit pattern, so results
// are bit for bit those of the values converted to double on the host.
#include <climits>
#include <cstddef>

#include "handle.h"

namespace {

// ---- exact widening ---------------------------------------------------------------------
struct F16Bits { unsigned short v; };
struct BF16Bits { unsigned short v; };

__device__ __forceinline__ double widen(double v) { return v; }
__device__ __forceinline__ double widen(float v) { return (double)v; }
// bf16 is the upper half of an fp32: place the bits, widen the fp32
__device__ __forceinline__ double widen(BF16Bits b) {
  return (double)__uint_as_float((unsigned)b.v << 16);
}
// fp16 by bits (no dependence on the fp16 denormal mode): normal numbers move exponent and
// mantissa into the fp64 fields, subnormals are mantissa * 2^-24 (an exact integer conversion
// and an exact scaling), exponent 31 becomes exponent 2047 with the payload kept
__device__ __forceinline__ double widen(F16Bits b) {
  const unsigned h = b.v;
  const unsigned long long sign = (unsigned long long)(h >> 15) << 63;
  const unsigned e = (h >> 10) & 31u, m = h & 1023u;
  unsigned long long bits;
  if (e == 31u) {
    bits = sign | (0x7ffull << 52) | ((unsigned long long)m << 42);
  } else if (e != 0u) {
    bits = sign | ((unsigned long long)(e + 1008u) << 52) | ((unsigned long long)m << 42);
  } else {
    bits = sign | (unsigned long long)__double_as_longlong((double)(int)m * 0x1p-24);
  }
  return __longlong_as_double((long long)bits);
}

// 16 bytes of source as one load
template <typename T>
struct alignas(16) Chunk {
  T v[16 / sizeof(T)];
};

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
  const bool fast = col_stride == 1 && (reinterpret_cast<uintptr_t>(src) & 15u) == 0 &&
                    (n == 1 || (row_stride * (long long)sizeof(T)) % 16 == 0);
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
  switch (dtype) {
    case SC_DTYPE_F64: launch_ingest_typed<double>(s, src, row_stride, col_stride, n, d, X, ldx); break;
    case SC_DTYPE_F32: launch_ingest_typed<float>(s, src, row_stride, col_stride, n, d, X, ldx); break;
    case SC_DTYPE_F16: launch_ingest_typed<F16Bits>(s, src, row_stride, col_stride, n, d, X, ldx); break;
    default: launch_ingest_typed<BF16Bits>(s, src, row_stride, col_stride, n, d, X, ldx); break;
  }
}

size_t dtype_bytes(int dtype) {
  return dtype == SC_DTYPE_F64 ? 8 : dtype == SC_DTYPE_F32 ? 4 : 2;
}

// Host rows that hipMemcpy2D cannot describe (a column stride, rows that overlap): gathered
// into `tmp` at the source's width.
void pack_host_rows(const sc_array& a, std::vector<unsigned char>* tmp) {
  const size_t eb = dtype_bytes(a.dtype);
  tmp->resize((size_t)a.rows * a.cols * eb);
  const unsigned char* base = static_cast<const unsigned char*>(a.data);
  unsigned char* out = tmp->data();
  for (int64_t r = 0; r < a.rows; ++r)
    for (int64_t c = 0; c < a.cols; ++c, out += eb)
      memcpy(out, base + (size_t)(r * a.row_stride + c * a.col_stride) * eb, eb);
}

}  // namespace

// ------------------------------------------------------------------------------
// validation (no launch, no copy)
// ------------------------------------------------------------------------------
int validate_array(sc_handle h, const sc_array* a) {
  if (!a) return fail(h, SC_ERR_INVALID, "embeddings descriptor is NULL");
  if (!a->data || a->rows <= 0 || a->cols <= 0)
    return fail(h, SC_ERR_INVALID, "embeddings must be (n, d)");
  if (a->rows > INT_MAX || a->cols > INT_MAX)
    return fail(h, SC_ERR_INVALID, "embeddings: rows and cols must fit an int");
  if (a->dtype < SC_DTYPE_F64 || a->dtype > SC_DTYPE_BF16)
    return fail(h, SC_ERR_INVALID, "embeddings: unknown dtype (SC_DTYPE_F64 / F32 / F16 / BF16)");
  if (a->location != SC_MEM_HOST && a->location != SC_MEM_DEVICE)
    return fail(h, SC_ERR_INVALID, "embeddings: unknown location (SC_MEM_HOST / SC_MEM_DEVICE)");
  if (a->row_stride < 0 || a->col_stride < 0)
    return fail(h, SC_ERR_INVALID, "embeddings: strides must not be negative");
  if (a->location == SC_MEM_DEVICE) {
    hipPointerAttribute_t attr;
    memset(&attr, 0, sizeof(attr));
    const hipError_t e = hipPointerGetAttributes(&attr, a->data);
    if (e != hipSuccess) (void)hipGetLastError();  // (the failed query is sticky otherwise)
    if (e != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != h->device)
      return fail(h, SC_ERR_INVALID,
                  "embeddings: location is SC_MEM_DEVICE but the pointer is not device memory of "
                  "the handle's device");
  }
  return SC_OK;
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
                     bool* sync_out) {
  const int n = (int)a.rows, d = (int)a.cols;
  bool sync = false;
  const size_t eb = dtype_bytes(a.dtype);
  if (a.location == SC_MEM_DEVICE) {
    launch_ingest_rows(s, a.dtype, a.data, a.row_stride, a.col_stride, n, d, X, ldx);
    SC_TRY(check_last(h, "ingest launch"));
  } else {
    std::vector<unsigned char> packed;
    const void* src = a.data;
    size_t spitch = (size_t)a.row_stride * eb;
    if (a.col_stride != 1 || (a.row_stride < a.cols && n > 1)) {
      pack_host_rows(a, &packed);
      src = packed.data();
      spitch = (size_t)d * eb;
      sync = true;  // (`packed` is a local)
    }
    if (n == 1) spitch = (size_t)d * eb;
    if (a.dtype == SC_DTYPE_F64) {
      SC_HIP(h, hipMemcpy2DAsync(X, (size_t)ldx * sizeof(double), src, spitch,
                                 (size_t)d * sizeof(double), n, hipMemcpyHostToDevice, s));
    } else {
      // staging rows on a 16-byte pitch (the kernel's wide loads); sized with the X buffer, so
      // an arena reserved for the largest member of a batch allocates it once
      const size_t pitch = ((size_t)d * eb + 15) / 16 * 16;
      const size_t need = std::max((size_t)n * pitch, h->X.bytes / sizeof(double) * eb);
      if (h->Xstage.bytes < need) {
        if (h->Xstage.p && s != h->stream) SC_HIP(h, hipStreamSynchronize(s));
        SC_TRY(grow(h, h->Xstage, need));
      }
      SC_HIP(h, hipMemcpy2DAsync(h->Xstage.p, pitch, src, spitch, (size_t)d * eb, n,
                                 hipMemcpyHostToDevice, s));
      launch_ingest_rows(s, a.dtype, h->Xstage.p, (long long)(pitch / eb), 1, n, d, X, ldx);
      SC_TRY(check_last(h, "ingest launch"));
    }
  }
  if (sync) *sync_out = true;
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
