// What the ingest (ingest.hip: caller memory -> the handle's fp64 buffers) and the egress
// (egress.hip: the way back) share: the 2-byte element types as bits, the 16-byte item, the
// 64 x 64 LDS tile with its swizzle, and the rule that says which way a view's memory runs.
#ifndef SC_ARRAY_LAYOUT_H_
#define SC_ARRAY_LAYOUT_H_

#include <climits>
#include <cstddef>

#include <hip/hip_runtime.h>

#include "../../include/spectralcluster_amd.h"

namespace {

struct F16Bits { unsigned short v; };
struct BF16Bits { unsigned short v; };

// 16 bytes of caller memory as one access
template <typename T>
struct alignas(16) Chunk {
  T v[16 / sizeof(T)];
};

inline size_t dtype_bytes(int dtype) {
  return dtype == SC_DTYPE_F64 ? 8 : dtype == SC_DTYPE_F32 ? 4 : 2;
}

// LDS rows of a tile are not padded (two fp64 tiles are the whole 64 KB): the pair index of a row
// is XOR-ed with the row number instead, which keeps 16-byte pairs together and spreads a column
// over all banks.
constexpr int kAffTile = 64;
__device__ __forceinline__ int aff_at(int r, int c) {
  return r * kAffTile + (c ^ ((r & 31) << 1));
}

// the direction of the memory: the smaller stride (a zero stride repeats one element, it walks
// nothing)
inline long long walked(long long stride) { return stride == 0 ? LLONG_MAX : stride; }
inline bool runs_along_columns(long long row_stride, long long col_stride, int dim) {
  const long long r = walked(row_stride), c = walked(col_stride);
  return r < c || (r == c && dim == 1);
}

}  // namespace

#endif  // SC_ARRAY_LAYOUT_H_
