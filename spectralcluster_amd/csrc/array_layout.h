// The rules every reader and writer of caller memory shares (ingest.hip: caller memory -> the
// handle's fp64 buffers; egress.hip: the way back; centroids.hip: both), each written once:
//   dispatch_dtype      an sc_array dtype -> its element type (the 2-byte types are bits),
//   Chunk / aligned16   the 16-byte item and the rule that says when an access may be one,
//   align16             sizes and pitches of staging memory,
//   aff_at              the 64 x 64 LDS tile with its swizzle,
//   widen / narrow      the exact widening and the narrowing by bits,
//   runs_along_columns  which way a view's memory runs.
#ifndef SC_ARRAY_LAYOUT_H_
#define SC_ARRAY_LAYOUT_H_

#include <climits>
#include <cstddef>
#include <cstdint>

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

// f(T{}) for the element type T of one of the four float dtypes (a validated descriptor has no
// other): `[&](auto t) { using T = decltype(t); ... }`
template <typename F>
__host__ __device__ __forceinline__ void dispatch_dtype(int dtype, F&& f) {
  switch (dtype) {
    case SC_DTYPE_F64: f(double{}); break;
    case SC_DTYPE_F32: f(float{}); break;
    case SC_DTYPE_F16: f(F16Bits{}); break;
    default: f(BF16Bits{}); break;
  }
}

// May the lines of a view (unit stride along a line, `pitch_elems` from one line to the next) be
// read or written 16 bytes at a time?  The base address is a multiple of 16 and so is the pitch in
// bytes -- or there is one line only, whose pitch addresses nothing.
inline bool aligned16(const void* p, long long pitch_elems, size_t elem_bytes, long long lines) {
  return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 &&
         (lines == 1 || (pitch_elems * (long long)elem_bytes) % 16 == 0);
}

// sizes and pitches of staging memory: the next multiple of 16 bytes
inline size_t align16(size_t bytes) { return (bytes + 15) / 16 * 16; }

// LDS rows of a tile are not padded (two fp64 tiles are the whole 64 KB): the pair index of a row
// is XOR-ed with the row number instead, which keeps 16-byte pairs together and spreads a column
// over all banks.
constexpr int kAffTile = 64;
__device__ __forceinline__ int aff_at(int r, int c) {
  return r * kAffTile + (c ^ ((r & 31) << 1));
}

// ---- exact widening ---------------------------------------------------------------------
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

// ---- narrowing by bits --------------------------------------------------------------------
__device__ __forceinline__ unsigned f64_to_f32_bits(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned sign = (unsigned)(b >> 32) & 0x80000000u;
  const unsigned long long a = b & 0x7fffffffffffffffull;
  if (a >= 0x7ff0000000000000ull) return sign | (a > 0x7ff0000000000000ull ? 0x7fc00000u : 0x7f800000u);
  const int e = (int)(a >> 52);  // biased by 1023; the fp32 exponent field is e - 896
  const unsigned long long m = a & 0xfffffffffffffull;
  if (e >= 897) {
    if (e - 896 >= 255) return sign | 0x7f800000u;
    // exponent and the upper 23 mantissa bits; a carry of the rounding runs into the exponent
    // (up to infinity) as it should
    unsigned r = ((unsigned)(e - 896) << 23) | (unsigned)(m >> 29);
    const unsigned rem = (unsigned)m & 0x1fffffffu;
    if (rem > 0x10000000u || (rem == 0x10000000u && (r & 1u))) ++r;
    return sign | r;
  }
  // a subnormal fp32 (units of 2^-149) or zero: (2^52 + m) * 2^(e - 1075) / 2^-149
  const int s = 926 - e;
  if (e == 0 || s > 63) return sign;
  const unsigned long long M = (1ull << 52) | m;
  unsigned r = (unsigned)(M >> s);
  const unsigned long long rem = M & ((1ull << s) - 1ull), half = 1ull << (s - 1);
  if (rem > half || (rem == half && (r & 1u))) ++r;
  return sign | r;
}

__device__ __forceinline__ unsigned short f32_bits_to_f16_bits(unsigned f) {
  const unsigned sign = (f >> 16) & 0x8000u, a = f & 0x7fffffffu;
  if (a >= 0x7f800000u) return (unsigned short)(sign | (a > 0x7f800000u ? 0x7e00u : 0x7c00u));
  const int e = (int)(a >> 23);  // biased by 127; the fp16 exponent field is e - 112
  const unsigned m = a & 0x7fffffu;
  if (e >= 113) {
    if (e - 112 >= 31) return (unsigned short)(sign | 0x7c00u);
    unsigned r = ((unsigned)(e - 112) << 10) | (m >> 13);
    const unsigned rem = m & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) ++r;  // (65520 -> 0x7c00, infinity)
    return (unsigned short)(sign | r);
  }
  // a subnormal fp16 (units of 2^-24) or zero: (2^23 + m) * 2^(e - 150) / 2^-24
  const int s = 126 - e;
  if (e == 0 || s > 31) return (unsigned short)sign;
  const unsigned M = (1u << 23) | m;
  unsigned r = M >> s;
  const unsigned rem = M & ((1u << s) - 1u), half = 1u << (s - 1);
  if (rem > half || (rem == half && (r & 1u))) ++r;
  return (unsigned short)(sign | r);
}

__device__ __forceinline__ unsigned short f32_bits_to_bf16_bits(unsigned f) {
  if ((f & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((f >> 16) | 0x0040u);
  return (unsigned short)((f + 0x7fffu + ((f >> 16) & 1u)) >> 16);
}

template <typename T>
__device__ __forceinline__ T narrow(double v);
template <>
__device__ __forceinline__ double narrow<double>(double v) { return v; }
template <>
__device__ __forceinline__ float narrow<float>(double v) {
  return __uint_as_float(f64_to_f32_bits(v));
}
template <>
__device__ __forceinline__ F16Bits narrow<F16Bits>(double v) {
  return F16Bits{f32_bits_to_f16_bits(f64_to_f32_bits(v))};
}
template <>
__device__ __forceinline__ BF16Bits narrow<BF16Bits>(double v) {
  return BF16Bits{f32_bits_to_bf16_bits(f64_to_f32_bits(v))};
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
