"""The narrowing rule of the egress (csrc/egress.hip) as NumPy bit arithmetic: float64 -> float32
round to nearest even, then float32 -> float16 / bfloat16 round to nearest even -- what PyTorch's
CPU `tensor.to(dtype)` computes.  Results are returned as BITS (uint32 / uint16; float64 as
uint64), so that signed zeros, subnormals and infinities are compared exactly; a NaN is any
pattern `is_nan_bits` accepts (its payload is not specified)."""

import numpy as np

DTYPES = ("float64", "float32", "float16", "bfloat16")
BITS = {"float64": np.uint64, "float32": np.uint32, "float16": np.uint16, "bfloat16": np.uint16}


def f64_to_f32_bits(x: np.ndarray) -> np.ndarray:
  b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
  sign = ((b >> np.uint64(32)) & np.uint64(0x80000000)).astype(np.uint32)
  a = b & np.uint64(0x7fffffffffffffff)
  e = (a >> np.uint64(52)).astype(np.int64)
  m = a & np.uint64(0xfffffffffffff)
  # normal results: exponent field e - 896, upper 23 mantissa bits, the carry runs into the exponent
  en = np.clip(e - 896, 1, 254).astype(np.uint64)
  r = (en << np.uint64(23)) | (m >> np.uint64(29))
  rem = m & np.uint64(0x1fffffff)
  up = (rem > np.uint64(0x10000000)) | ((rem == np.uint64(0x10000000)) & ((r & np.uint64(1)) == 1))
  normal = (r + up.astype(np.uint64)).astype(np.uint32)
  # subnormal results in units of 2^-149: (2^52 + m) >> (926 - e)
  s = np.clip(926 - e, 1, 63).astype(np.uint64)
  big = np.uint64(1 << 52) | m
  q = big >> s
  rem = big & ((np.uint64(1) << s) - np.uint64(1))
  half = np.uint64(1) << (s - np.uint64(1))
  up = (rem > half) | ((rem == half) & ((q & np.uint64(1)) == 1))
  sub = (q + up.astype(np.uint64)).astype(np.uint32)
  sub = np.where((e == 0) | (926 - e > 63), np.uint32(0), sub)
  out = np.where(e >= 897, normal, sub)
  out = np.where(e - 896 >= 255, np.uint32(0x7f800000), out)
  out = np.where(a > np.uint64(0x7ff0000000000000), np.uint32(0x7fc00000), out)
  return (sign | out).astype(np.uint32)


def f32_bits_to_f16_bits(f: np.ndarray) -> np.ndarray:
  f = f.astype(np.uint32)
  sign = (f >> np.uint32(16)) & np.uint32(0x8000)
  a = f & np.uint32(0x7fffffff)
  e = (a >> np.uint32(23)).astype(np.int64)
  m = a & np.uint32(0x7fffff)
  en = np.clip(e - 112, 1, 30).astype(np.uint32)
  r = (en << np.uint32(10)) | (m >> np.uint32(13))
  rem = m & np.uint32(0x1fff)
  up = (rem > np.uint32(0x1000)) | ((rem == np.uint32(0x1000)) & ((r & np.uint32(1)) == 1))
  normal = r + up.astype(np.uint32)
  s = np.clip(126 - e, 1, 31).astype(np.uint32)
  big = np.uint32(1 << 23) | m
  q = big >> s
  rem = big & ((np.uint32(1) << s) - np.uint32(1))
  half = np.uint32(1) << (s - np.uint32(1))
  up = (rem > half) | ((rem == half) & ((q & np.uint32(1)) == 1))
  sub = q + up.astype(np.uint32)
  sub = np.where((e == 0) | (126 - e > 31), np.uint32(0), sub)
  out = np.where(e >= 113, normal, sub)
  out = np.where(e - 112 >= 31, np.uint32(0x7c00), out)
  out = np.where(a > np.uint32(0x7f800000), np.uint32(0x7e00), out)
  return (sign | out).astype(np.uint16)


def f32_bits_to_bf16_bits(f: np.ndarray) -> np.ndarray:
  f = f.astype(np.uint64)  # (room for the carry out of bit 31)
  rounded = (f + np.uint64(0x7fff) + ((f >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
  nan = (f & np.uint64(0x7fffffff)) > np.uint64(0x7f800000)
  return np.where(nan, (f >> np.uint64(16)) | np.uint64(0x40), rounded).astype(np.uint16)


def narrow_bits(x: np.ndarray, dtype: str) -> np.ndarray:
  """The bits of `x` (float64 values) narrowed to `dtype`, in x's shape."""
  x = np.ascontiguousarray(x, dtype=np.float64)
  if dtype == "float64":
    return x.view(np.uint64).copy()
  f = f64_to_f32_bits(x.ravel())
  if dtype == "float16":
    f = f32_bits_to_f16_bits(f)
  elif dtype == "bfloat16":
    f = f32_bits_to_bf16_bits(f)
  else:
    assert dtype == "float32", dtype
  return f.reshape(x.shape)


def is_nan_bits(bits: np.ndarray, dtype: str) -> np.ndarray:
  if dtype == "float64":
    return (bits & np.uint64(0x7fffffffffffffff)) > np.uint64(0x7ff0000000000000)
  if dtype == "float32":
    return (bits & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
  inf = np.uint16(0x7c00 if dtype == "float16" else 0x7f80)
  return (bits & np.uint16(0x7fff)) > inf


def assert_same_bits(got: np.ndarray, want: np.ndarray, dtype: str, what: str = "") -> None:
  """Bit for bit, a NaN by position."""
  assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
  gn, wn = is_nan_bits(got, dtype), is_nan_bits(want, dtype)
  assert np.array_equal(gn, wn), "%s: NaNs at different positions" % what
  bad = (got != want) & ~wn
  if bad.any():
    at = tuple(int(i[0]) for i in np.nonzero(bad))
    raise AssertionError("%s: %d of %d elements differ, first at %s: got 0x%x, want 0x%x"
                         % (what, int(bad.sum()), bad.size, at, int(got[at]), int(want[at])))


def edge_values() -> np.ndarray:
  """Where the narrowing can go wrong: values half an fp16 / bf16 / fp32 ulp from a representable
  number, +- 2^-40 relative (double rounding and direct rounding part here), the overflow
  thresholds, subnormal results of all three widths, the largest finite values, signed zeros,
  infinities and NaN."""
  v = []
  for base in (1.0, 1.5, 1023.0, 0.333251953125, 2.0 ** -14, 3.0 * 2.0 ** -16):
    for ulp_bits in (10, 7, 23):  # mantissa bits of fp16, bf16, fp32
      ulp = 2.0 ** (np.floor(np.log2(base)) - ulp_bits)
      for k in (0.5, 1.5):
        for eps in (0.0, 2.0 ** -40, -2.0 ** -40):
          v.append(base + k * ulp + eps * base)
  # an fp16 tie that only exists after the fp32 rounding: 1 + 2^-11 + 2^-30 rounds to fp32
  # 1 + 2^-11 (a tie, to even: 1.0) while direct rounding gives 1 + 2^-10
  v += [1.0 + 2.0 ** -11 + 2.0 ** -30, 1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 3 * 2.0 ** -11 - 2.0 ** -30]
  v += [np.nextafter(65520.0, 0.0), 65520.0, 65519.0, 65504.0, 65536.0,
        float(np.finfo(np.float32).max), float(np.finfo(np.float32).max) * (1 + 2.0 ** -25),
        float(np.finfo(np.float32).max) * (1 + 2.0 ** -24), 3.3895313892515355e38, 3.4e38, 1e39,
        float(np.finfo(np.float64).max)]
  # subnormal results: fp16 (< 2^-14), bf16 / fp32 (< 2^-126), halves and ties among them
  for p in (-15, -20, -24, -25, -26, -126, -127, -130, -133, -134, -140, -149, -150, -151, -1000,
            -1074):
    for mant in (1.0, 1.5, 1.25, 1.75, 1.0 + 2.0 ** -30):
      v.append(mant * 2.0 ** p if p > -1074 else 5e-324)
  v += [0.0, np.inf, np.nan, 1e-320]
  v = np.array(v, dtype=np.float64)
  return np.concatenate([v, -v])
