"""The narrowing rule the egress kernels are held to (`_narrow_ref`) is, bit for bit, PyTorch's CPU
`tensor.to(float32 / float16 / bfloat16)` of a float64 tensor: fp64 -> fp32 round to nearest even,
then fp32 -> the 16-bit type round to nearest even (NOT NumPy's direct float64 -> float16)."""

import numpy as np
import pytest
import torch

import _narrow_ref as nr

TORCH = {"float32": (torch.float32, torch.int32, np.uint32),
         "float16": (torch.float16, torch.int16, np.uint16),
         "bfloat16": (torch.bfloat16, torch.int16, np.uint16)}


def torch_bits(x: np.ndarray, dtype: str) -> np.ndarray:
  tdtype, idtype, udtype = TORCH[dtype]
  t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(tdtype)
  return t.view(idtype).numpy().view(udtype)


def random_doubles() -> np.ndarray:
  rng = np.random.default_rng(20240611)
  # every exponent the three formats can reach and some beyond, random mantissas and signs
  mant = rng.uniform(1.0, 2.0, 100000)
  expo = rng.integers(-160, 132, 100000)
  sign = rng.choice([-1.0, 1.0], 100000)
  x = sign * mant * np.exp2(expo.astype(np.float64))
  x[:20000] = rng.standard_normal(20000)  # and the everyday range
  return x


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_random_doubles_narrow_as_torch_narrows_them(dtype):
  x = random_doubles()
  nr.assert_same_bits(nr.narrow_bits(x, dtype), torch_bits(x, dtype), dtype, dtype)


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_constructed_edges_narrow_as_torch_narrows_them(dtype):
  x = nr.edge_values()
  got, want = nr.narrow_bits(x, dtype), torch_bits(x, dtype)
  nr.assert_same_bits(got, want, dtype, dtype)
  # NaN by position, and it is a NaN of the target type
  assert np.array_equal(nr.is_nan_bits(got, dtype), np.isnan(x))


def test_the_edges_are_the_ones_that_matter():
  x = nr.edge_values()
  h = nr.narrow_bits(x, "float16").view(np.float16)
  # 65520 overflows; so does the double just below it (fp32 rounds it up to 65520 first: direct
  # rounding would give 65504), 65519 does not; signed zeros survive
  assert h[x == 65520.0] == np.inf and h[x == np.nextafter(65520.0, 0.0)] == np.inf
  assert h[x == 65519.0] == np.float16(65504.0)
  assert np.signbit(h[(x == 0.0) & np.signbit(x)]).all()
  # double rounding and direct rounding part somewhere in the set, and the rule is the double one
  with np.errstate(over="ignore"):
    direct = x.astype(np.float16)
    twice = x.astype(np.float32).astype(np.float16)
  finite = np.isfinite(x)
  assert (direct[finite] != twice[finite]).any()
  assert np.array_equal(h[finite].view(np.uint16), twice[finite].view(np.uint16))
  # subnormal results of all three widths occur
  f = nr.narrow_bits(x, "float32")
  b = nr.narrow_bits(x, "bfloat16")
  assert (((f & 0x7f800000) == 0) & ((f & 0x7fffff) != 0)).any()
  assert (((b & 0x7f80) == 0) & ((b & 0x7f) != 0)).any()
  assert (((h.view(np.uint16) & 0x7c00) == 0) & ((h.view(np.uint16) & 0x3ff) != 0)).any()


def test_float64_is_a_copy_of_the_bits():
  x = nr.edge_values()
  assert np.array_equal(nr.narrow_bits(x, "float64"), x.view(np.uint64))
