"""GPU: the way out alone (`sc_stage_egress`, csrc/egress.hip).  A host float64 matrix is uploaded
into a NaN-filled buffer at the library's pitch and written by the egress into a view inside a
larger tensor that was filled with a sentinel: inside the view every element is, bit for bit, the
narrowing rule of `_narrow_ref` (a NaN by position); outside it no byte has changed."""

import ctypes

import numpy as np
import pytest
# (at module level on purpose: PyTorch has to be in the process before the library is loaded,
#  so that both use one HIP runtime -- INTEGRATION.md section 6)
import torch

import _narrow_ref as nr

from spectralcluster_amd import _dlpack
from spectralcluster_amd import _lib

pytestmark = pytest.mark.gpu

# dtype name -> (integer type of the same width, its sentinel)
INT = {"float64": (torch.int64, 0x5A5A5A5A5A5A5A5A), "float32": (torch.int32, 0x5A5A5A5A),
       "float16": (torch.int16, 0x5A5A), "bfloat16": (torch.int16, 0x5A5A)}
FLOAT = {"float64": torch.float64, "float32": torch.float32, "float16": torch.float16,
         "bfloat16": torch.bfloat16}
# every size at which the 64 x 64 tile, the 16-byte item (2 / 4 / 8 elements) or the rounding of
# the pitch to 16 changes
SIZES = [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 191, 200]
EDGES = nr.edge_values()


def source(rows, cols):
  """The edge values tiled over the matrix, from a start that depends on the shape."""
  idx = (np.arange(rows * cols) + 7 * rows + cols) % EDGES.size
  return np.ascontiguousarray(EDGES[idx].reshape(rows, cols))


def destinations(rows, cols):
  """name -> (shape of the larger tensor, function that takes the (rows, cols) view of it; it is
  applied to the torch tensor and to its NumPy twin).  Row pitches are multiples of 16 elements
  and the aligned views begin 8 elements into a row: 16-byte aligned for every dtype."""
  r, c = rows, cols
  pr, pc = (r + 31) // 16 * 16, (c + 31) // 16 * 16
  return {
      "contiguous": ((r * c + 32,), lambda b: b[16:16 + r * c].reshape(r, c)),
      "pitched": ((r + 2, pc), lambda b: b[1:1 + r, 8:8 + c]),
      # the base one element further: the 16-byte form must not be taken
      "pitched_offset_1": ((r + 2, pc), lambda b: b[1:1 + r, 9:9 + c]),
      "transposed": ((c + 2, pr), lambda b: b[1:1 + c, 8:8 + r].T),
      "transposed_offset_1": ((c + 2, pr), lambda b: b[1:1 + c, 9:9 + r].T),
      "step_2_columns": ((r + 2, 2 * pc), lambda b: b[1:1 + r, 8:8 + 2 * c:2]),
      "step_2_rows": ((2 * r + 2, pc), lambda b: b[1:1 + 2 * r:2, 8:8 + c]),
      "step_2_both": ((2 * r + 2, 2 * pc), lambda b: b[1:1 + 2 * r:2, 8:8 + 2 * c:2]),
  }


def egress(handle, src, column_major, dest):
  desc = _dlpack.describe_out(dest, lambda: handle, src.shape)
  try:
    handle.check(handle.lib.sc_stage_egress(handle.raw, _lib.as_double_p(src), src.shape[0],
                                            src.shape[1], int(column_major),
                                            ctypes.byref(desc.array)))
  finally:
    desc.release()


def check_shape(handle, rows, cols, dtype, source_layouts):
  src = source(rows, cols)
  want = nr.narrow_bits(src, dtype)
  itype, sentinel = INT[dtype]
  for name, (shape, view) in destinations(rows, cols).items():
    for device in ("cuda", "cpu"):
      for column_major in source_layouts:
        big = torch.full(shape, sentinel, dtype=itype, device=device)
        dest = view(big.view(FLOAT[dtype]))
        assert tuple(dest.shape) == (rows, cols)
        egress(handle, src, column_major, dest)
        got = big.cpu().numpy().view(nr.BITS[dtype])
        what = "%s %s %dx%d column_major=%d -> %s" % (dtype, device, rows, cols, column_major, name)
        inside = view(got)
        nr.assert_same_bits(np.ascontiguousarray(inside), want, dtype, what)
        # outside the view: every byte as it was
        inside[...] = 0
        untouched = np.full(shape, sentinel, dtype=nr.BITS[dtype])
        view(untouched)[...] = 0
        assert np.array_equal(got, untouched), what + ": memory outside the view was written"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", nr.DTYPES)
def test_square_matrices_from_both_source_layouts_into_every_destination(handle, dtype, n):
  check_shape(handle, n, n, dtype, (0, 1))


@pytest.mark.parametrize("shape", [(129, 5), (200, 64)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dtype", nr.DTYPES)
def test_eigenvector_shapes_from_the_column_major_buffer(handle, dtype, shape):
  check_shape(handle, shape[0], shape[1], dtype, (1,))


def test_numpy_destinations_and_a_vector(handle):
  src = source(33, 17)
  for dtype in ("float64", "float32", "float16"):
    big = np.full((40, 64), -7.0, dtype=dtype)
    for view in (lambda b: b[2:35, 8:25], lambda b: b[8:25, 2:35].T, lambda b: b[2:35, 8:42:2]):
      big[...] = -7.0
      dest = view(big)
      egress(handle, src, 0, dest)
      nr.assert_same_bits(np.ascontiguousarray(dest).view(nr.BITS[dtype]),
                          nr.narrow_bits(src, dtype), dtype, dtype)
      dest[...] = -7.0
      assert (big == -7.0).all()
  # one row into a 1-D destination with a step: what the eigenvalues take
  row = source(1, 21)
  t = torch.full((50,), 3.0, dtype=torch.bfloat16, device="cuda")
  desc = _dlpack.describe_out(t[4:46:2], lambda: handle, (21,), "out values")
  handle.check(handle.lib.sc_stage_egress(handle.raw, _lib.as_double_p(row), 1, 21, 0,
                                          ctypes.byref(desc.array)))
  desc.release()
  got = t.cpu().view(torch.int16).numpy().view(np.uint16)
  nr.assert_same_bits(np.ascontiguousarray(got[4:46:2]), nr.narrow_bits(row[0], "bfloat16"),
                      "bfloat16", "vector")
  rest = np.ones(50, dtype=bool)
  rest[4:46:2] = False
  assert (got[rest] == np.uint16(0x4040)).all()  # 3.0


def test_descriptors_the_library_refuses(handle):
  lib = handle.lib
  src = source(8, 8)
  t = torch.zeros(8, 8, dtype=torch.float64, device="cuda")

  def call(**changes):
    arr = _lib.ScArray(t.data_ptr(), _lib.SC_DTYPE_F64, _lib.SC_MEM_DEVICE, 8, 8, 8, 1)
    for k, v in changes.items():
      setattr(arr, k, v)
    return lib.sc_stage_egress(handle.raw, _lib.as_double_p(src), 8, 8, 0, ctypes.byref(arr))

  assert call() == _lib.SC_OK
  nr.assert_same_bits(t.cpu().numpy().view(np.uint64), src.view(np.uint64), "float64", "good")
  t.zero_()
  torch.cuda.synchronize()
  for bad in (dict(rows=7), dict(cols=9), dict(dtype=9), dict(location=5), dict(row_stride=-8),
              dict(col_stride=-1), dict(row_stride=0), dict(row_stride=7), dict(col_stride=0),
              dict(row_stride=1, col_stride=7), dict(data=None),
              dict(data=src.ctypes.data)):  # host memory called device memory
    assert call(**bad) == _lib.SC_ERR_INVALID, bad
    assert "out" in handle.last_error()
  assert (t.cpu() == 0).all()  # ... and none of them wrote
