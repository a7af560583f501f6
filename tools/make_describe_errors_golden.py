"""What `_dlpack` answers for a grid of acceptable and unacceptable objects, per role (embeddings,
strided input, `out` 1-D and 2-D, labels in, labels out): the exception type and full message, or
the seven `sc_array` fields with the data pointer relative to the object's base address.

  python tools/make_describe_errors_golden.py     writes tests/golden/describe_errors.json

tests/test_stage_device_host.py replays `CASES` against that file, so a change of `_dlpack` that
moves a check, a message or a described field shows as a difference.  Needs no GPU: objects that
say they live on one are fakes around a host twin.
"""

import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from spectralcluster_amd import _dlpack  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "describe_errors.json")
as_strided = np.lib.stride_tricks.as_strided


class Handle:
  """Stands in for the library handle of device 0."""
  device = 0

  def stream(self):
    return 0


def get_handle():
  return Handle()


class Fake:
  """A DLPack object around a host twin (ndarray or tensor) that reports `device`; `error`: what
  `__dlpack__` raises; `name`: the capsule's name when it is not "dltensor"; `strides`: element
  strides written over the capsule's."""

  def __init__(self, host, device=(_dlpack.KDL_ROCM, 0), error=None, name=None, strides=None):
    self.host = torch.from_numpy(host) if isinstance(host, np.ndarray) else host
    self.device, self.error, self.name, self.strides = device, error, name, strides

  def __dlpack_device__(self):
    return self.device

  def __dlpack__(self, stream=None):
    if self.error is not None:
      raise self.error
    capsule = self.host.__dlpack__()
    address = _dlpack._get_pointer(capsule, _dlpack._NAME)
    managed = ctypes.cast(address, ctypes.POINTER(_dlpack.DLManagedTensor))
    for i, s in enumerate(self.strides or ()):
      managed.contents.dl_tensor.strides[i] = s
    if self.name is not None:
      _dlpack._set_name(capsule, self.name)
    return capsule


class NoDlpack:
  shape = (4, 4)


def read_only(shape, dtype=np.float64):
  a = np.zeros(shape, dtype=dtype)
  a.flags.writeable = False
  return a


def bytes_view(dtype, count):
  """`count` elements of `dtype` one byte off their alignment: a stride of 2 * itemsize + 1."""
  item = np.dtype(dtype).itemsize
  raw = np.zeros((2 * item + 1) * count + item, dtype=np.uint8)
  return as_strided(raw[:item].view(dtype), (count,), (2 * item + 1,)), raw


# role -> the call; every role's objects below are sized for it
ROLES = {
    "embeddings": lambda o: _dlpack.describe(o, get_handle),
    "strided": lambda o: _dlpack.describe_input(o, get_handle),
    "out2d": lambda o: _dlpack.describe_out(o, get_handle, (4, 4)),
    "out1d": lambda o: _dlpack.describe_out(o, get_handle, (5,), "out values"),
    "labels_in": lambda o: _dlpack.describe_labels(o, get_handle, 6, "labels of member 1"),
    "labels_out": lambda o: _dlpack.describe_labels_out(o, get_handle, 6),
}


def matrix_objects(dtype_ok, dtype_bad):
  """(name, maker) for the 2-D roles: a (4, 4) matrix is what `out2d` expects."""
  z = lambda *shape, dtype=dtype_ok: np.zeros(shape, dtype=dtype)
  return [
      ("contiguous", lambda: z(4, 4)),
      ("float32", lambda: z(4, 4, dtype=np.float32)),
      ("float16", lambda: z(4, 4, dtype=np.float16)),
      ("interior view", lambda: z(8, 8)[2:6, 1:5]),
      ("transposed", lambda: z(4, 6)[:, :4].T),
      ("step 2 in both", lambda: z(8, 8)[::2, ::2]),
      ("one row", lambda: z(4, 4)[1:2]),
      ("wrong ndim", lambda: z(16)),
      ("three dimensions", lambda: z(4, 4, 1)),
      ("wrong shape", lambda: z(4, 5)),
      ("a dtype that is not taken", lambda: z(4, 4, dtype=dtype_bad)),
      ("longdouble", lambda: z(4, 4, dtype=np.longdouble)),
      ("read-only", lambda: read_only((4, 4))),
      ("negative row stride", lambda: z(4, 4)[::-1]),
      ("negative column stride", lambda: z(4, 4)[:, ::-1]),
      ("stride no multiple of the item size",
       lambda: as_strided(np.zeros(200, dtype=np.uint8)[:8].view(np.float64), (4, 4), (36, 9))),
      ("zero row stride", lambda: as_strided(z(4), (4, 4), (0, 8))),
      ("overlapping rows", lambda: as_strided(z(16), (4, 4), (16, 8))),
      ("a list", lambda: [[0.0] * 4] * 4),
      ("no __dlpack__", NoDlpack),
      ("host tensor", lambda: torch.zeros(4, 4, dtype=torch.float32)),
      ("bfloat16 tensor", lambda: torch.zeros(4, 4, dtype=torch.bfloat16)),
      ("transposed tensor", lambda: torch.zeros(4, 6)[:, :4].t()),
      ("integer tensor", lambda: torch.zeros(4, 4, dtype=torch.int64)),
      ("1-D tensor", lambda: torch.zeros(16)),
      ("tensor of the wrong shape", lambda: torch.zeros(4, 3)),
      ("expanded tensor", lambda: torch.zeros(1, 4).expand(4, 4)),
      ("tensor that needs grad", lambda: torch.zeros(4, 4, requires_grad=True)),
      ("fake on the device", lambda: Fake(z(4, 4))),
      ("fake on the device as CUDA", lambda: Fake(z(4, 4), (_dlpack.KDL_CUDA, 0))),
      ("fake in pinned host memory", lambda: Fake(z(4, 4), (_dlpack.KDL_ROCM_HOST, 0))),
      ("fake on a foreign device type", lambda: Fake(z(4, 4), (7, 0))),
      ("fake on device 1", lambda: Fake(z(4, 4), (_dlpack.KDL_ROCM, 1))),
      ("fake that raises BufferError", lambda: Fake(z(4, 4), error=BufferError("not exportable"))),
      ("fake host that raises BufferError",
       lambda: Fake(z(4, 4), (_dlpack.KDL_CPU, 0), error=BufferError("not exportable"))),
      ("fake with a capsule of the wrong name", lambda: Fake(z(4, 4), name=_dlpack._USED_NAME)),
      ("fake with a negative stride", lambda: Fake(z(4, 4), strides=(-4, 1))),
      # two rules at once: which one answers
      ("read-only and a dtype that is not taken", lambda: read_only((4, 4), dtype_bad)),
      ("a dtype that is not taken and the wrong shape", lambda: z(4, 5, dtype=dtype_bad)),
      ("wrong shape and a negative stride", lambda: z(4, 5)[::-1]),
      ("negative stride and not injective", lambda: as_strided(z(16)[12:], (4, 4), (-8, 8))),
      ("fake: foreign device type and device 1", lambda: Fake(z(4, 4), (7, 1))),
      ("fake: device 1 and BufferError",
       lambda: Fake(z(4, 4), (_dlpack.KDL_ROCM, 1), error=BufferError("not exportable"))),
      ("fake: wrong ndim and a dtype that is not taken", lambda: Fake(z(16, dtype=dtype_bad))),
      ("fake: a dtype that is not taken and a negative stride",
       lambda: Fake(z(4, 4, dtype=dtype_bad), strides=(-4, 1))),
      ("fake: wrong shape and not injective", lambda: Fake(torch.zeros(1, 5).expand(4, 5))),
  ]


def vector_objects(count, dtype_ok, dtype_bad):
  """(name, maker) for the 1-D roles: `count` entries is what the role expects."""
  z = lambda n, dtype=dtype_ok: np.zeros(n, dtype=dtype)
  return [
      ("contiguous", lambda: z(count)),
      ("int32 or float32", lambda: z(count, np.int32 if dtype_ok == np.int64 else np.float32)),
      ("step 2", lambda: z(2 * count)[::2]),
      ("one entry too few", lambda: z(count - 1)),
      ("wrong ndim", lambda: z(count).reshape(1, count)),
      ("a dtype that is not taken", lambda: z(count, dtype_bad)),
      ("float64", lambda: z(count, np.float64)),
      ("float64 that is not integral", lambda: z(count, np.float64) + 0.5),
      ("float32 with an infinity", lambda: np.full(count, np.inf, dtype=np.float32)),
      ("int16", lambda: z(count, np.int16)),
      ("uint64 above the largest label", lambda: np.full(count, 2**40, dtype=np.uint64)),
      ("int64 above the largest label", lambda: np.full(count, 2**31 - 1, dtype=np.int64)),
      ("bool", lambda: z(count, np.bool_)),
      ("complex", lambda: z(count, np.complex128)),
      ("read-only", lambda: read_only(count, dtype_ok)),
      ("negative stride", lambda: z(2 * count)[::-2]),
      ("stride no multiple of the item size", lambda: bytes_view(dtype_ok, count)[0]),
      ("zero stride", lambda: as_strided(z(1), (count,), (0,))),
      ("a list", lambda: [0] * count),
      ("a list of the wrong length", lambda: [0] * (count + 1)),
      ("no __dlpack__", NoDlpack),
      ("host tensor", lambda: torch.zeros(count, dtype=torch.from_numpy(z(1)).dtype)),
      ("strided tensor", lambda: torch.zeros(2 * count, dtype=torch.from_numpy(z(1)).dtype)[::2]),
      ("tensor of a dtype that is not taken",
       lambda: torch.zeros(count, dtype=torch.from_numpy(z(1, dtype_bad)).dtype)),
      ("float64 tensor", lambda: torch.zeros(count, dtype=torch.float64)),
      ("int16 tensor", lambda: torch.zeros(count, dtype=torch.int16)),
      ("2-D tensor", lambda: torch.zeros(1, count, dtype=torch.from_numpy(z(1)).dtype)),
      ("tensor of the wrong length", lambda: torch.zeros(count + 1, dtype=torch.from_numpy(z(1)).dtype)),
      ("expanded tensor", lambda: torch.zeros(1, dtype=torch.from_numpy(z(1)).dtype).expand(count)),
      ("fake on the device", lambda: Fake(z(count))),
      ("fake on a foreign device type", lambda: Fake(z(count), (7, 0))),
      ("fake on device 1", lambda: Fake(z(count), (_dlpack.KDL_ROCM, 1))),
      ("fake that raises BufferError", lambda: Fake(z(count), error=BufferError("not exportable"))),
      ("fake with a capsule of the wrong name", lambda: Fake(z(count), name=_dlpack._USED_NAME)),
      ("fake with a negative stride", lambda: Fake(z(count), strides=(-1,))),
      # two rules at once: which one answers
      ("read-only and a dtype that is not taken", lambda: read_only(count, dtype_bad)),
      ("a dtype that is not taken and the wrong length", lambda: z(count + 1, dtype_bad)),
      ("wrong length and a negative stride", lambda: z(2 * count + 2)[::-2]),
      ("wrong ndim and the wrong length", lambda: z(count + 1).reshape(1, count + 1)),
      ("fake: foreign device type and device 1", lambda: Fake(z(count), (7, 1))),
      ("fake: wrong length and zero stride", lambda: Fake(torch.from_numpy(z(1)).expand(count + 1))),
      ("fake: wrong ndim and a dtype that is not taken",
       lambda: Fake(z(count, dtype_bad).reshape(1, count))),
  ]


def _cases():
  grid = []
  for role in ("embeddings", "strided", "out2d"):
    grid += [(role, name, make) for name, make in matrix_objects(np.float64, np.int32)]
  grid += [("out1d", name, make) for name, make in vector_objects(5, np.float64, np.int32)]
  for role in ("labels_in", "labels_out"):
    grid += [(role, name, make) for name, make in vector_objects(6, np.int64, np.complex64)]
  return grid


CASES = {"%s: %s" % (role, name): (role, make) for role, name, make in _cases()}


def base_address(obj):
  """The lowest address of the memory an object is a view of, or None."""
  if isinstance(obj, Fake):
    obj = obj.host
  if isinstance(obj, torch.Tensor):
    return obj.untyped_storage().data_ptr()
  if isinstance(obj, np.ndarray):
    while isinstance(obj.base, np.ndarray):
      obj = obj.base
    return obj.ctypes.data
  return None


def record(key):
  """One case -> {"raises", "message"} or {"array": [data, dtype, location, rows, cols, row_stride,
  col_stride]} with data = ["base", offset] inside the object's memory or ["copy", offset] from
  the beginning of the array the Source keeps."""
  role, make = CASES[key]
  obj = make()
  try:
    src = ROLES[role](obj)
  except Exception as e:  # pylint: disable=broad-except
    return {"raises": type(e).__name__, "message": str(e)}
  a = src.array
  if src.capsule is not None or src.keep is obj:
    data = ["base", int(a.data) - base_address(obj)]
  else:
    data = ["copy", int(a.data or 0) - src.keep.ctypes.data]
  got = {"array": [data, int(a.dtype), int(a.location), int(a.rows), int(a.cols),
                   int(a.row_stride), int(a.col_stride)]}
  src.release()
  return got


def main():
  table = {key: record(key) for key in CASES}
  with open(GOLDEN, "w") as f:
    json.dump(table, f, indent=1, sort_keys=True)
    f.write("\n")
  raised = sum("raises" in v for v in table.values())
  print("%s: %d cases, %d raise" % (GOLDEN, len(table), raised))


if __name__ == "__main__":
  main()
