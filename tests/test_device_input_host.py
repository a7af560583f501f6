"""Embeddings where they are, the part that needs no GPU: an input (NumPy array or DLPack
object) becomes the right `sc_array` descriptor, what cannot be taken is rejected before any
device call, and the C ABI grew by additions only.  PyTorch appears in tests only: the package
reads the DLPack capsule with ctypes."""

import ctypes
import gc
import os
import re

import numpy as np
import pytest
import torch

import spectralcluster_amd as sca
from spectralcluster_amd import _dlpack
from spectralcluster_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DTYPES = [(torch.float64, _lib.SC_DTYPE_F64), (torch.float32, _lib.SC_DTYPE_F32),
          (torch.float16, _lib.SC_DTYPE_F16), (torch.bfloat16, _lib.SC_DTYPE_BF16)]
LAYOUTS = {
    "contiguous": lambda b: b,
    "window": lambda b: b[1:5, 3:8],
    "transposed": lambda b: b.t(),
    "row_step_2": lambda b: b[::2],
}

NEW_SYMBOLS = ("sc_array_layout", "sc_set_embeddings_array", "sc_predict_array",
               "sc_predict_batch_arrays", "sc_stage_ingest")


def no_handle():
  raise AssertionError("a host input must not touch the device")


def capsule_name(capsule) -> bytes:
  get_name = ctypes.pythonapi.PyCapsule_GetName
  get_name.restype = ctypes.c_char_p
  get_name.argtypes = [ctypes.py_object]
  return get_name(capsule)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("dtype,code", DTYPES)
def test_descriptor_from_a_dlpack_capsule(dtype, code, layout):
  base = torch.arange(7 * 11, dtype=torch.float32).reshape(7, 11).to(dtype)
  t = LAYOUTS[layout](base)
  src = _dlpack.describe(t, no_handle)
  a = src.array
  assert a.data == t.data_ptr()
  assert a.dtype == code and a.location == _lib.SC_MEM_HOST
  assert (a.rows, a.cols) == tuple(t.shape) == src.shape
  assert (a.row_stride, a.col_stride) == tuple(t.stride())
  assert src.numpy is None
  # every element the descriptor names is the tensor's (read through the raw address)
  raw = (ctypes.c_char * (base.numel() * base.element_size())).from_address(base.data_ptr())
  flat = torch.frombuffer(raw, dtype=dtype)
  off = (a.data - base.data_ptr()) // base.element_size()
  for r in (0, a.rows - 1):
    for c in (0, a.cols - 1):
      got = flat[off + r * a.row_stride + c * a.col_stride]
      assert got == t[r, c]
  # consumed: the capsule has the name that keeps its destructor from deleting the tensor a
  # second time, and the producer gets it back when the library call is over
  assert capsule_name(src.capsule) == b"used_dltensor"
  src.release()
  src.release()  # (idempotent)
  del src, t, base, flat, raw
  gc.collect()


def test_only_compact_float64_host_rows_take_the_double_pointer_forms():
  d = lambda x: _dlpack.describe(x, no_handle)
  assert d(np.zeros((4, 3))).is_host_f64
  assert d(np.zeros((4, 3), dtype=np.int32)).is_host_f64      # promoted on the host
  assert d(np.zeros((4, 6))[:, ::2]).is_host_f64              # compacted
  assert not d(np.zeros((4, 3), dtype=np.float32)).is_host_f64
  t = torch.zeros(4, 6, dtype=torch.float64)
  assert d(t).is_host_f64
  assert not d(t[:, 1:4]).is_host_f64
  assert not d(t.t()).is_host_f64


@pytest.mark.parametrize("dtype,code", [(np.float64, _lib.SC_DTYPE_F64),
                                        (np.float32, _lib.SC_DTYPE_F32),
                                        (np.float16, _lib.SC_DTYPE_F16)])
def test_descriptor_from_numpy(dtype, code):
  x = np.arange(40, dtype=dtype).reshape(5, 8)
  src = _dlpack.describe(x, no_handle)
  a = src.array
  assert a.data == x.ctypes.data and src.keep is x and src.numpy is x
  assert (a.dtype, a.location, a.rows, a.cols, a.row_stride, a.col_stride) == (
      code, _lib.SC_MEM_HOST, 5, 8, 8, 1)
  # a view that is not C-contiguous is compacted in its own dtype
  for view in (x[:, 1:6], x.T, x[::2]):
    src = _dlpack.describe(view, no_handle)
    a = src.array
    assert src.keep.dtype == dtype and src.keep.flags["C_CONTIGUOUS"]
    assert np.array_equal(src.keep, view) and src.numpy is view
    assert a.data == src.keep.ctypes.data and a.dtype == code
    assert (a.rows, a.cols, a.row_stride, a.col_stride) == view.shape + (view.shape[1], 1)


def test_other_numpy_dtypes_are_promoted_to_float64_on_the_host():
  for x in (np.arange(12, dtype=np.int32).reshape(3, 4),
            np.arange(12, dtype=">f4").reshape(3, 4),
            np.ones((3, 4), dtype=bool)):
    src = _dlpack.describe(x, no_handle)
    assert src.keep.dtype == np.float64 and np.array_equal(src.keep, x.astype(np.float64))
    assert src.array.dtype == _lib.SC_DTYPE_F64 and src.array.data == src.keep.ctypes.data
    assert src.is_host_f64


def test_rejections_come_before_any_device_call(monkeypatch):
  def no_device(*a, **k):
    raise AssertionError("a device call was made")

  monkeypatch.setattr(_lib, "default_handle", no_device)
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=4)
  with pytest.raises(TypeError, match="embeddings must be a numpy array"):
    c.predict([[1.0, 2.0], [3.0, 4.0]])
  with pytest.raises(TypeError, match="embeddings must be a numpy array"):
    c.predict_batch([np.ones((3, 2)), [[1.0, 2.0]]])
  for t in (torch.zeros(5), torch.zeros(2, 3, 4)):
    with pytest.raises(ValueError, match="embeddings must be 2-dimensional"):
      c.predict(t)
  for dtype in (torch.int32, torch.int64, torch.uint8, torch.bool, torch.complex64):
    with pytest.raises(TypeError):
      c.predict(torch.zeros(4, 3, dtype=dtype))
  with pytest.raises(BufferError):  # PyTorch's own refusal, passed on as it is
    c.predict(torch.zeros(4, 3, requires_grad=True))
  with pytest.raises(ValueError, match="same d"):
    c.predict_batch([torch.zeros(4, 3), torch.zeros(4, 5)])

  class Elsewhere:  # an object that says it lives on a device type this library does not read
    def __dlpack_device__(self):
      return (8, 0)  # kDLMetal

    def __dlpack__(self, **kw):
      raise AssertionError("not asked for a capsule")

  with pytest.raises(TypeError, match="device type 8"):
    c.predict(Elsewhere())


def test_a_device_object_must_be_on_the_clusterers_device():
  class OnDevice3:
    def __dlpack_device__(self):
      return (10, 3)  # kDLROCM

    def __dlpack__(self, **kw):
      raise AssertionError("not asked for a capsule")

  class FakeHandle:
    device = 0

  with pytest.raises(ValueError, match="device 3"):
    _dlpack.describe(OnDevice3(), lambda: FakeHandle())


def test_a_device_object_is_asked_to_order_itself_before_the_handles_stream():
  asked = []
  t = torch.arange(12, dtype=torch.bfloat16).reshape(3, 4)

  class Device:
    def __dlpack_device__(self):
      return (10, 0)

    def __dlpack__(self, stream=None):
      asked.append(stream)
      return t.__dlpack__()

  class FakeHandle:
    device = 0

    def stream(self):
      return 0x5eed

  src = _dlpack.describe(Device(), lambda: FakeHandle())
  assert asked == [0x5eed]
  assert src.array.location == _lib.SC_MEM_DEVICE and src.array.dtype == _lib.SC_DTYPE_BF16
  assert src.array.data == t.data_ptr()
  src.release()


def test_header_binding_and_library_agree_on_the_additions():
  header = open(os.path.join(ROOT, "include", "spectralcluster_amd.h")).read()
  declared = set(re.findall(r"^(?:int|const char\*)\s+(sc_[a-z0-9_]+)\s*\(", header, flags=re.M))
  lib = _lib.load()
  for name in NEW_SYMBOLS:
    assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
  assert re.search(r"^void\*\s+sc_stream\s*\(", header, flags=re.M)
  assert "sc_stream" in _lib.POINTER_PROTOTYPES and hasattr(lib, "sc_stream")
  assert declared == set(_lib.PROTOTYPES)
  assert lib.sc_abi_version() == _lib.SC_ABI_VERSION == 11
  for i, name in enumerate(("F64", "F32", "F16", "BF16")):
    assert re.search(r"SC_DTYPE_%s\s*=\s*%d\b" % (name, i), header)
    assert getattr(_lib, "SC_DTYPE_" + name) == i
  for i, name in enumerate(("HOST", "DEVICE")):
    assert re.search(r"SC_MEM_%s\s*=\s*%d\b" % (name, i), header)
    assert getattr(_lib, "SC_MEM_" + name) == i
  # the mirror of sc_array: size and every field offset as the library was compiled
  size = ctypes.c_int(0)
  offsets = (ctypes.c_int * 7)()
  assert lib.sc_array_layout(ctypes.byref(size), offsets) == 0
  assert size.value == ctypes.sizeof(_lib.ScArray) == 48
  assert list(offsets) == [getattr(_lib.ScArray, f).offset for f, _ in _lib.ScArray._fields_]
  # the structs of ABI 7 are untouched
  cfg, diag = ctypes.c_int(0), ctypes.c_int(0)
  lib.sc_struct_sizes(ctypes.byref(cfg), ctypes.byref(diag))
  assert (cfg.value, diag.value) == (ctypes.sizeof(_lib.ScConfig), ctypes.sizeof(_lib.ScDiag))
