"""Embeddings as the caller holds them -> an `sc_array` descriptor (include/spectralcluster_amd.h).

A NumPy array of float64 / float32 / float16 is described in its own dtype (other dtypes are
promoted to float64 on the host, as always); anything with `__dlpack__` / `__dlpack_device__` --
a PyTorch tensor on the GPU, say, float64 / float32 / float16 / bfloat16 -- is read where it
is, strides and all, through the legacy "dltensor" capsule.  The capsule is parsed with ctypes:
this package imports no tensor library.

For a device object the producer is asked to order its work before the library's stream
(`__dlpack__(stream=<the handle's hipStream_t>)`), so the caller synchronises nothing.
"""

from __future__ import annotations

import ctypes
import typing

import numpy as np

from spectralcluster_amd import _lib

# DLDeviceType
KDL_CPU, KDL_CUDA, KDL_ROCM, KDL_ROCM_HOST = 1, 2, 10, 11
HOST_DEVICE_TYPES = (KDL_CPU, KDL_ROCM_HOST)
# (a ROCm build of PyTorch may report its device memory as kDLCUDA)
DEVICE_DEVICE_TYPES = (KDL_ROCM, KDL_CUDA)
# DLDataTypeCode
KDL_INT, KDL_FLOAT, KDL_BFLOAT = 0, 2, 4

_NUMPY_DTYPES = {np.dtype(np.float64): _lib.SC_DTYPE_F64, np.dtype(np.float32): _lib.SC_DTYPE_F32,
                 np.dtype(np.float16): _lib.SC_DTYPE_F16}
_DLPACK_DTYPES = {(KDL_FLOAT, 64): _lib.SC_DTYPE_F64, (KDL_FLOAT, 32): _lib.SC_DTYPE_F32,
                  (KDL_FLOAT, 16): _lib.SC_DTYPE_F16, (KDL_BFLOAT, 16): _lib.SC_DTYPE_BF16}
# label arrays (`describe_labels` / `describe_labels_out`): int64 / int32; as an input also float64 /
# float32 holding integral values (predict() returns float64 labels for a size-reduced utterance)
_LABEL_NUMPY_DTYPES = {np.dtype(np.int64): _lib.SC_DTYPE_I64, np.dtype(np.int32): _lib.SC_DTYPE_I32}
_LABEL_NUMPY_FLOATS = {np.dtype(np.float64): _lib.SC_DTYPE_F64,
                       np.dtype(np.float32): _lib.SC_DTYPE_F32}
_LABEL_DLPACK_DTYPES = {(KDL_INT, 64): _lib.SC_DTYPE_I64, (KDL_INT, 32): _lib.SC_DTYPE_I32}
_LABEL_DLPACK_INPUTS = {(KDL_INT, 64): _lib.SC_DTYPE_I64, (KDL_INT, 32): _lib.SC_DTYPE_I32,
                        (KDL_FLOAT, 64): _lib.SC_DTYPE_F64, (KDL_FLOAT, 32): _lib.SC_DTYPE_F32}
# the largest label: k = max + 1 is an int32 as well
MAX_LABEL = 2**31 - 2
# bytes of an element, by sc_array.dtype
ITEM_BYTES = {_lib.SC_DTYPE_F64: 8, _lib.SC_DTYPE_F32: 4, _lib.SC_DTYPE_F16: 2,
              _lib.SC_DTYPE_BF16: 2, _lib.SC_DTYPE_I64: 8, _lib.SC_DTYPE_I32: 4}


class DLDevice(ctypes.Structure):
  _fields_ = [("device_type", ctypes.c_int32), ("device_id", ctypes.c_int32)]


class DLDataType(ctypes.Structure):
  _fields_ = [("code", ctypes.c_uint8), ("bits", ctypes.c_uint8), ("lanes", ctypes.c_uint16)]


class DLTensor(ctypes.Structure):
  _fields_ = [("data", ctypes.c_void_p), ("device", DLDevice), ("ndim", ctypes.c_int32),
              ("dtype", DLDataType), ("shape", ctypes.POINTER(ctypes.c_int64)),
              ("strides", ctypes.POINTER(ctypes.c_int64)), ("byte_offset", ctypes.c_uint64)]


class DLManagedTensor(ctypes.Structure):
  pass


_deleter_t = ctypes.CFUNCTYPE(None, ctypes.POINTER(DLManagedTensor))
DLManagedTensor._fields_ = [("dl_tensor", DLTensor), ("manager_ctx", ctypes.c_void_p),
                            ("deleter", _deleter_t)]

# (PyCapsule_SetName keeps the pointer, not a copy: the names live as long as the module)
_NAME = b"dltensor"
_USED_NAME = b"used_dltensor"
_get_pointer = ctypes.pythonapi.PyCapsule_GetPointer
_get_pointer.restype = ctypes.c_void_p
_get_pointer.argtypes = [ctypes.py_object, ctypes.c_char_p]
_set_name = ctypes.pythonapi.PyCapsule_SetName
_set_name.restype = ctypes.c_int
_set_name.argtypes = [ctypes.py_object, ctypes.c_char_p]


def dtype_message(what: str, detail: str) -> str:
  """The TypeError text for a source of a dtype that is none of the four."""
  return "%s must be float64, float32, float16 or bfloat16 (%s)" % (what, detail)


def negative_strides_message(what: str) -> str:
  """The ValueError text for a source with a negative stride."""
  return "%s with negative strides are not supported" % what


class Source:
  """An `sc_array` and what keeps its memory alive until `release()`.

  `array`    the descriptor (pass `ctypes.byref(src.array)`),
  `numpy`    the caller's ndarray when the input was one (host branches use it as it is),
  `capsule`  the consumed DLPack capsule otherwise.
  """

  def __init__(self, array: _lib.ScArray, keep, numpy=None, capsule=None, managed=None):
    self.array = array
    self.keep = keep
    self.numpy = numpy
    self.capsule = capsule
    self._managed = managed

  @property
  def shape(self) -> typing.Tuple[int, int]:
    return int(self.array.rows), int(self.array.cols)

  @property
  def is_host_f64(self) -> bool:
    """Compact float64 rows in host memory: what the `double*` entry points take."""
    a = self.array
    return (a.location == _lib.SC_MEM_HOST and a.dtype == _lib.SC_DTYPE_F64 and
            a.col_stride == 1 and a.row_stride == a.cols)

  def host_f64(self, handle: "_lib.Handle") -> np.ndarray:
    """The values as a host float64 array, for the branches that compute on the host side of
    the API (fallback clusterer, size reduction, a user's affinity function): the caller's own
    ndarray, or one copy through `sc_stage_ingest`."""
    if self.numpy is not None:
      return self.numpy
    out = np.empty(self.shape, dtype=np.float64)
    handle.check(handle.lib.sc_stage_ingest(handle.raw, ctypes.byref(self.array),
                                            _lib.as_double_p(out)))
    return out

  def release(self) -> None:
    """The library call has returned: hand a DLPack tensor back to its producer."""
    managed, self._managed = self._managed, None
    if managed is not None and managed.contents.deleter:
      managed.contents.deleter(managed)
    self.keep = None

  def __del__(self):
    try:
      self.release()
    except Exception:  # interpreter shutdown
      pass


def _from_numpy(a: np.ndarray, strided: bool = False) -> Source:
  if a.ndim != 2:
    raise ValueError("embeddings must be 2-dimensional")
  dtype = _NUMPY_DTYPES.get(a.dtype)
  if (strided and dtype is not None and
      all(s >= 0 and s % a.itemsize == 0 for s in a.strides)):
    # a view (a .T, a [::2, ::2] slice) is described as it lies: no host copy of n x n values
    arr = _lib.ScArray(a.ctypes.data, dtype, _lib.SC_MEM_HOST, a.shape[0], a.shape[1],
                       a.strides[0] // a.itemsize, a.strides[1] // a.itemsize)
    return Source(arr, a, numpy=a)
  if dtype is None:  # ints, bools, longdouble, other byte orders: promoted on the host
    x = np.ascontiguousarray(a, dtype=np.float64)
    dtype = _lib.SC_DTYPE_F64
  else:
    x = np.ascontiguousarray(a)
  arr = _lib.ScArray(x.ctypes.data, dtype, _lib.SC_MEM_HOST, x.shape[0], x.shape[1],
                     x.shape[1], 1)
  return Source(arr, x, numpy=a)


def _from_capsule(capsule, location: int, what: str = "embeddings", ndim: int = 2,
                  dtypes=None, dtype_error=None) -> Source:
  """`ndim` 1 (a vector): described as one row, (1, count).  `dtypes` / `dtype_error`: the DLPack
  dtypes taken and the TypeError text for another one (default: the four float dtypes)."""
  dtypes = _DLPACK_DTYPES if dtypes is None else dtypes
  dtype_error = dtype_message if dtype_error is None else dtype_error
  address = _get_pointer(capsule, _NAME)  # raises ValueError for a capsule of another name
  managed = ctypes.cast(address, ctypes.POINTER(DLManagedTensor))
  _set_name(capsule, _USED_NAME)  # consumed: the deleter is ours to call now
  src = Source(_lib.ScArray(), None, capsule=capsule, managed=managed)
  try:
    t = managed.contents.dl_tensor
    if t.ndim != ndim:
      raise ValueError("%s must be %d-dimensional" % (what, ndim))
    dtype = dtypes.get((t.dtype.code, t.dtype.bits)) if t.dtype.lanes == 1 else None
    if dtype is None:
      raise TypeError(dtype_error(what, "DLPack type code %d, %d bits, %d lanes"
                                  % (t.dtype.code, t.dtype.bits, t.dtype.lanes)))
    if ndim == 1:
      rows, cols = 1, int(t.shape[0])
      row_stride, col_stride = 0, (int(t.strides[0]) if t.strides else 1)
    else:
      rows, cols = int(t.shape[0]), int(t.shape[1])
      row_stride, col_stride = (int(t.strides[0]), int(t.strides[1])) if t.strides else (cols, 1)
    if row_stride < 0 or col_stride < 0:
      raise ValueError(negative_strides_message(what))
    itemsize = t.dtype.bits // 8
    assert int(t.byte_offset) % itemsize == 0
    src.array = _lib.ScArray((t.data or 0) + int(t.byte_offset), dtype, location, rows, cols,
                             row_stride, col_stride)
  except Exception:
    src.release()
    raise
  return src


def describe(embeddings, get_handle: typing.Callable[[], "_lib.Handle"],
             strided: bool = False) -> Source:
  """`embeddings` -> Source.  TypeError / ValueError for what cannot be taken, before any
  device call (`get_handle` is only called for an object that says it lives on a GPU: its
  device must be the handle's, and the handle's stream goes to `__dlpack__`).  `strided`: a
  NumPy view keeps its strides (the affinity entry points take them); otherwise it is made
  contiguous on the host, as the embeddings paths expect."""
  if isinstance(embeddings, np.ndarray):
    return _from_numpy(embeddings, strided)
  if not (hasattr(embeddings, "__dlpack__") and hasattr(embeddings, "__dlpack_device__")):
    raise TypeError("embeddings must be a numpy array")
  device_type, device_id = embeddings.__dlpack_device__()
  device_type = int(device_type)
  if device_type in HOST_DEVICE_TYPES:
    return _from_capsule(embeddings.__dlpack__(), _lib.SC_MEM_HOST)
  if device_type not in DEVICE_DEVICE_TYPES:
    raise TypeError("embeddings live on DLPack device type %d: host memory and ROCm device "
                    "memory are supported" % device_type)
  handle = get_handle()
  if int(device_id) != handle.device:
    raise ValueError("embeddings are on device %d, the clusterer runs on device %d"
                     % (int(device_id), handle.device))
  # the producer makes the library's stream wait for whatever still writes the tensor
  return _from_capsule(embeddings.__dlpack__(stream=handle.stream()), _lib.SC_MEM_DEVICE)


# ---- results where the caller wants them -------------------------------------------------------

def is_described(obj) -> bool:
  """Not an ndarray, but something that can say where it is: it is read through DLPack."""
  return (not isinstance(obj, np.ndarray) and hasattr(obj, "__dlpack__") and
          hasattr(obj, "__dlpack_device__"))


def describe_input(obj, get_handle: typing.Callable[[], "_lib.Handle"]) -> Source:
  """`describe(..., strided=True)` for the building blocks: whatever is neither an ndarray nor a
  DLPack object (a list, say) becomes an ndarray first, as `np.ascontiguousarray` made it one."""
  if not isinstance(obj, np.ndarray) and not is_described(obj):
    obj = np.asarray(obj)
  return describe(obj, get_handle, strided=True)


def view_is_injective(shape: typing.Sequence[int], strides: typing.Sequence[int]) -> bool:
  """No two indices of the view share an address -- the rule `out=` is held to: over the
  dimensions of more than one element, ordered by stride, the small stride is >= 1 and the big
  one >= small stride * extent of the small one (element strides; the library checks the same)."""
  dims = sorted((int(s), int(e)) for e, s in zip(shape, strides) if int(e) > 1)
  if not dims:
    return True
  if dims[0][0] < 1:
    return False
  return len(dims) == 1 or dims[1][0] >= dims[0][0] * dims[0][1]


def describe_out(out, get_handle: typing.Callable[[], "_lib.Handle"],
                 shape: typing.Tuple[int, ...], what: str = "out") -> Source:
  """`out` -> the Source the library writes into.  A writeable ndarray (float64 / float32 /
  float16) or a DLPack object (those and bfloat16) in host memory or on the handle's device, of
  exactly `shape` (1-D or 2-D), with non-negative strides under which no two indices share an
  address.  TypeError / ValueError naming `what` for anything else, before any launch."""
  shape = tuple(int(e) for e in shape)
  if isinstance(out, np.ndarray):
    if not out.flags.writeable:
      raise ValueError("%s is not writeable" % what)
    dtype = _NUMPY_DTYPES.get(out.dtype)
    if dtype is None:
      raise TypeError(dtype_message(what, "numpy %s" % out.dtype))
    if out.shape != shape:
      raise ValueError("%s must have shape %s, not %s" % (what, shape, out.shape))
    if any(s < 0 for s in out.strides):
      raise ValueError(negative_strides_message(what))
    if any(s % out.itemsize for s in out.strides):
      raise ValueError("%s: strides must be multiples of the item size" % what)
    strides = [s // out.itemsize for s in out.strides]
    if not view_is_injective(shape, strides):
      raise ValueError("%s maps two indices to one address (strides %s of shape %s)"
                       % (what, tuple(strides), shape))
    if len(shape) == 1:
      shape, strides = (1,) + shape, [0] + strides
    arr = _lib.ScArray(out.ctypes.data, dtype, _lib.SC_MEM_HOST, shape[0], shape[1],
                       strides[0], strides[1])
    return Source(arr, out, numpy=out)
  if not (hasattr(out, "__dlpack__") and hasattr(out, "__dlpack_device__")):
    raise TypeError("%s must be a numpy array or an object with __dlpack__" % what)
  device_type, device_id = out.__dlpack_device__()
  device_type = int(device_type)
  try:
    if device_type in HOST_DEVICE_TYPES:
      src = _from_capsule(out.__dlpack__(), _lib.SC_MEM_HOST, what, len(shape))
    elif device_type in DEVICE_DEVICE_TYPES:
      handle = get_handle()
      if int(device_id) != handle.device:
        raise ValueError("%s is on device %d, the library runs on device %d"
                         % (what, int(device_id), handle.device))
      # the producer makes the library's stream wait for whatever still uses the tensor
      src = _from_capsule(out.__dlpack__(stream=handle.stream()), _lib.SC_MEM_DEVICE, what,
                          len(shape))
    else:
      raise TypeError("%s lives on DLPack device type %d: host memory and ROCm device memory "
                      "are supported" % (what, device_type))
  except BufferError as e:  # what a producer answers for memory it will not hand out writeable
    raise ValueError("%s cannot be exported as writeable memory: %s" % (what, e)) from e
  a = src.array
  got = (int(a.cols),) if len(shape) == 1 else (int(a.rows), int(a.cols))
  try:
    if got != shape:
      raise ValueError("%s must have shape %s, not %s" % (what, shape, got))
    if not view_is_injective((a.rows, a.cols), (a.row_stride, a.col_stride)):
      raise ValueError("%s maps two indices to one address (strides %s of shape %s)"
                       % (what, (int(a.row_stride), int(a.col_stride)), got))
  except Exception:
    src.release()
    raise
  return src


# ---- label arrays --------------------------------------------------------------------------

def label_dtype_message(what: str, detail: str) -> str:
  """The TypeError text for a label array of a dtype that is not taken."""
  return "%s must be int64 or int32 (%s)" % (what, detail)


def label_input_dtype_message(what: str, detail: str) -> str:
  return ("%s must be int64 or int32, or float64 / float32 holding integral values (%s)"
          % (what, detail))


def _label_capsule(obj, get_handle, what: str, dtypes, dtype_error) -> Source:
  """A 1-D DLPack object in host memory or on the handle's device -> Source."""
  device_type, device_id = obj.__dlpack_device__()
  device_type = int(device_type)
  try:
    if device_type in HOST_DEVICE_TYPES:
      return _from_capsule(obj.__dlpack__(), _lib.SC_MEM_HOST, what, 1, dtypes, dtype_error)
    if device_type not in DEVICE_DEVICE_TYPES:
      raise TypeError("%s lives on DLPack device type %d: host memory and ROCm device memory "
                      "are supported" % (what, device_type))
    handle = get_handle()
    if int(device_id) != handle.device:
      raise ValueError("%s is on device %d, the library runs on device %d"
                       % (what, int(device_id), handle.device))
    return _from_capsule(obj.__dlpack__(stream=handle.stream()), _lib.SC_MEM_DEVICE, what, 1,
                         dtypes, dtype_error)
  except BufferError as e:  # what a producer answers for memory it will not hand out
    raise ValueError("%s cannot be exported: %s" % (what, e)) from e


def _label_vector(a: np.ndarray, dtype: int, what: str) -> _lib.ScArray:
  if a.strides[0] < 0:
    raise ValueError(negative_strides_message(what))
  if a.strides[0] % a.itemsize:
    raise ValueError("%s: the stride must be a multiple of the item size" % what)
  return _lib.ScArray(a.ctypes.data, dtype, _lib.SC_MEM_HOST, 1, a.shape[0], 0,
                      a.strides[0] // a.itemsize)


def describe_labels(labels, get_handle: typing.Callable[[], "_lib.Handle"], n: int,
                    what: str = "labels") -> Source:
  """A label array as an input -> Source: 1-D, `n` entries, a NumPy array (anything else that is
  no DLPack object becomes one first) or a DLPack object, in host memory or on the handle's
  device, any non-negative stride.  int64 / int32 are read as they are, and so are float64 /
  float32 holding integral values; host arrays of other integer types are converted on the host.
  The values of a host NumPy array are checked here (finite, integral, at most `MAX_LABEL`); those
  of a DLPack object by the library.  TypeError / ValueError naming `what`, before any launch."""
  if not isinstance(labels, np.ndarray) and not is_described(labels):
    labels = np.asarray(labels)
  if not isinstance(labels, np.ndarray):
    src = _label_capsule(labels, get_handle, what, _LABEL_DLPACK_INPUTS, label_input_dtype_message)
    if int(src.array.cols) != n:
      got = int(src.array.cols)
      src.release()
      raise ValueError("%s must hold %d entries, not %d" % (what, n, got))
    return src
  if labels.ndim != 1:
    raise ValueError("%s must be 1-dimensional" % what)
  if labels.shape[0] != n:
    raise ValueError("%s must hold %d entries, not %d" % (what, n, labels.shape[0]))
  a = labels
  dtype = _LABEL_NUMPY_DTYPES.get(a.dtype)
  if dtype is None:
    dtype = _LABEL_NUMPY_FLOATS.get(a.dtype)
    if dtype is not None:
      if not np.all(np.isfinite(a)) or not np.all(a == np.trunc(a)):
        raise ValueError("%s: a float label array must hold finite integral values" % what)
    elif a.dtype.kind in "iub":  # other widths, byte orders, bools: converted on the host
      if a.dtype.kind == "u" and a.size and int(a.max()) > MAX_LABEL:
        raise ValueError("%s: a label is above %d" % (what, MAX_LABEL))
      a, dtype = a.astype(np.int64), _lib.SC_DTYPE_I64
    else:
      raise TypeError(label_input_dtype_message(what, "numpy %s" % a.dtype))
  if a.size and a.max() > MAX_LABEL:
    raise ValueError("%s: a label is above %d" % (what, MAX_LABEL))
  return Source(_label_vector(a, dtype, what), a, numpy=a)


def describe_labels_out(out, get_handle: typing.Callable[[], "_lib.Handle"], n: int,
                        what: str = "out") -> Source:
  """`out` for labels -> the Source they are written into: a writeable 1-D ndarray or DLPack
  object of int64 or int32 with exactly `n` entries, in host memory or on the handle's device,
  with a non-negative stride that gives every entry its own address.  TypeError / ValueError
  naming `what` for anything else, before any launch."""
  if isinstance(out, np.ndarray):
    if not out.flags.writeable:
      raise ValueError("%s is not writeable" % what)
    dtype = _LABEL_NUMPY_DTYPES.get(out.dtype)
    if dtype is None:
      raise TypeError(label_dtype_message(what, "numpy %s" % out.dtype))
    if out.shape != (n,):
      raise ValueError("%s must have shape %s, not %s" % (what, (n,), out.shape))
    src = Source(_label_vector(out, dtype, what), out, numpy=out)
  elif hasattr(out, "__dlpack__") and hasattr(out, "__dlpack_device__"):
    src = _label_capsule(out, get_handle, what, _LABEL_DLPACK_DTYPES, label_dtype_message)
    if int(src.array.cols) != n:
      got = int(src.array.cols)
      src.release()
      raise ValueError("%s must have shape %s, not %s" % (what, (n,), (got,)))
  else:
    raise TypeError("%s must be a numpy array or an object with __dlpack__" % what)
  if n > 1 and int(src.array.col_stride) < 1:
    src.release()
    raise ValueError("%s maps two indices to one address (stride 0)" % what)
  return src


def device_overlap(outs: typing.Sequence[Source], sources: typing.Sequence[Source]
                   ) -> typing.Optional[int]:
  """The index of the first of `outs` in device memory whose byte range overlaps the byte range
  of one of `sources` in device memory, or None.  `sc_cluster_centroids_arrays` makes this check
  itself and is the authority (callers of the C ABI have no other); it is made here as well
  because every argument error of the Python functions is raised before a library call, as
  `describe_out` does for shapes and strides."""
  def byte_range(a):
    eb = ITEM_BYTES[int(a.dtype)]
    last = (int(a.rows) - 1) * int(a.row_stride) + (int(a.cols) - 1) * int(a.col_stride)
    lo = int(a.data or 0)
    return lo, lo + (last + 1) * eb
  read = sorted(byte_range(s.array) for s in sources
                if s.array.location == _lib.SC_MEM_DEVICE and s.array.rows and s.array.cols)
  if not read:
    return None
  starts = np.array([r[0] for r in read], dtype=np.uint64)
  reach = np.maximum.accumulate(np.array([r[1] for r in read], dtype=np.uint64))
  for i, out in enumerate(outs):
    a = out.array
    if a.location != _lib.SC_MEM_DEVICE or not (a.rows and a.cols):
      continue
    lo, hi = byte_range(a)
    before = int(np.searchsorted(starts, np.uint64(hi), side="left"))
    if before > 0 and int(reach[before - 1]) > lo:
      return i
  return None
