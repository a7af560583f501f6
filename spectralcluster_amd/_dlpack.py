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
  """An `sc_array` and what keeps its memory alive until `release()` (a context manager: leaving
  the `with` block releases).

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

  def __enter__(self) -> "Source":
    return self

  def __exit__(self, *exc) -> None:
    self.release()

  def __del__(self):
    try:
      self.release()
    except Exception:  # interpreter shutdown
      pass


def label_dtype_message(what: str, detail: str) -> str:
  """The TypeError text for a label array of a dtype that is not taken."""
  return "%s must be int64 or int32 (%s)" % (what, detail)


def label_input_dtype_message(what: str, detail: str) -> str:
  return ("%s must be int64 or int32, or float64 / float32 holding integral values (%s)"
          % (what, detail))


def is_described(obj) -> bool:
  """Not an ndarray, but something that can say where it is: it is read through DLPack."""
  return (not isinstance(obj, np.ndarray) and hasattr(obj, "__dlpack__") and
          hasattr(obj, "__dlpack_device__"))


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


# ---- one description path ------------------------------------------------------------------

def _promote_embeddings(a: np.ndarray, dtype, what: str):
  """ints, bools, longdouble, other byte orders: promoted to float64 on the host."""
  if dtype is None:
    return np.ascontiguousarray(a, dtype=np.float64), _lib.SC_DTYPE_F64
  return a, dtype


class _Role(typing.NamedTuple):
  """What one kind of argument asks of the object that is passed for it (`_describe`)."""
  what: str
  ndim: int
  numpy_dtypes: dict
  dlpack_dtypes: dict
  dtype_error: typing.Callable[[str, str], str]  # (what, detail) -> the TypeError text
  # ndarray only: (array, dtype or None, what) -> (array to describe, dtype); None: TypeError
  host_values: typing.Optional[typing.Callable] = None
  shape: typing.Optional[typing.Tuple[int, ...]] = None  # the shape it must have (None: any)
  shape_error: str = "%s must have shape %s, not %s"
  entries: bool = False     # a vector of n entries: the length is checked before the dtype
  writeable: bool = False   # an output: writeable memory, no two indices at one address
  alias_error: str = "%s maps two indices to one address (strides %s of shape %s)"
  strided: bool = True      # a NumPy view keeps its strides ...
  copies: bool = False      # ... and one that cannot is made contiguous on the host (no error)
  stride_error: str = "%s: strides must be multiples of the item size"
  not_array: str = "%s must be a numpy array or an object with __dlpack__"
  foreign_device: str = ("%s lives on DLPack device type %d: host memory and ROCm device memory "
                         "are supported")
  other_device: str = "%s is on device %d, the library runs on device %d"
  export_error: typing.Optional[str] = None  # a producer's BufferError as ValueError (None: as is)


_EMBEDDINGS = _Role(
    "embeddings", 2, _NUMPY_DTYPES, _DLPACK_DTYPES, dtype_message, _promote_embeddings,
    copies=True, not_array="%s must be a numpy array",
    foreign_device="%s live on DLPack device type %d: host memory and ROCm device memory are "
                   "supported",
    other_device="%s are on device %d, the clusterer runs on device %d")
_OUT = _Role("out", 2, _NUMPY_DTYPES, _DLPACK_DTYPES, dtype_message, writeable=True,
             export_error="%s cannot be exported as writeable memory: %s")
_LABELS = _Role("labels", 1, _LABEL_NUMPY_DTYPES, _LABEL_DLPACK_INPUTS, label_input_dtype_message,
                shape_error="%s must hold %s entries, not %s", entries=True,
                stride_error="%s: the stride must be a multiple of the item size",
                export_error="%s cannot be exported: %s")
_LABELS_OUT = _Role("out", 1, _LABEL_NUMPY_DTYPES, _LABEL_DLPACK_DTYPES, label_dtype_message,
                    writeable=True, alias_error="%s maps two indices to one address (stride 0)",
                    stride_error=_LABELS.stride_error, export_error=_LABELS.export_error)


def _alias_message(role: _Role, strides, shape) -> str:
  text = role.alias_error
  return text % ((role.what, tuple(strides), shape) if text.count("%s") == 3 else role.what)


def _shape_message(role: _Role, got) -> str:
  want = role.shape
  if role.entries:
    want, got = want[0], got[0]
  return role.shape_error % (role.what, want, got)


def _from_numpy(a: np.ndarray, role: _Role) -> Source:
  what, given = role.what, a
  if role.writeable and not a.flags.writeable:
    raise ValueError("%s is not writeable" % what)
  if role.host_values is not None and a.ndim != role.ndim:
    raise ValueError("%s must be %d-dimensional" % (what, role.ndim))
  if role.entries and a.shape != role.shape:
    raise ValueError(_shape_message(role, a.shape))
  dtype = role.numpy_dtypes.get(a.dtype)
  if role.host_values is not None:
    a, dtype = role.host_values(a, dtype, what)
  elif dtype is None:
    raise TypeError(role.dtype_error(what, "numpy %s" % a.dtype))
  if role.shape is not None and a.shape != role.shape:
    raise ValueError(_shape_message(role, a.shape))
  lies = role.strided and all(s >= 0 and s % a.itemsize == 0 for s in a.strides)
  if not lies and not role.copies:
    if any(s < 0 for s in a.strides):
      raise ValueError(negative_strides_message(what))
    raise ValueError(role.stride_error % what)
  shape, strides = a.shape, [s // a.itemsize for s in a.strides]
  if not lies:
    a = np.ascontiguousarray(a)
    strides = [shape[1], 1]
  if role.writeable and not view_is_injective(shape, strides):
    raise ValueError(_alias_message(role, strides, shape))
  if role.ndim == 1:  # a vector is described as one row
    shape, strides = (1,) + shape, [0] + strides
  arr = _lib.ScArray(a.ctypes.data, dtype, _lib.SC_MEM_HOST, shape[0], shape[1], strides[0],
                     strides[1])
  # (host branches compute on the caller's own embeddings, and on the labels as they were read)
  return Source(arr, a, numpy=given if role.copies else a)


def _from_capsule(capsule, location: int, role: _Role) -> Source:
  """The legacy "dltensor" capsule of a DLPack object -> Source (a vector as one row)."""
  what, ndim = role.what, role.ndim
  address = _get_pointer(capsule, _NAME)  # raises ValueError for a capsule of another name
  managed = ctypes.cast(address, ctypes.POINTER(DLManagedTensor))
  _set_name(capsule, _USED_NAME)  # consumed: the deleter is ours to call now
  src = Source(_lib.ScArray(), None, capsule=capsule, managed=managed)
  try:
    t = managed.contents.dl_tensor
    if t.ndim != ndim:
      raise ValueError("%s must be %d-dimensional" % (what, ndim))
    dtype = role.dlpack_dtypes.get((t.dtype.code, t.dtype.bits)) if t.dtype.lanes == 1 else None
    if dtype is None:
      raise TypeError(role.dtype_error(what, "DLPack type code %d, %d bits, %d lanes"
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
    got = (cols,) if ndim == 1 else (rows, cols)
    if role.shape is not None and got != role.shape:
      raise ValueError(_shape_message(role, got))
    if role.writeable and not view_is_injective((rows, cols), (row_stride, col_stride)):
      raise ValueError(_alias_message(role, (row_stride, col_stride), got))
  except Exception:
    src.release()
    raise
  return src


def _describe(obj, get_handle: typing.Callable[[], "_lib.Handle"], role: _Role) -> Source:
  """`obj` in `role` -> Source.  TypeError / ValueError naming `role.what` for what cannot be
  taken, before any device call.  An ndarray is checked and described here; anything else has
  to say where it lives (`__dlpack_device__`): host memory is read through its capsule as it is;
  for the handle's device (`get_handle` is called for such an object only) the producer is handed
  the library's stream, which it makes wait for whatever still uses the tensor."""
  what = role.what
  if isinstance(obj, np.ndarray):
    return _from_numpy(obj, role)
  if not (hasattr(obj, "__dlpack__") and hasattr(obj, "__dlpack_device__")):
    raise TypeError(role.not_array % what)
  device_type, device_id = obj.__dlpack_device__()
  device_type = int(device_type)
  try:
    if device_type in HOST_DEVICE_TYPES:
      return _from_capsule(obj.__dlpack__(), _lib.SC_MEM_HOST, role)
    if device_type not in DEVICE_DEVICE_TYPES:
      raise TypeError(role.foreign_device % (what, device_type))
    handle = get_handle()
    if int(device_id) != handle.device:
      raise ValueError(role.other_device % (what, int(device_id), handle.device))
    return _from_capsule(obj.__dlpack__(stream=handle.stream()), _lib.SC_MEM_DEVICE, role)
  except BufferError as e:  # what a producer answers for memory it will not hand out
    if role.export_error is None:
      raise
    raise ValueError(role.export_error % (what, e)) from e


# ---- the roles' public names -----------------------------------------------------------------

def describe(embeddings, get_handle: typing.Callable[[], "_lib.Handle"],
             strided: bool = False) -> Source:
  """`embeddings` -> Source.  TypeError / ValueError for what cannot be taken, before any
  device call (`get_handle` is only called for an object that says it lives on a GPU: its
  device must be the handle's, and the handle's stream goes to `__dlpack__`).  `strided`: a
  NumPy view keeps its strides (the affinity entry points take them); otherwise it is made
  contiguous on the host, as the embeddings paths expect."""
  return _describe(embeddings, get_handle, _EMBEDDINGS._replace(strided=strided))


def describe_input(obj, get_handle: typing.Callable[[], "_lib.Handle"]) -> Source:
  """`describe(..., strided=True)` for the building blocks: whatever is neither an ndarray nor a
  DLPack object (a list, say) becomes an ndarray first, as `np.ascontiguousarray` made it one."""
  if not isinstance(obj, np.ndarray) and not is_described(obj):
    obj = np.asarray(obj)
  return describe(obj, get_handle, strided=True)


def describe_out(out, get_handle: typing.Callable[[], "_lib.Handle"],
                 shape: typing.Tuple[int, ...], what: str = "out") -> Source:
  """`out` -> the Source the library writes into.  A writeable ndarray (float64 / float32 /
  float16) or a DLPack object (those and bfloat16) in host memory or on the handle's device, of
  exactly `shape` (1-D or 2-D), with non-negative strides under which no two indices share an
  address.  TypeError / ValueError naming `what` for anything else, before any launch."""
  shape = tuple(int(e) for e in shape)
  return _describe(out, get_handle, _OUT._replace(what=what, ndim=len(shape), shape=shape))


def _label_values(a: np.ndarray, dtype, what: str):
  """The values of a host label array: finite, integral, at most `MAX_LABEL`; integer types the
  library does not read are converted here."""
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
  return a, dtype


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
  return _describe(labels, get_handle,
                   _LABELS._replace(what=what, shape=(n,), host_values=_label_values))


def describe_labels_out(out, get_handle: typing.Callable[[], "_lib.Handle"], n: int,
                        what: str = "out") -> Source:
  """`out` for labels -> the Source they are written into: a writeable 1-D ndarray or DLPack
  object of int64 or int32 with exactly `n` entries, in host memory or on the handle's device,
  with a non-negative stride that gives every entry its own address.  TypeError / ValueError
  naming `what` for anything else, before any launch."""
  return _describe(out, get_handle, _LABELS_OUT._replace(what=what, shape=(n,)))


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
