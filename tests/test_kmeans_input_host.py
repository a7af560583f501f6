"""The k-means entries take their input where it is, the part that needs no GPU: the C ABI grew
by three functions and nothing else, and the Python layer hands a C-contiguous float64 ndarray
to the `double*` entry points exactly as before and everything else it can describe to their
`_array` forms."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import custom_distance_kmeans as ckm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sc_stage_kmeans_general_array", "sc_stage_kmeans_metric_array",
               "sc_stage_ingest_columns")


def test_header_binding_and_library_agree_on_the_additions():
  header = open(os.path.join(ROOT, "include", "spectralcluster_amd.h")).read()
  declared = set(re.findall(r"^(?:int|const char\*)\s+(sc_[a-z0-9_]+)\s*\(", header, flags=re.M))
  lib = _lib.load()
  for name in NEW_SYMBOLS:
    assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
  assert declared == set(_lib.PROTOTYPES)
  # argument counts as the header declares them
  for name in NEW_SYMBOLS:
    args = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, header, flags=re.M | re.S).group(1)
    assert len(args.split(",")) == len(_lib.PROTOTYPES[name][1]), name
    assert _lib.PROTOTYPES[name][1][1] == ctypes.POINTER(_lib.ScArray)
  # additions only: the version every host test pins
  assert re.search(r"#define\s+SC_ABI_VERSION\s+11\b", header)
  assert lib.sc_abi_version() == _lib.SC_ABI_VERSION == 11


class Recorder:
  """Stands in for the handle: records every library call, answers SC_OK and writes nothing."""
  device, raw = 0, "raw"

  def __init__(self):
    self.calls = []
    self.lib = self

  def __getattr__(self, name):
    if not name.startswith("sc_"):
      raise AttributeError(name)

    def call(*args):
      self.calls.append((name,) + args)
      return _lib.SC_OK
    return call

  def check(self, rc):
    assert rc == _lib.SC_OK

  def stream(self):
    raise AssertionError("a host input must not ask for the stream")


@pytest.fixture
def recorder(monkeypatch):
  rec = Recorder()
  monkeypatch.setattr(_lib, "default_handle", lambda device=None: rec)
  return rec


def address(p) -> int:
  return ctypes.cast(p, ctypes.c_void_p).value


def described(arg):
  a = arg._obj  # (of ctypes.byref)
  return (a.data, a.dtype, a.location, a.rows, a.cols, a.row_stride, a.col_stride)


def test_a_contiguous_float64_ndarray_reaches_the_double_pointer_entries_as_before(recorder):
  x = np.arange(40, dtype=np.float64).reshape(10, 4)
  labels = ckm.run_kmeans(x, 4, "cosine", 7)
  (name, raw, e, n, k, max_iter, metric, lab, cent, iters), = recorder.calls
  assert (name, raw, n, k, max_iter, metric, cent) == (
      "sc_stage_kmeans_metric", "raw", 10, 4, 7, _lib.KMEANS_METRICS["cosine"], None)
  assert address(e) == x.ctypes.data and address(lab) == labels.ctypes.data
  assert labels.shape == (10,) and labels.dtype == np.int64

  del recorder.calls[:]
  ckm.run_kmeans(x, 3, "euclidean", 7)
  (name, raw, e, n, dim, k, max_iter, metric, tol, init, lab, cent, iters), = recorder.calls
  assert (name, raw, n, dim, k, max_iter, metric, tol, init) == (
      "sc_stage_kmeans_general", "raw", 10, 4, 3, 7, _lib.KMEANS_METRICS["euclidean"], 0.001, None)
  assert address(e) == x.ctypes.data

  del recorder.calls[:]
  init = x[:2].copy()
  km = ckm.CustomKMeans(2, centroids=init, max_iter=5, tol=0.25)
  km.predict(x)
  (name, raw, e, n, dim, k, max_iter, metric, tol, c0, lab, cent, iters), = recorder.calls
  assert (name, raw, n, dim, k, max_iter, metric, tol) == (
      "sc_stage_kmeans_general", "raw", 10, 4, 2, 5, _lib.KMEANS_METRICS["cosine"], 0.25)
  assert address(e) == x.ctypes.data and address(c0) == init.ctypes.data
  assert km.centroids is init

  # what is no float array is promoted on the host, as always
  for other in (x.astype(np.int32), x.tolist()):
    del recorder.calls[:]
    ckm.run_kmeans(other, 3, "cosine", 7)
    (name, _, _, n, dim, k), = [c[:6] for c in recorder.calls]
    assert (name, n, dim, k) == ("sc_stage_kmeans_general", 10, 4, 3)


def test_a_float32_ndarray_reaches_the_array_entries_at_its_own_width(recorder):
  x = np.arange(60, dtype=np.float32).reshape(10, 6)
  view = x[:, 1:5]
  ckm.run_kmeans(view, 4, "cosine", 7)
  (name, raw, arr, max_iter, metric, lab, cent, iters), = recorder.calls
  assert (name, raw, max_iter, metric, cent) == (
      "sc_stage_kmeans_metric_array", "raw", 7, _lib.KMEANS_METRICS["cosine"], None)
  assert described(arr) == (x.ctypes.data + 4, _lib.SC_DTYPE_F32, _lib.SC_MEM_HOST, 10, 4, 6, 1)

  del recorder.calls[:]
  ckm.run_kmeans(x, 4, "cosine", 7)
  (name, raw, arr, k, max_iter, metric, tol, init, lab, cent, iters), = recorder.calls
  assert (name, k, max_iter, metric, tol, init) == (
      "sc_stage_kmeans_general_array", 4, 7, _lib.KMEANS_METRICS["cosine"], 0.001, None)
  assert described(arr) == (x.ctypes.data, _lib.SC_DTYPE_F32, _lib.SC_MEM_HOST, 10, 6, 6, 1)

  del recorder.calls[:]
  init = np.zeros((3, 10))
  km = ckm.CustomKMeans(3, centroids=init)
  km.predict(x.T)  # a transposed view: its own strides, no host copy
  (name, raw, arr, k, max_iter, metric, tol, c0, lab, cent, iters), = recorder.calls
  assert (name, k, max_iter, tol) == ("sc_stage_kmeans_general_array", 3, 10, 0.001)
  assert described(arr) == (x.ctypes.data, _lib.SC_DTYPE_F32, _lib.SC_MEM_HOST, 6, 10, 1, 6)
  assert address(c0) == init.ctypes.data and km.centroids is init

  # float64 that is not C-contiguous, float16, and a DLPack object in host memory
  for obj, want in (
      (np.zeros((10, 8))[:, ::2], (_lib.SC_DTYPE_F64, 10, 4, 8, 2)),
      (np.zeros((10, 4), dtype=np.float16), (_lib.SC_DTYPE_F16, 10, 4, 4, 1)),
      (torch.zeros(10, 4, dtype=torch.bfloat16), (_lib.SC_DTYPE_BF16, 10, 4, 4, 1)),
      (torch.zeros(4, 10, dtype=torch.float64).t(), (_lib.SC_DTYPE_F64, 10, 4, 1, 10))):
    del recorder.calls[:]
    ckm.run_kmeans(obj, 4, "cosine", 7)
    (name, _, arr), = [c[:3] for c in recorder.calls]
    assert name == "sc_stage_kmeans_metric_array"
    d = described(arr)
    assert (d[1], d[3], d[4], d[5], d[6]) == want and d[2] == _lib.SC_MEM_HOST


def test_validation_order_is_the_references_whatever_the_input(recorder):
  for x in (np.zeros((8, 3), dtype=np.float32), torch.zeros(8, 3, dtype=torch.float16)):
    with pytest.raises(ValueError, match="Number of iterations"):
      ckm.CustomKMeans(9, centroids=np.zeros((3, 4)), max_iter=-1).predict(x)
    with pytest.raises(ValueError, match=r"^n_samples=8 should be >= n_clusters=9$"):
      ckm.CustomKMeans(9, centroids=np.zeros((3, 4))).predict(x)
    with pytest.raises(ValueError, match="shape of the initial centroids"):
      ckm.CustomKMeans(2, centroids=np.zeros((3, 3))).predict(x)
    with pytest.raises(ValueError, match="number of features of the initial centroids 4"):
      ckm.CustomKMeans(2, centroids=np.zeros((2, 4))).predict(x)
    with pytest.raises(sca.UnsupportedOnDeviceError):
      ckm.CustomKMeans(2, centroids=np.zeros((2, 3)), custom_dist="mahalanobis").predict(x)
    with pytest.raises(sca.UnsupportedOnDeviceError, match="float64"):
      ckm.CustomKMeans(2, centroids=np.zeros((2, 3), dtype=np.float32)).predict(x)
    with pytest.raises(sca.UnsupportedOnDeviceError):
      ckm.run_kmeans(x, 2, "mahalanobis", 10)
  with pytest.raises(TypeError, match="float64, float32, float16 or bfloat16"):
    ckm.run_kmeans(torch.zeros(8, 3, dtype=torch.int32), 2, "cosine", 10)
  with pytest.raises(BufferError):
    ckm.run_kmeans(torch.zeros(8, 3, requires_grad=True), 2, "cosine", 10)
  with pytest.raises(ValueError, match="2-dimensional"):
    ckm.run_kmeans(torch.zeros(8), 2, "cosine", 10)
  with pytest.raises(ValueError, match="spectral_embeddings must be 2-dimensional"):
    ckm.run_kmeans(np.zeros(8), 2, "cosine", 10)
  assert recorder.calls == []


def test_a_described_source_is_released_when_the_call_raises(monkeypatch):
  released = []

  class Failing(Recorder):
    def check(self, rc):
      raise ValueError("the library refused")

  rec = Failing()
  monkeypatch.setattr(_lib, "default_handle", lambda device=None: rec)
  real = ckm._describe

  def describe(obj):
    src = real(obj)
    release = src.release
    # (True for the call that hands the tensor back, False for the idempotent ones after it)
    src.release = lambda: (released.append(src._managed is not None), release())
    return src

  monkeypatch.setattr(ckm, "_describe", describe)
  t = torch.zeros(8, 3, dtype=torch.float32)
  with pytest.raises(ValueError, match="refused"):
    ckm.run_kmeans(t, 3, "cosine", 10)
  with pytest.raises(ValueError, match="refused"):
    ckm.CustomKMeans(2, centroids=np.zeros((2, 3))).predict(t)
  assert released[0] and released.count(True) == 2
