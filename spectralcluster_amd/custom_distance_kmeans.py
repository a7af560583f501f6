"""K-means on the spectral embedding (mirror of reference
`spectralcluster/custom_distance_kmeans.py`): sklearn's k-means++ seeds + the custom-distance
loop (cosine by default; euclidean, sqeuclidean, cityblock, chebyshev, correlation, braycurtis,
canberra) in HIP kernels.  `run_kmeans` on an (n, n_clusters) embedding (what predict() hands
it) runs the single-kernel form of kmeans.hip / kmeans_chain.hip; any other width, and
`CustomKMeans`, run the general form of kmeans_general.hip.

Both take their input where it is, as predict() does: a NumPy array of float64 / float32 /
float16 at its own width, or any `__dlpack__` object (a PyTorch tensor in host memory or on the
GPU, float64 / float32 / float16 / bfloat16, contiguous or a strided view).  It is widened
exactly on the device (ingest.hip), so the results are bit for bit those of the same values as
a float64 array.  Anything else (lists, integer arrays) is promoted on the host, as always."""

from __future__ import annotations

import contextlib
import ctypes
import typing
from dataclasses import dataclass

import numpy as np

from spectralcluster_amd import _dlpack
from spectralcluster_amd import _lib

_FLOAT_DTYPES = (np.dtype(np.float64), np.dtype(np.float32), np.dtype(np.float16))


def _describe(embeddings) -> typing.Optional[_dlpack.Source]:
  """The `_dlpack.Source` of an input that is read where it lies -- a 2-D float64 / float32 /
  float16 ndarray with its strides, or a DLPack object -- or None for anything else, which is
  promoted to a host float64 array.  release() it when the library call has returned."""
  if isinstance(embeddings, np.ndarray):
    if embeddings.ndim != 2 or embeddings.dtype not in _FLOAT_DTYPES:
      return None
  elif not (hasattr(embeddings, "__dlpack__") and hasattr(embeddings, "__dlpack_device__")):
    return None
  return _dlpack.describe(embeddings, _lib.default_handle, strided=True)


def _input(source: typing.Optional[_dlpack.Source], embeddings):
  """What the library call is handed: the C-contiguous float64 ndarray of the `double*` entry
  points where the input is one (or is promoted to one), else the described source."""
  if source is None:
    return np.ascontiguousarray(embeddings, dtype=np.float64)
  if source.numpy is not None and source.is_host_f64:
    return source.keep
  return source


def _host_rows(source: _dlpack.Source, idx: np.ndarray) -> np.ndarray:
  """Rows `idx` of a described source as a host float64 array: one (1, dim) descriptor per row
  through `sc_stage_ingest`, nothing else of the source is read."""
  a = source.array
  itemsize = {_lib.SC_DTYPE_F64: 8, _lib.SC_DTYPE_F32: 4}.get(a.dtype, 2)
  out = np.empty((len(idx), int(a.cols)), dtype=np.float64)
  handle = _lib.default_handle()
  for i, r in enumerate(idx):
    row = _lib.ScArray(a.data + int(r) * a.row_stride * itemsize, a.dtype, a.location, 1, a.cols,
                       a.row_stride, a.col_stride)
    handle.check(handle.lib.sc_stage_ingest(handle.raw, ctypes.byref(row),
                                            _lib.as_double_p(out[i])))
  return out


def _kmeans_general(e: typing.Union[np.ndarray, _dlpack.Source], n_clusters: int, max_iter: int,
                    metric: int, tol: float, init_centroids: typing.Optional[np.ndarray]):
  """sc_stage_kmeans_general on a C-contiguous float64 (n, dim) array, its `_array` form on a
  described source: (labels, centroids of the last assignment pass, distance passes run)."""
  n, dim = e.shape
  labels = np.empty(n, dtype=np.int64)
  cent = np.empty((n_clusters, dim), dtype=np.float64)
  iters = ctypes.c_int(0)
  init = None
  if init_centroids is not None:
    init = np.ascontiguousarray(init_centroids, dtype=np.float64)
  handle = _lib.default_handle()
  init_p = None if init is None else _lib.as_double_p(init)
  if isinstance(e, _dlpack.Source):
    handle.check(handle.lib.sc_stage_kmeans_general_array(
        handle.raw, ctypes.byref(e.array), int(n_clusters), int(max_iter), metric, float(tol),
        init_p, _lib.as_int64_p(labels), _lib.as_double_p(cent), ctypes.byref(iters)))
  else:
    handle.check(handle.lib.sc_stage_kmeans_general(
        handle.raw, _lib.as_double_p(e), n, dim, int(n_clusters), int(max_iter), metric,
        float(tol), init_p, _lib.as_int64_p(labels), _lib.as_double_p(cent),
        ctypes.byref(iters)))
  return labels, cent, iters.value


def run_kmeans(spectral_embeddings, n_clusters: int,
               custom_dist: typing.Union[str, typing.Callable],
               max_iter: int) -> np.ndarray:
  """k-means++ (sklearn `RandomState(0)` stream) + one Lloyd step for the seeds, then the
  reference's custom-distance loop (custom_distance_kmeans.py:39-51, 85-141).  A falsy
  `custom_dist` raises NotFittedError, as the reference does (it predicts with an unfitted
  sklearn KMeans, :33-36, :51)."""
  metric = _lib.kmeans_metric_code(custom_dist)
  source = _describe(spectral_embeddings)
  with source or contextlib.nullcontext():
    e = _input(source, spectral_embeddings)
    if len(e.shape) != 2:
      raise ValueError("spectral_embeddings must be 2-dimensional")
    n, k = e.shape
    if k != n_clusters:
      # any other width: the general form (CustomKMeans' default tol, :36-50)
      return _kmeans_general(e, n_clusters, max_iter, metric, 0.001, None)[0]
    labels = np.empty(n, dtype=np.int64)
    iters = ctypes.c_int(0)
    handle = _lib.default_handle()
    if isinstance(e, _dlpack.Source):
      handle.check(handle.lib.sc_stage_kmeans_metric_array(
          handle.raw, ctypes.byref(e.array), int(max_iter), metric, _lib.as_int64_p(labels),
          None, ctypes.byref(iters)))
    else:
      handle.check(handle.lib.sc_stage_kmeans_metric(
          handle.raw, _lib.as_double_p(e), n, int(n_clusters), int(max_iter), metric,
          _lib.as_int64_p(labels), None, ctypes.byref(iters)))
    return labels


def _custom_metric_code(custom_dist) -> int:
  """SC_KMEANS_* for CustomKMeans.custom_dist, which the reference hands straight to scipy's
  cdist (:123-124): scipy's errors for a metric that is neither a name nor a function and for
  the empty name; other scipy metrics and callables are not on the device."""
  if callable(custom_dist):
    raise _lib.UnsupportedOnDeviceError(
        "custom_dist=%r: callables are not on the device" % (custom_dist,))
  if not isinstance(custom_dist, str):
    raise TypeError("2nd argument metric must be a string identifier or a function.")
  if not custom_dist:
    raise ValueError("Unknown Distance Metric: ")
  return _lib.kmeans_metric_code(custom_dist)


@dataclass
class CustomKMeans:
  """Class CustomKMeans performs KMeans clustering (reference custom_distance_kmeans.py:55-141).

  Deviations, as elsewhere in the package: the embeddings are widened to float64 (on the
  device; `predict` takes what `run_kmeans` takes, a tensor on the GPU included); initial
  `centroids` that are not float64 raise UnsupportedOnDeviceError (the reference would round
  every centroid update into their dtype)."""

  # The number of clusters to form.
  n_clusters: typing.Optional[int] = None

  # The cluster centroids. If given, initial centroids are set as
  # the input samples. If not, centroids are randomly initialized.
  centroids: typing.Optional[np.ndarray] = None

  # Maximum number of iterations of the k-means algorithm to run.
  max_iter: int = 10

  # The relative increment in the results before declaring convergence.
  tol: float = 0.001

  # Custom distance measure to use. If a string, "cosine", "euclidean",
  # "mahalanobis", or any other distance functions
  # defined in scipy.spatial.distance can be used.
  custom_dist: typing.Union[str, typing.Callable] = "cosine"

  def _init_centroids(self, embeddings, source: typing.Optional[_dlpack.Source] = None):
    """Compute the initial centroids (the global numpy RNG moves as the reference's does).  Of
    a DLPack source the k chosen rows come to the host, as float64, and nothing else."""
    n_samples = embeddings.shape[0]
    idx = np.random.choice(
        np.arange(n_samples), size=self.n_clusters, replace=False)
    if source is not None and source.numpy is None:
      self.centroids = _host_rows(source, idx)
    else:
      self.centroids = embeddings[idx, :]

  def predict(self, embeddings) -> np.ndarray:
    """Performs the clustering on the device; the final centroids are written back into
    `self.centroids` in place, as the reference updates that array.

    Raises:
      ValueError: if input observations have wrong shape (the reference's messages)
    """
    n_samples, n_features = embeddings.shape
    if self.max_iter <= 0:
      raise ValueError("Number of iterations should be a positive number,"
                       " got %d instead" % self.max_iter)
    if n_samples < self.n_clusters:
      raise ValueError("n_samples=%d should be >= n_clusters=%d" %
                       (n_samples, self.n_clusters))
    drawn = self.centroids is None
    if not drawn:
      n_centroids, c_n_features = self.centroids.shape
      if n_centroids != self.n_clusters:
        raise ValueError("The shape of the initial centroids (%s)"
                         "does not match the number of clusters %d" %
                         (str(self.centroids.shape), self.n_clusters))
      if n_features != c_n_features:
        raise ValueError(
            "The number of features of the initial centroids %d"
            "does not match the number of features of the data %d." %
            (c_n_features, n_features))
      metric = _custom_metric_code(self.custom_dist)
      if not (isinstance(self.centroids, np.ndarray) and self.centroids.dtype == np.float64):
        raise _lib.UnsupportedOnDeviceError(
            "CustomKMeans.centroids of dtype %s: the device path updates float64 centroids "
            "only" % getattr(self.centroids, "dtype", type(self.centroids).__name__))
    source = _describe(embeddings)
    with source or contextlib.nullcontext():
      return self._predict(embeddings, source, drawn, None if drawn else metric)

  def _predict(self, embeddings, source, drawn, metric):
    if drawn:
      self._init_centroids(embeddings, source)
      metric = _custom_metric_code(self.custom_dist)
    e = _input(source, embeddings)
    if drawn:
      # the reference never binds n_centroids on this branch: its first centroid update
      # (:135) raises UnboundLocalError, so only a loop that stops after its first distance
      # pass returns (one pass plus, if the rule does not fire, one update decides it)
      labels, _, passes = _kmeans_general(e, self.n_clusters, 1, metric, self.tol,
                                          self.centroids)
      if passes != 1:
        raise UnboundLocalError(
            "local variable 'n_centroids' referenced before assignment")
      return labels
    labels, cent, _ = _kmeans_general(e, self.n_clusters, self.max_iter, metric, self.tol,
                                      self.centroids)
    np.copyto(self.centroids, cent)
    return labels
