"""K-means on the spectral embedding (mirror of reference
`spectralcluster/custom_distance_kmeans.py`): sklearn's k-means++ seeds + the custom-distance
loop (cosine by default; euclidean, sqeuclidean, cityblock, chebyshev, correlation, braycurtis,
canberra) in HIP kernels.  `run_kmeans` on an (n, n_clusters) embedding (what predict() hands
it) runs the single-kernel form of kmeans.hip / kmeans_chain.hip; any other width, and
`CustomKMeans`, run the general form of kmeans_general.hip."""

from __future__ import annotations

import ctypes
import typing
from dataclasses import dataclass

import numpy as np

from spectralcluster_amd import _lib


def _kmeans_general(e: np.ndarray, n_clusters: int, max_iter: int, metric: int, tol: float,
                    init_centroids: typing.Optional[np.ndarray]):
  """sc_stage_kmeans_general on a C-contiguous float64 (n, dim) array: (labels, centroids of the
  last assignment pass, distance passes run)."""
  n, dim = e.shape
  labels = np.empty(n, dtype=np.int64)
  cent = np.empty((n_clusters, dim), dtype=np.float64)
  iters = ctypes.c_int(0)
  init = None
  if init_centroids is not None:
    init = np.ascontiguousarray(init_centroids, dtype=np.float64)
  handle = _lib.default_handle()
  handle.check(handle.lib.sc_stage_kmeans_general(
      handle.raw, _lib.as_double_p(e), n, dim, int(n_clusters), int(max_iter), metric,
      float(tol), None if init is None else _lib.as_double_p(init), _lib.as_int64_p(labels),
      _lib.as_double_p(cent), ctypes.byref(iters)))
  return labels, cent, iters.value


def run_kmeans(spectral_embeddings: np.ndarray, n_clusters: int,
               custom_dist: typing.Union[str, typing.Callable],
               max_iter: int) -> np.ndarray:
  """k-means++ (sklearn `RandomState(0)` stream) + one Lloyd step for the seeds, then the
  reference's custom-distance loop (custom_distance_kmeans.py:39-51, 85-141).  A falsy
  `custom_dist` raises NotFittedError, as the reference does (it predicts with an unfitted
  sklearn KMeans, :33-36, :51)."""
  metric = _lib.kmeans_metric_code(custom_dist)
  e = np.ascontiguousarray(spectral_embeddings, dtype=np.float64)
  if e.ndim != 2:
    raise ValueError("spectral_embeddings must be 2-dimensional")
  n, k = e.shape
  if k != n_clusters:
    # any other width: the general form (CustomKMeans' default tol, :36-50)
    return _kmeans_general(e, n_clusters, max_iter, metric, 0.001, None)[0]
  labels = np.empty(n, dtype=np.int64)
  iters = ctypes.c_int(0)
  handle = _lib.default_handle()
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

  Deviations, as elsewhere in the package: the embeddings are promoted to float64; initial
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

  def _init_centroids(self, embeddings: np.ndarray):
    """Compute the initial centroids (the global numpy RNG moves as the reference's does)."""
    n_samples = embeddings.shape[0]
    idx = np.random.choice(
        np.arange(n_samples), size=self.n_clusters, replace=False)
    self.centroids = embeddings[idx, :]

  def predict(self, embeddings: np.ndarray) -> np.ndarray:
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
    if drawn:
      self._init_centroids(embeddings)
    else:
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
    e = np.ascontiguousarray(embeddings, dtype=np.float64)
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
    if not (isinstance(self.centroids, np.ndarray) and self.centroids.dtype == np.float64):
      raise _lib.UnsupportedOnDeviceError(
          "CustomKMeans.centroids of dtype %s: the device path updates float64 centroids "
          "only" % getattr(self.centroids, "dtype", type(self.centroids).__name__))
    labels, cent, _ = _kmeans_general(e, self.n_clusters, self.max_iter, metric, self.tol,
                                      self.centroids)
    np.copyto(self.centroids, cent)
    return labels
