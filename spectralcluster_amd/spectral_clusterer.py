"""SpectralClusterer facade: same constructor and predict() surface as the
reference `spectralcluster/spectral_clusterer.py`, with the dense hot path
(affinity -> refinement -> Laplacian -> top-k eigen + eigengap -> cosine k-means)
executed on one MI355X through the C ABI in `include/spectralcluster_amd.h`.

Constraints (`constraint_options` + `predict(embeddings, constraint_matrix)`) run on the
device too; `constraint_matrix` may be a `ConstraintMatrix`, whose
band travels instead of an (n, n) array.  Refinement sequences whose result is not
diagonally similar to a symmetric matrix take the general eigen path (8f-N2);
`max_spectral_size` pre-clusters on the device (cosine complete-linkage AHC) and
`fallback_options` (too-few-embeddings fallback, single-cluster test for min_clusters=1) run
there too (8f-N4).  `custom_dist`: cosine, euclidean (minkowski), sqeuclidean, cityblock,
chebyshev, correlation, braycurtis, canberra and scipy's aliases of them; metrics that need more
than the two vectors and callables are out of the device scope.  Those raise
`UnsupportedOnDeviceError`; nothing silently falls back to the CPU.
"""

from __future__ import annotations

import contextlib
import ctypes
import typing

import numpy as np

from spectralcluster_amd import _batch
from spectralcluster_amd import _dlpack
from spectralcluster_amd import _lib
from spectralcluster_amd import autotune as autotune_lib
from spectralcluster_amd import constraint as constraint_lib
from spectralcluster_amd import custom_distance_kmeans
from spectralcluster_amd import fallback_clusterer
from spectralcluster_amd import laplacian
from spectralcluster_amd import naive_clusterer
from spectralcluster_amd import refinement
from spectralcluster_amd import utils

AutoTune = autotune_lib.AutoTune
AutoTuneProxy = autotune_lib.AutoTuneProxy
LaplacianType = laplacian.LaplacianType
RefinementName = refinement.RefinementName
RefinementOptions = refinement.RefinementOptions
EigenGapType = utils.EigenGapType


class SpectralClusterer:
  """Spectral clustering of speaker embeddings on the GPU.

  Constructor arguments are those of the reference (spectral_clusterer.py:29-46),
  plus `device` (HIP device ordinal; default: LOCAL_RANK or 0).
  """

  def __init__(self,
               min_clusters: typing.Optional[int] = None,
               max_clusters: typing.Optional[int] = None,
               refinement_options: typing.Optional[RefinementOptions] = None,
               autotune: typing.Optional[AutoTune] = None,
               fallback_options=None,
               laplacian_type: typing.Optional[LaplacianType] = None,
               stop_eigenvalue: float = 1e-2,
               row_wise_renorm: bool = False,
               custom_dist: typing.Union[str, typing.Callable] = "cosine",
               max_iter: int = 300,
               constraint_options=None,
               eigengap_type: EigenGapType = EigenGapType.Ratio,
               max_spectral_size: typing.Optional[int] = None,
               affinity_function: typing.Callable = utils.compute_affinity_matrix,
               post_eigen_cluster_function: typing.Callable = (
                   custom_distance_kmeans.run_kmeans),
               device: typing.Optional[int] = None):
    self.min_clusters = min_clusters
    self.max_clusters = max_clusters
    self.refinement_options = refinement_options or RefinementOptions()
    self.autotune = autotune
    self.fallback_options = fallback_options or fallback_clusterer.FallbackOptions()
    self.laplacian_type = laplacian_type
    self.row_wise_renorm = row_wise_renorm
    self.stop_eigenvalue = stop_eigenvalue
    self.custom_dist = custom_dist
    self.max_iter = max_iter
    self.constraint_options = constraint_options
    self.eigengap_type = eigengap_type
    self.max_spectral_size = max_spectral_size
    self.affinity_function = affinity_function
    self.post_eigen_cluster_function = post_eigen_cluster_function
    self.device = device
    self.last_diag: typing.Optional[_lib.ScDiag] = None
    # one route code per utterance of the last predict_batch (None before the first)
    self.last_batch_routes: typing.Optional[typing.List[int]] = None
    # after a min_clusters = 1 batch that ran as ONE sc_predict_batch_single call: per utterance,
    # did the single-cluster test find one cluster?  None after any other batch call
    self.last_batch_single: typing.Optional[typing.List[bool]] = None
    # what each utterance of the last size-reducing predict_batch was (`_lib.BATCH_KIND_*`)
    self.last_batch_reduced: typing.Optional[typing.List[int]] = None
    # not in the reference: restart cycles block Lanczos may spend before the dense
    # eigensolver takes over (0 = the library default, 40); predict() returns either way
    self.eig_max_cycles = 0
    # not in the reference: bound on |eigenvalue error| / |eigenvalue| for the values the
    # eigengap rule reads (0 = the library default, 1e-6; the parity bar is 1e-5)
    self.eig_value_tol = 0.0
    # not in the reference: route of a Diffuse that only feeds RowWiseNormalize / the Laplacian
    # (sc_config.diffuse_mode): 0 default (matrix-free from n = 2048 on), 1 explicit fp64
    # product, 2 matrix-free wherever the sequence allows it.  Same results to summation order.
    self.diffuse_mode = 0

  # ----------------------------------------------------------------- plumbing
  def _handle(self) -> _lib.Handle:
    return _lib.default_handle(self.device)

  def build_config(self, p_percentile: typing.Optional[float] = None) -> _lib.ScConfig:
    """Flatten the constructor arguments into an `sc_config`."""
    cfg = _lib.ScConfig()
    _lib.load().sc_config_default(cfg)
    self.refinement_options.to_config(cfg)
    if p_percentile is not None:
      cfg.p_percentile = float(p_percentile)
    if self.laplacian_type is None:
      cfg.laplacian_type = 0
    elif isinstance(self.laplacian_type, LaplacianType):
      cfg.laplacian_type = self.laplacian_type.value
    else:
      raise TypeError("laplacian_type must be a LaplacianType")
    if not isinstance(self.eigengap_type, EigenGapType):
      raise TypeError("eigengap_type must be a EigenGapType")
    cfg.eigengap_type = self.eigengap_type.value
    cfg.min_clusters = int(self.min_clusters or 0)
    cfg.max_clusters = int(self.max_clusters or 0)
    cfg.stop_eigenvalue = float(self.stop_eigenvalue)
    cfg.row_wise_renorm = int(bool(self.row_wise_renorm))
    cfg.max_iter = int(self.max_iter)
    cfg.eig_max_cycles = int(getattr(self, "eig_max_cycles", 0) or 0)
    if getattr(self, "eig_value_tol", 0.0):
      cfg.eig_value_tol = float(self.eig_value_tol)
    cfg.diffuse_mode = int(getattr(self, "diffuse_mode", 0) or 0)
    if self.post_eigen_cluster_function is custom_distance_kmeans.run_kmeans:
      cfg.kmeans_metric = _lib.kmeans_metric_code(self.custom_dist)
    if self.constraint_options is not None:
      self.constraint_options.to_config(cfg)
    if getattr(cfg, "_blur_ext", None) is not None:  # sigma > 8: weights go to the handle
      _lib.sync_blur_weights(self._handle(), cfg)
    return cfg

  def _set_constraint(self, handle: _lib.Handle, n: int, constraint_matrix) -> bool:
    """Make `constraint_matrix` resident (or clear a stale one).  Like the reference
    (spectral_clusterer.py:137-142, 259-264) it is used only when both
    `constraint_options` and the matrix are given.  A `ConstraintMatrix` goes up as its band
    of n - 1 values (`sc_set_constraint_band`), a `PairwiseConstraints` as its directed entries
    (`sc_set_constraint_pairs`), a `DenseConstraints` is read where it is
    (`sc_set_constraint_array`), anything else goes up as a dense (n, n) float64 host array."""
    if self.constraint_options is None or constraint_matrix is None:
      handle.check(handle.lib.sc_clear_constraint(handle.raw))
      return False
    if isinstance(constraint_matrix, constraint_lib.PairwiseConstraints):
      _batch.check_constraint(self, n, constraint_matrix)
      rows, cols, vals = constraint_matrix.entries()
      handle.check(handle.lib.sc_set_constraint_pairs(
          handle.raw, _lib.as_int32_p(rows), _lib.as_int32_p(cols), _lib.as_double_p(vals),
          len(vals), n))
      return True
    if isinstance(constraint_matrix, constraint_lib.DenseConstraints):
      _batch.check_constraint(self, n, constraint_matrix)
      with _lib.use_device(self.device):
        with constraint_matrix.describe(self._handle) as source:
          handle.check(handle.lib.sc_set_constraint_array(
              handle.raw, ctypes.byref(source.array)), TypeError)
      return True
    if isinstance(constraint_matrix, constraint_lib.ConstraintMatrix):
      _batch.check_constraint(self, n, constraint_matrix)
      band = np.ascontiguousarray(constraint_matrix.band(), dtype=np.float64)
      handle.check(handle.lib.sc_set_constraint_band(handle.raw, _lib.as_double_p(band), n))
      return True
    con = np.asarray(constraint_matrix)
    _batch.check_constraint(self, n, con)
    con = np.ascontiguousarray(con, dtype=np.float64)
    handle.check(handle.lib.sc_set_constraint(handle.raw, _lib.as_double_p(con), n))
    return True

  def _upload(self, handle: _lib.Handle, embeddings):
    """Embeddings (anything predict() takes, or an already described `_dlpack.Source`) ->
    resident affinity (device GEMM, or the user's function, which gets them as a host array)."""
    if not isinstance(embeddings, _dlpack.Source):
      with _dlpack.describe(embeddings, lambda: handle) as source:
        return self._upload(handle, source)
    source = embeddings
    if self.affinity_function is utils.compute_affinity_matrix:
      handle.check(handle.lib.sc_set_embeddings_array(handle.raw, ctypes.byref(source.array)))
      handle.check(handle.lib.sc_compute_affinity(handle.raw))
    else:
      # what the user's function returns is read where it is (sc_set_affinity_array): a float64
      # host array as before, but also float32 / float16 / bfloat16 or a tensor on the GPU
      a = self.affinity_function(source.host_f64(handle))
      if not isinstance(a, np.ndarray) and not hasattr(a, "__dlpack__"):
        a = np.asarray(a, dtype=np.float64)
      with _dlpack.describe(a, lambda: handle, strided=True) as affinity:
        handle.check(handle.lib.sc_set_affinity_array(handle.raw, ctypes.byref(affinity.array)))

  def _eig_resident(self, handle: _lib.Handle, p_percentile=None) -> _lib.ScDiag:
    diag = _lib.ScDiag()
    cfg = self.build_config(p_percentile)
    handle.check(handle.lib.sc_eig_ncluster(handle.raw, cfg, diag), TypeError)
    self.last_diag = diag
    return diag

  def _eig_sweep(self, handle: _lib.Handle,
                 p_values: typing.Sequence[float]) -> typing.List[_lib.ScDiag]:
    """`_eig_resident` for every p of one AutoTune level (no eigenvectors left resident)."""
    count = len(p_values)
    diags = (_lib.ScDiag * count)()
    ps = (ctypes.c_double * count)(*[float(p) for p in p_values])
    handle.check(handle.lib.sc_eig_ncluster_sweep(handle.raw, self.build_config(), ps, count,
                                                  diags), TypeError)
    self.last_sweep_diags = list(diags)
    self._last_sweep_ps = [float(p) for p in p_values]
    return self.last_sweep_diags

  def _adopt_or_evaluate(self, handle: _lib.Handle, p: float) -> _lib.ScDiag:
    """Make the eigenvectors for p_percentile `p` resident: adopted from the last sweep when
    `p` was one of its values (the AutoTune winner normally is: the reference keeps the
    winner's eigenvectors from the search, spectral_clusterer.py:274-292), evaluated with
    `_eig_resident` otherwise."""
    ps = getattr(self, "_last_sweep_ps", None)
    if ps and float(p) in ps:
      diag = _lib.ScDiag()
      if handle.lib.sc_sweep_adopt(handle.raw, self.build_config(p), ps.index(float(p)),
                                   diag) == _lib.SC_OK:
        self.last_diag = diag
        return diag
    return self._eig_resident(handle, p)

  def consumed_eigenvalues(self) -> np.ndarray:
    """Every eigenvalue the last eigen call consumed, in the reference's order
    (`compute_sorted_eigenvectors`, utils.py:62-70): max_clusters + 1 of them, or all n
    with max_clusters=None and a Laplacian (`last_diag.eigenvalues` holds at most 128)."""
    handle = self._handle()
    count = handle.lib.sc_num_eigenvalues(handle.raw)
    out = np.empty(count, dtype=np.float64)
    handle.check(handle.lib.sc_get_eigenvalues(handle.raw, _lib.as_double_p(out), count))
    return out

  def _download_eigenvectors(self, handle: _lib.Handle, n: int,
                             cols: typing.Optional[int] = None) -> np.ndarray:
    have = handle.lib.sc_num_eigenvectors(handle.raw)
    cols = have if cols is None else cols
    out = np.empty((n, cols), dtype=np.float64)
    handle.check(handle.lib.sc_get_eigenvectors(handle.raw, _lib.as_double_p(out), n,
                                                cols))
    return out

  # ------------------------------------------------------------- reference API
  def _compute_eigenvectors_ncluster(
      self, affinity: np.ndarray, constraint_matrix=None
  ) -> typing.Tuple[np.ndarray, int, float]:
    """Refinement + eigen-decomposition + eigengap for a given affinity matrix
    (reference spectral_clusterer.py:108-168).

    Returns (eigenvectors, n_clusters, max_delta_norm).  For n <= 128 the
    eigenvector matrix is (n, n) like the reference's; above that it has only the
    columns the eigengap search can select (max_clusters + 1, at most 64 from a Krylov solve;
    on the dense routes -- max_clusters=None with a Laplacian, where every eigenvalue is read,
    more than 64 selected clusters, the general path up to n = 512 -- the
    max(n_clusters, min_clusters) columns predict() uses).
    """
    a = np.ascontiguousarray(affinity, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
      raise ValueError("affinity must be a square matrix")
    handle = self._handle()
    handle.check(handle.lib.sc_set_affinity(handle.raw, _lib.as_double_p(a), a.shape[0]))
    # only the after-refinement branch lives in this method (reference :137-142)
    self._set_constraint(handle, a.shape[0], constraint_matrix)
    diag = self._eig_resident(handle)
    vectors = self._download_eigenvectors(handle, a.shape[0])
    return vectors, int(diag.n_clusters_raw), float(diag.max_delta)

  def _reduce_size_and_predict(self, embeddings: np.ndarray) -> np.ndarray:
    """Complete-linkage cosine AHC down to `max_spectral_size` clusters, spectral
    clustering of their centroids, labels chained back (reference :170-199)."""
    ahc_labels = utils.cosine_agglomerative_clustering(
        embeddings, n_clusters=self.max_spectral_size, linkage="complete")
    ahc_centroids = utils.get_cluster_centroids(embeddings, ahc_labels)
    spectral_labels = self.predict(ahc_centroids)
    return utils.chain_labels(ahc_labels, spectral_labels)

  def predict(self, embeddings, constraint_matrix=None, *, out=None) -> np.ndarray:
    """Cluster `embeddings` (n_samples, n_features); returns int64 labels as a host array
    (reference spectral_clusterer.py:201-314).

    `out` (keyword only): a 1-D int64 or int32 array of exactly n entries -- a NumPy array or an
    object with `__dlpack__`, in host memory or on the clusterer's GPU, with a non-negative
    stride -- receives the labels and is returned in the place of the new host array (the
    float64 labels of a size-reduced utterance are converted exactly).  It is validated before
    anything is launched.  The labels still pass through the host inside the call.

    `embeddings`: a NumPy array, or any object with `__dlpack__` / `__dlpack_device__` -- a
    PyTorch tensor, say -- of float64, float32, float16 or bfloat16, in host memory or on the
    clusterer's GPU, contiguous or a strided view.  It is read where it is and widened to
    float64 on the device (exactly: labels and eigenvalues are those of
    `predict(x.astype(np.float64))`).  A device tensor needs no synchronisation by the caller:
    its producer orders its pending writes before the library's stream, and the tensor may be
    overwritten or freed when predict() has returned.

    With `fallback_options.spectral_min_embeddings`, `max_spectral_size` or `min_clusters=1`
    under the `FallbackClusterer` condition, predict() brings a device tensor to the host (up to
    three times when they meet).  `predict_batch([x], batch_multi_stage=True)` runs that regime
    on a single tensor without a host round trip, with the same labels."""
    if out is not None:
      return _batch.labels_into(self, [out], [_batch.rows_of(self, embeddings)],
                                lambda: [self.predict(embeddings, constraint_matrix)])[0]
    with _lib.use_device(self.device):  # helpers without a device argument follow self.device
      with _dlpack.describe(embeddings, self._handle) as source:
        return self._predict(source, constraint_matrix)

  def _predict(self, source: _dlpack.Source, constraint_matrix=None) -> np.ndarray:
    n = source.shape[0]
    if n < self.fallback_options.spectral_min_embeddings:
      # too few embeddings for spectral clustering (reference :229-233)
      return fallback_clusterer.FallbackClusterer(self.fallback_options).predict(
          source.host_f64(self._handle()))
    if self.max_spectral_size is not None and n > self.max_spectral_size:
      # reference spectral_clusterer.py:236-248
      if constraint_matrix is not None:
        raise RuntimeError(
            "Cannot handle constraint_matrix when max_spectral_size is set")
      if _batch.spectral_size_too_small(self):
        raise _batch.small_spectral_size()
      return self._reduce_size_and_predict(source.host_f64(self._handle()))
    handle = self._handle()
    default_tail = (self.post_eigen_cluster_function is custom_distance_kmeans.run_kmeans)
    if default_tail:
      _lib.kmeans_metric_code(self.custom_dist)  # raises for metrics that are not on the device
    constrained = self._set_constraint(handle, n, constraint_matrix)

    single_check = self.min_clusters == 1
    by_fallback = (self.fallback_options.single_cluster_condition ==
                   fallback_clusterer.SingleClusterCondition.FallbackClusterer)
    if single_check and by_fallback:
      # this condition only needs the embeddings; it runs on the same device handle, so
      # it goes first and the affinity is built afterwards (reference :253-256)
      if fallback_clusterer.check_single_cluster(self.fallback_options,
                                                 source.host_f64(handle), None):
        return np.array([0] * n)

    if (self.autotune is None and default_tail and not single_check
        and self.affinity_function is utils.compute_affinity_matrix):
      # the whole path in one call: ingest(X), device pipeline, D2H(labels)
      labels = np.empty(n, dtype=np.int64)
      diag = _lib.ScDiag()
      handle.check(handle.lib.sc_predict_array(
          handle.raw, ctypes.byref(source.array), self.build_config(),
          _lib.as_int64_p(labels), diag), TypeError)
      self.last_diag = diag
      return labels

    self._upload(handle, source)
    return self._predict_resident(handle, n, constrained, single_check and not by_fallback,
                                  default_tail)

  def _predict_resident(self, handle: _lib.Handle, n: int, constrained: bool,
                        affinity_single_check: bool, default_tail: bool) -> np.ndarray:
    """predict() from the resident affinity on (the embeddings' GEMM or a caller's matrix put it
    there): single-cluster test, constraint, AutoTune or one evaluation, the clustering tail."""
    if affinity_single_check:
      # single-vs-multi cluster(s) decision on the resident affinity (reference :253-256; the
      # affinity conditions do not read the embeddings)
      if fallback_clusterer.check_single_cluster(self.fallback_options, None, None,
                                                 _resident_on=handle):
        return np.array([0] * n)
    if constrained and self.constraint_options.apply_before_refinement:
      # reference :259-264 -- once, before the AutoTune sweep re-reads the affinity
      handle.check(handle.lib.sc_apply_constraint(handle.raw, self.build_config()))
    if self.autotune:
      _batch.check_autotune_sequence(self)
      evaluated = []

      def evaluate_level(ps):
        # one search level = one library call: the values of a level differ only in the row
        # threshold, the device evaluates them as a group (sc_eig_ncluster_sweep)
        diags = self._eig_sweep(handle, ps)
        evaluated.extend(ps)
        return [(self.autotune.ratio(p, d.max_delta), p, int(d.n_clusters_raw))
                for p, d in zip(ps, diags)]

      _, n_clusters, best_p = self.autotune.tune(None, evaluate_many=evaluate_level)
      # reference closure leaves refinement_options.p_percentile at the LAST
      # evaluated value (spectral_clusterer.py:277); keep that observable state
      self.refinement_options.p_percentile = evaluated[-1]
      self.last_best_p = best_p  # (not in the reference: the value the labels come from)
      diag = self._adopt_or_evaluate(handle, best_p)  # the winner's vectors, resident
    else:
      diag = self._eig_resident(handle)
      n_clusters = int(diag.n_clusters_raw)

    if self.min_clusters is not None:
      n_clusters = max(n_clusters, self.min_clusters)

    if default_tail:
      labels = np.empty(n, dtype=np.int64)
      handle.check(handle.lib.sc_cluster(handle.raw, self.build_config(), n_clusters,
                                         _lib.as_int64_p(labels), diag))
      return labels
    # user-supplied post_eigen_cluster_function: hand it the spectral embedding
    spectral = self._download_eigenvectors(handle, n, n_clusters)
    if self.row_wise_renorm:
      spectral = spectral / np.linalg.norm(spectral, axis=1, ord=2)[:, None]
    return self.post_eigen_cluster_function(
        spectral_embeddings=spectral, n_clusters=n_clusters,
        custom_dist=self.custom_dist, max_iter=self.max_iter)

  # ------------------------------------------------- an affinity the caller holds
  def _check_affinity_input(self, affinity, what: str = "affinity") -> int:
    """The ValueErrors of predict_affinity that need no device: a matrix that is not 2-D or not
    square, and the options that read embeddings.  Returns n."""
    n = constraint_lib.check_square_input(affinity, what)
    if n < self.fallback_options.spectral_min_embeddings:
      raise ValueError(
          "fallback_options.spectral_min_embeddings = %d is above n = %d: the fallback clusterer "
          "reads embeddings, which predict_affinity does not have"
          % (self.fallback_options.spectral_min_embeddings, n))
    if self.max_spectral_size is not None and n > self.max_spectral_size:
      raise ValueError(
          "max_spectral_size = %d is below n = %d: the size reduction clusters embeddings, which "
          "predict_affinity does not have" % (self.max_spectral_size, n))
    if (self.min_clusters == 1 and self.fallback_options.single_cluster_condition ==
        fallback_clusterer.SingleClusterCondition.FallbackClusterer):
      raise ValueError(
          "single_cluster_condition = FallbackClusterer with min_clusters = 1 clusters the "
          "embeddings, which predict_affinity does not have: use one of the conditions that "
          "read the affinity")
    return n

  def predict_affinity(self, affinity, constraint_matrix=None, *, out=None) -> np.ndarray:
    """Cluster from an (n, n) affinity the caller already holds -- PLDA or other learned scores,
    raw cosine in [-1, 1], a Gaussian kernel, what a model has just written on the GPU.

    The result is that of `predict(x, constraint_matrix)` on a copy of this clusterer whose
    `affinity_function` is `lambda _: A64`, A64 being `affinity` widened to float64, for any `x`
    of n rows.  `affinity` is whatever predict() takes, but square: a NumPy array or an object
    with `__dlpack__`, in host memory or on the clusterer's GPU, float64 / float32 / float16 /
    bfloat16, contiguous or a strided view (a `.T`, a `[::2, ::2]` slice).  It is read where it
    is and widened exactly on the device; the same kernel pass decides whether it is symmetric.
    A device tensor needs no synchronisation by the caller and may be overwritten or freed when
    the call has returned.  Every Laplacian and eigengap rule, AutoTune, the three constraint
    forms, `min_clusters=1` under the four conditions that read the affinity and a user
    `post_eigen_cluster_function` work as in predict(); without AutoTune, a single-cluster test
    or a user tail it is ONE `sc_predict_affinity_array` call.

    ValueError, before any device is touched: a matrix that is not 2-D or not square, and the
    options that read embeddings -- n below `fallback_options.spectral_min_embeddings`,
    `max_spectral_size` below n, `min_clusters == 1` under the `FallbackClusterer` condition.

    `out` (keyword only): predict()'s -- the labels go into it and it is returned."""
    n = self._check_affinity_input(affinity)
    if out is not None:
      return _batch.labels_into(self, [out], [n],
                                lambda: [self.predict_affinity(affinity, constraint_matrix)])[0]
    with _lib.use_device(self.device):
      with _dlpack.describe(affinity, self._handle, strided=True) as source:
        handle = self._handle()
        default_tail = (self.post_eigen_cluster_function is custom_distance_kmeans.run_kmeans)
        if default_tail:
          _lib.kmeans_metric_code(self.custom_dist)  # raises for metrics not on the device
        constrained = self._set_constraint(handle, n, constraint_matrix)
        single_check = self.min_clusters == 1
        if self.autotune is None and default_tail and not single_check:
          labels = np.empty(n, dtype=np.int64)
          diag = _lib.ScDiag()
          handle.check(handle.lib.sc_predict_affinity_array(
              handle.raw, ctypes.byref(source.array), self.build_config(),
              _lib.as_int64_p(labels), diag), TypeError)
          self.last_diag = diag
          return labels
        handle.check(handle.lib.sc_set_affinity_array(handle.raw, ctypes.byref(source.array)))
        return self._predict_resident(handle, n, constrained, single_check, default_tail)

  def predict_affinity_batch(self, affinities: typing.Sequence,
                             constraint_matrices: typing.Optional[typing.Sequence] = None,
                             group: typing.Optional[int] = None,
                             *,
                             batch_any_metric: bool = False,
                             out: typing.Optional[typing.Sequence] = None
                             ) -> typing.List[np.ndarray]:
    """`[predict_affinity(a, c) for a, c in zip(affinities, constraint_matrices)]`; host and
    device matrices of any of the four dtypes may be mixed.

    Every check of predict_affinity, the length of `constraint_matrices` and the size of each
    `ConstraintMatrix` / `PairwiseConstraints` are made for the whole list before anything is
    launched.  The batch is the `predict_affinity_batch` row of predict_batch's table: ONE
    `sc_predict_batch_affinities` call when the clusterer is one `_library_batch_covers()`
    accepts but for its `affinity_function` (no AutoTune, `min_clusters` not 1, the default
    k-means function), the metric is on the device (cosine when constraints travel), `group` is
    not 1 and every constraint is a `ConstraintMatrix`, a `PairwiseConstraints`, a
    `DenseConstraints` (then `sc_predict_batch_constraint_arrays`) or None.  It takes
    `predict_batch`'s routes -- n <= 128 in Jacobi waves (route 2), 128 < n < 4096 in lockstep
    groups of up to `group` (route 1), n >= 4096 and members that leave their route as single
    calls inside the call (route 0) -- with one grouped ingest launch per group or wave and the
    member-by-member refinement front; results agree with predict_affinity as predict_batch's do
    with predict() (labels equal unless an eigengap decision is a near tie, eigenvalues within
    1e-10 relative on route 2 and 1e-6 on route 1), and the same list gives the same results.
    With a device tensor in the list the library synchronises its stream once at entry; the
    tensors may be overwritten or freed when the call has returned.  Otherwise -- AutoTune,
    `min_clusters=1`, a user k-means function, a raw dense ndarray constraint, `group=1` -- the
    matrices run one after the other through predict_affinity (routes all 0).
    `last_batch_routes` / `last_batch_diags` are filled as in predict_batch.

    `batch_any_metric` (keyword only, default False): predict_batch's flag.  With it a
    `custom_dist` other than cosine that is on the device takes routes 1 and 2 as cosine does,
    constrained or not; see there for how the labels then compare with predict_affinity's.

    `out` (keyword only): predict_batch's -- one label destination per matrix."""
    count = len(affinities)
    _batch.check_length(constraint_matrices, count)
    if constraint_matrices is None:
      constraint_matrices = [None] * count
    if group is not None and int(group) < 1:
      raise ValueError("group must be at least 1")
    for i, (a, cm) in enumerate(zip(affinities, constraint_matrices)):
      n = self._check_affinity_input(a, "affinity %d" % i)
      if self.constraint_options is not None and isinstance(cm, _batch.BATCH_CONSTRAINTS):
        _batch.check_constraint(self, n, cm)
    self.last_batch_single = None
    form = _batch.Form.make(group, None)
    flags = _batch.Flags(any_metric=batch_any_metric)
    with self._permission_if(_batch.wants_permission(self, form, flags)):
      plan = _batch.plan_affinity(self, form, constraint_matrices, count)
      return _batch.execute(self, plan, form, affinities, out)

  # -------------------------------------------------------------- batch (new)
  def predict_batch(self, utterances: typing.Sequence,
                    streams: typing.Optional[int] = None,
                    group: typing.Optional[int] = None,
                    constraint_matrices: typing.Optional[typing.Sequence] = None,
                    autotune_from_entry_state: bool = False,
                    batch_fallback_condition: bool = False,
                    batch_naive_fallback: bool = False,
                    *,
                    batch_multi_stage: bool = False,
                    batch_any_metric: bool = False,
                    out: typing.Optional[typing.Sequence] = None
                    ) -> typing.List[np.ndarray]:
    """Independent predict() calls (the reference has no batch API: a batch is a
    Python loop).

    Small utterances cannot fill 256 CUs, and their pipeline is a chain of short dependent
    launches.  Two ways around that, both ONE library call with the GIL released:
      group       `sc_predict_batch_grouped` (the default, group=16): `group` (<= 16)
                  utterances per launch -- the eigensolver and k-means chains of a group
                  advance in lockstep on one stream while the GEMMs and refinement passes of
                  the next group run on another; the groups are dealt to three lanes (a host
                  thread and a set of streams each) inside the call.  That is the route of
                  128 < n < 4096; utterances of n <= 128 take the short route of the same
                  call (the dense Jacobi eigensolver, one workgroup per utterance, up to 64
                  utterances per launch, then the lockstep k-means), and n >= 4096, a
                  full-spectrum request above 128, or a member that leaves its route run as
                  single calls inside it;
      streams     `sc_predict_batch_streams` (when `streams` is given and `group` is not):
                  the batch spread (longest-processing-time first) over `streams` HIP
                  streams, one host thread and arena per stream; streams=1 is a plain loop.
    Per-utterance results agree with predict() to the solver's tolerance, not bit for bit:
    the grouped GEMMs sum K in whole tiles where a short single call splits K, and the
    lockstep eigensolver checks convergence on the group's schedule, so a member can leave
    with a different basis size (eigenvalues within 1e-6 relative, labels equal unless an
    eigengap decision is a near tie; an utterance of n <= 128 runs the kernel body of its own
    predict(): eigenvalues within 1e-10 relative).  A batch call is deterministic: the same
    list gives the same results.

    `last_batch_routes` (a list of ints, one per utterance) says what ran after the grouped and
    the streams forms: 0 the single-call path, 1 the grouped block Lanczos, 2 the grouped short
    route (`_lib.BATCH_ROUTE_*`).

    An utterance is whatever predict() takes: NumPy arrays and DLPack objects (device tensors,
    float64 / float32 / float16 / bfloat16) may be mixed.  With a device tensor in the batch the
    library synchronises its own stream once at entry -- the producers have ordered their work
    before it -- and the streams of the batch read the tensors from then on; they may be
    overwritten or freed when the call has returned.

    How a batch chooses its call (`_batch.plan`; `tests/golden/batch_dispatch.json` records it
    case by case).  THE LIBRARY-BATCH FORM, which every one-call regime below needs: `streams`
    is not given and `group` is not 1 (the grouped form); there is no AutoTune (but for the first
    row); the affinity and k-means functions are the default ones; k-means is the cosine one
    (with `batch_any_metric`: any metric on the device).  The first row that applies is taken:

      call (sc_predict_batch_...)   regime                              flag it needs               what keeps the loop
      ----------------------------  ----------------------------------  --------------------------  ---------------------------------
      _autotune                     a clusterer with AutoTune           autotune_from_entry_state   a metric other than cosine, a
                                                                                                    constraint that is no
                                                                                                    ConstraintMatrix (on copies of
                                                                                                    the AutoTune object); without
                                                                                                    the flag: the order-dependent loop
      _multi_stage                  min_clusters=1 with                 batch_multi_stage           constraint_matrices given,
                                    max_spectral_size and / or                                      max_spectral_size below
                                    spectral_min_embeddings > 1                                     spectral_min_embeddings
      _single_fallback              min_clusters=1, the                 batch_fallback_condition    the Naive type, constraints,
                                    FallbackClusterer condition,                                    max_spectral_size,
                                    Agglomerative type                                              spectral_min_embeddings > 1
      _single_naive                 the same, Naive type                batch_fallback_condition    as above
                                                                        and batch_naive_fallback
      _single                       min_clusters=1, a condition         --                          constraints, the two size
                                    that reads the affinity                                         options
      _constrained, _constraints,   constraint_options and              --                          a raw ndarray among the
      _constraint_arrays            constraint_matrices                                             entries, min_clusters=1, the
                                                                                                    two size options
      _reduced                      max_spectral_size and / or          --                          the Naive type for a fallback
                                    spectral_min_embeddings > 1,                                    utterance, min_clusters=1,
                                    min_clusters not 1                                              max_spectral_size below
                                                                                                    spectral_min_embeddings
      _reduced_naive                the same, a fallback utterance      batch_naive_fallback        as above
                                    meeting the Naive type
      _grouped, _streams, _arrays   every other clusterer the library   --                          (user functions, AutoTune, the
                                    batch covers; any form                                          fallback decisions: the loop)
      _affinities,                  predict_affinity_batch              --                          see there
      _constraint_arrays

    The loop is per-utterance `predict(u, c)` calls (routes all 0); `group=1` and `streams` keep
    it for every row but the plain one, and so does a metric other than cosine without
    `batch_any_metric`.  The rows, in that order:

    `autotune_from_entry_state` (a clusterer without AutoTune ignores it).  `AutoTune.tune`
    leaves the object's range and step narrowed, so the default loop searches utterance i + 1 on
    the grid utterance i left behind: results depend on the order of the batch.  With the flag
    every utterance is searched from the state the `AutoTune` object has when the call is
    entered -- what a fresh clusterer per utterance gives -- and the object is left as it was
    found.  The missing-RowWiseThreshold ValueError and the ValueError of a `ConstraintMatrix`
    of the wrong length are raised before anything is launched.  Afterwards `last_batch_best_p`
    holds the winning p_percentile per utterance, `last_batch_diags` the winner's diagnostics,
    and `refinement_options.p_percentile` the last value evaluated for the last utterance.  It
    is ONE `sc_predict_batch_autotune` call in the library-batch form when the metric is cosine
    (this row ignores `batch_any_metric`) and every constraint is a `ConstraintMatrix` or None:
    utterances of n <= 128 in waves whose (utterance, p) pairs
    share one front launch and one Jacobi launch per 64 pairs and level (route 2), 128 < n < 4096
    dealt to three lanes that each run the per-utterance search on a handle, stream and thread
    of their own (route 1), the rest per utterance on the caller's handle (route 0).  Otherwise
    -- a dense ndarray constraint among them -- every utterance runs predict() on a copy of the
    AutoTune object (routes all 0), with the same results.

    `batch_multi_stage` (keyword only; default False: the loop).
    The three options of a robust offline diarizer together -- `max_spectral_size` and / or
    `fallback_options.spectral_min_embeddings` above 1, with `min_clusters=1` -- are ONE
    `sc_predict_batch_multi_stage` call in the library-batch form when no `constraint_matrices`
    are given and `max_spectral_size >= spectral_min_embeddings` when both are set.
    Any of the five single-cluster conditions and either fallback type is
    taken; `batch_fallback_condition` / `batch_naive_fallback` are not needed as well.  Per
    utterance, in predict()'s order: fewer than `spectral_min_embeddings` rows, the fallback
    clusterer's labels and no single-cluster test; more than `max_spectral_size` rows,
    complete-linkage pre-clustering, then what predict() does with the centroids -- which stay on
    the device --, their single-cluster test included; otherwise the single-cluster test and the
    spectral path.  Results have predict()'s dtypes: float64 for a size-reduced utterance (zeros
    when its centroids hold one cluster), `np.array([0] * n)` for an utterance of one cluster,
    int64 otherwise.  Afterwards `last_batch_reduced` holds the kinds, `last_batch_single` True /
    False / None (None: a fallback utterance, not tested), `last_batch_routes` the route of the
    spectral run (under the `FallbackClusterer` condition 3 for an utterance found single; 3 for a
    fallback utterance) and `last_batch_diags` its diagnostics (zeroed for single and fallback
    utterances).  predict()'s ValueErrors -- `max_spectral_size` not above `max_clusters` /
    `min_clusters`, an agglomerative utterance of one row, an AffinityGmmBic diagonal offset that
    is not below the tested rows - 1, a threshold pair `NaiveClusterer` rejects -- are raised,
    with the utterance's index, before anything is launched.  A batch of one utterance is
    covered.  Without the flag, and for every other clusterer, nothing changes.

    `batch_fallback_condition` (default False: the loop).  With it a `min_clusters=1`
    batch under the `FallbackClusterer` condition -- what `MultiStageClusterer`'s constructor
    sets -- is ONE `sc_predict_batch_single_fallback` call in the library-batch form when the
    fallback type is `Agglomerative`, the batch is unconstrained, and there is no
    `max_spectral_size` and no `spectral_min_embeddings` above 1.  The
    verdicts of the whole batch are computed first -- "does average-linkage cosine AHC, cut at
    `agglomerative_threshold`, leave one cluster?", a wavefront or a workgroup per utterance, no
    merge list downloaded --, then one grouped batch clusters the utterances of several clusters
    from the rows the verdict waves left on the device.  Results are predict()'s:
    `np.array([0] * n)` for an utterance of one cluster (route 3, a zeroed diag), int64 labels
    otherwise (route 0, 1 or 2); `last_batch_single` lists the verdicts.  An utterance of one
    row raises predict()'s ValueError before anything is launched, one with a zero or non-finite
    row a ValueError that names its index.  Anything else keeps the loop, flag or no flag.

    `batch_naive_fallback` (default False: the `Naive` fallback type -- what a default
    `FallbackOptions` selects -- keeps the loop in the fallback-condition and the reduced
    regimes).  With it
      * a batch that is the `sc_predict_batch_reduced` call but for a fallback utterance meeting
        the `Naive` type is ONE `sc_predict_batch_reduced_naive` call: the fallback utterances
        are walked by the naive clusterer from the empty state, a workgroup each in one launch
        per wave, with `naive_threshold` / `naive_adaptation_threshold` (None: the threshold).
        `last_batch_reduced`, `last_batch_routes` (3 for a fallback utterance), `last_batch_diags`
        and the result dtypes are as in the reduced regime; a fallback utterance of one row is
        fine (label 0);
      * together with `batch_fallback_condition`, a `min_clusters=1` batch under the
        `FallbackClusterer` condition with the `Naive` type is ONE `sc_predict_batch_single_naive`
        call under every other clause of that flag: the verdict of an utterance is "the naive walk
        ends with one centroid", and its work ends at the row that would open a second one.  An
        utterance of one row is single; one with a zero or non-finite row raises a ValueError that
        names its index.
    Labels equal predict()'s: the batch kernel shares its arithmetic with the one predict() runs.
    A threshold pair that `NaiveClusterer` rejects raises its ValueError before anything is
    launched.  With the `Agglomerative` type the flag does nothing.

    `min_clusters=1` (the streaming regime: the clusterer may say "one speaker"): the batch is
    ONE `sc_predict_batch_single` call in the library-batch form when
    `fallback_options.single_cluster_condition` is one of the four that read the affinity
    (AffinityGmmBic, AllAffinity, NeighborAffinity, AffinityStd) and the batch is
    unconstrained.  The
    single-cluster test of every utterance runs on the device inside the call, group by group and
    wave by wave, before the utterance's eigensolver.  Results are predict()'s:
    `np.array([0] * n)` for an utterance of one cluster, int64 labels otherwise;
    `last_batch_single` lists the verdicts (None after a call that did not take this path) and
    `last_batch_routes` the route each utterance's affinity took (0, 1 or 2).  With
    AffinityGmmBic an utterance of `single_cluster_affinity_diagonal_offset >= n - 1` raises
    predict()'s ValueError, with the utterance's index, before anything is launched.  These keep
    the per-utterance loop (routes all 0) with `min_clusters=1`: the `FallbackClusterer` condition
    (it clusters the embeddings, not the affinity; see `batch_fallback_condition`), constrained
    batches, AutoTune batches, and batches with `max_spectral_size` / `spectral_min_embeddings`
    (but see `batch_multi_stage`).

    `constraint_matrices`: one `ConstraintMatrix` / ndarray / None per utterance, used when
    `constraint_options` is set (without it a batch carries no constraints); a list that is not
    as long as the batch raises a ValueError.  When every entry
    is a `ConstraintMatrix` or None and the batch is in the library-batch form, it is ONE
    `sc_predict_batch_constrained` call:
    the same routes as an unconstrained batch, each utterance's band (`ConstraintMatrix.band()`,
    n - 1 values) resident in its member arena.  ConstraintPropagation before refinement then runs
    as one chain of grouped launches per group of up to 16 utterances; AffinityIntegration and
    the after-refinement operators run per utterance inside the group's front; an utterance
    whose entry is None is clustered as in a batch without constraints.  A `ConstraintMatrix`
    whose length is not its utterance's raises the ValueError of predict() before anything is
    launched.  `PairwiseConstraints` entries are taken in the same way, in any mix with the
    other two: with one among them the call is `sc_predict_batch_constraints`, each list (K
    directed entries, 16 bytes each) resident in its member arena, the last stage of the chain
    run once for the band members and once for the pair members of a group; a list of more
    entries than its utterance has rows runs that utterance as a single call (route 0), and one
    whose n is not its utterance's raises predict()'s ValueError before anything is launched.
    `DenseConstraints` entries travel too (`sc_predict_batch_constraint_arrays`): their matrices
    are read where they are, widened into the member arenas by one grouped launch per 64 of a
    group or wave, and take the dense arithmetic -- inside the group's chain for a symmetric
    matrix on a symmetric affinity, the member's own operator otherwise; one whose n is not its
    utterance's raises the same ValueError before anything is launched.
    Anything else -- a raw dense ndarray among the entries, AutoTune (the Turn-to-Diarize
    preset), group=1, `streams` -- runs as per-utterance `predict(u, c)` calls (routes all 0).

    `max_spectral_size` and `fallback_options.spectral_min_embeddings` (the multi-stage
    regime): the batch is ONE `sc_predict_batch_reduced` call in the library-batch form when
    `min_clusters` is not 1, no constraint matrices travel, the fallback -- if an utterance
    needs it -- is the
    agglomerative one, and `max_spectral_size >= spectral_min_embeddings` when both are set.
    The utterances of more than `max_spectral_size` rows are pre-clustered together (complete
    linkage, a workgroup per utterance in one launch per wave), the ones below
    `spectral_min_embeddings` clustered by the fallback together (average linkage), and one
    grouped batch then clusters the centroids of the first kind with the utterances that needed
    neither.  Results are predict()'s -- float64 labels for a size-reduced utterance (the
    reference's `chain_labels`), int64 otherwise.  `last_batch_reduced` lists what each
    utterance was (`_lib.BATCH_KIND_*`: 0 spectral, 1 size-reduced, 2 fallback),
    `last_batch_routes` the route of its spectral run (3, `_lib.BATCH_ROUTE_FALLBACK`, for a
    fallback utterance), `last_batch_diags` that run's diagnostics (zeroed for a fallback
    utterance).  Raised before anything is launched: predict()'s ValueError for a
    `max_spectral_size` that is not above `max_clusters` / `min_clusters`, and for a fallback
    utterance of one row.  An utterance with a zero or non-finite row raises a ValueError that
    names its index.  Everything else -- the `Naive` fallback (but see
    `batch_naive_fallback`), `min_clusters=1` (but see `batch_multi_stage`), constraints,
    AutoTune, `group=1`, `streams` -- stays the per-utterance loop (routes all 0).

    `batch_any_metric` (keyword only; default False).  Wherever the library-batch form says
    "k-means is the cosine one", a `custom_dist` other than cosine keeps the batch out of the
    grouped and short routes: a plain batch is still one library call, but every utterance runs
    as a single call inside it (routes all 0), and the constrained, `min_clusters=1`, reduced,
    fallback-condition, naive and multi-stage batches are the per-utterance loop.  With the
    flag that clause reads "k-means is on the device" -- any `custom_dist` predict() runs there:
    euclidean (minkowski), sqeuclidean, cityblock, chebyshev, correlation, braycurtis, canberra
    -- in every one-call form above but the AutoTune one (`autotune_from_entry_state`), which
    ignores the flag: `last_batch_routes` reports 1 and 2 as for cosine, and the k-means of a
    group is the lockstep chain with the metric's distance in its assignment.  The call gives
    the handle the permission (`sc_set_batch_any_metric`) before the library call and takes it
    back afterwards, also when the call raises.  Results agree with predict() to the statement
    made for the cosine grouped batch at the top.  In addition, for a metric other than cosine
    predict()'s own k-means is another kernel (one workgroup) than the batch's chain, which adds
    the mean distance and the centroid sums in another order: labels are equal unless an
    assignment or the stop rule is a near tie, and that holds on the short route (n <= 128) as
    well, whose eigenvectors are otherwise predict()'s own.  Without the flag, with "cosine",
    or with `group=1` / `streams`, nothing changes; a metric that is not on the device raises
    what predict() raises.

    `out` (keyword only; default None): a list with one entry per utterance, each what
    predict()'s `out` is -- a 1-D int64 / int32 array of exactly n_i entries, NumPy or DLPack,
    host or device, views into one flat tensor included.  All of them are validated before
    anything is launched; after the call, whatever family ran it, the labels are written into
    them in one `sc_labels_egress` call (one upload and one launch for the device destinations)
    and the list of `out` entries is returned.
    """
    self.last_batch_single = None
    form = _batch.Form.make(group, streams)
    flags = _batch.Flags(autotune_from_entry_state, batch_fallback_condition,
                         batch_naive_fallback, batch_multi_stage, batch_any_metric)
    with self._permission_if(_batch.wants_permission(self, form, flags)):
      plan = _batch.plan(self, form, flags, constraint_matrices, utterances)
      return _batch.execute(self, plan, form, utterances, out)

  def predict_device_batch(self, arrays: typing.Sequence[_lib.ScArray],
                           group: int = 16,
                           batch_fallback_condition: bool = False) -> typing.List[np.ndarray]:
    """predict_batch for utterances that are already described (`sc_array`s, e.g. the resident
    centroid buffers of a stream pool) on a clusterer `_library_batch_covers`: one grouped
    library call, `last_batch_routes` / `last_batch_diags` as after predict_batch.
    `batch_fallback_condition`: as predict_batch's, for a clusterer
    `_fallback_condition_covers(min_embeddings_met=True)` (the caller vouches for the rows)."""
    _lib.kmeans_metric_code(self.custom_dist)  # raises for metrics that are not on the device
    self.last_batch_single = None
    plan = _batch.plan_device(self, batch_fallback_condition)
    return _batch.execute_device(self, plan, _batch.Form(True, int(group), 1), arrays)

  def _autotune_library_batch(self, utterances: typing.Sequence,
                              constraint_matrices: typing.Sequence,
                              group: int) -> typing.List[np.ndarray]:
    """ONE `sc_predict_batch_autotune` call; the checks of `_batch.plan` passed."""
    return _batch.autotune_call(self, utterances, constraint_matrices, group)

  # ------------------------------------------- what the plan reads of the clusterer
  def _single_check_struct(self) -> typing.Optional[_lib.ScSingleCheck]:
    """The `sc_single_check` of this clusterer's single-cluster test, or None when the condition
    does not read the affinity (FallbackClusterer clusters the embeddings)."""
    options = self.fallback_options
    codes = {
        fallback_clusterer.SingleClusterCondition.AffinityGmmBic: _lib.SC_SINGLE_GMM_BIC,
        fallback_clusterer.SingleClusterCondition.AllAffinity: _lib.SC_SINGLE_ALL_AFFINITY,
        fallback_clusterer.SingleClusterCondition.NeighborAffinity:
            _lib.SC_SINGLE_NEIGHBOR_AFFINITY,
        fallback_clusterer.SingleClusterCondition.AffinityStd: _lib.SC_SINGLE_AFFINITY_STD,
    }
    code = codes.get(options.single_cluster_condition)
    if code is None:
      return None
    return _lib.ScSingleCheck(code, int(options.single_cluster_affinity_diagonal_offset),
                              float(options.single_cluster_affinity_threshold))

  # predict_batch(..., batch_any_metric=True) while its library call runs
  _batch_any_metric = False

  def _batch_kmeans_ok(self) -> bool:
    """Is this clusterer's k-means one the grouped batch runs?  (`_batch.kmeans_ok`)"""
    return _batch.kmeans_ok(self)

  def _metric_needs_permission(self) -> bool:
    """A device metric other than cosine, outside a call that already holds the permission."""
    if self._batch_any_metric:
      return False
    try:
      return _lib.kmeans_metric_code(self.custom_dist) != _lib.KMEANS_METRICS["cosine"]
    except (ValueError, _lib.UnsupportedOnDeviceError):
      return False  # (predict() raises what it raises today)

  @contextlib.contextmanager
  def _any_metric_permission(self):
    """The handle's `sc_set_batch_any_metric` permission for the body: set before, cleared
    after, also when the body raises."""
    handle = self._handle()
    handle.check(handle.lib.sc_set_batch_any_metric(handle.raw, 1))
    self._batch_any_metric = True
    try:
      yield
    finally:
      self._batch_any_metric = False
      handle.lib.sc_set_batch_any_metric(handle.raw, 0)

  def _permission_if(self, wanted: bool):
    return self._any_metric_permission() if wanted else contextlib.nullcontext()

  def _library_batch_covers(self, min_embeddings_met: bool = False,
                            single_check_covered: bool = False,
                            affinity_input: bool = False) -> bool:
    """Is this clusterer one whose predict() the library batch calls reproduce?  (What is not:
    AutoTune, size reduction, the fallback decisions, user-supplied functions -- those go
    through predict().)  `min_embeddings_met`: the caller knows every utterance to hold at
    least `fallback_options.spectral_min_embeddings` rows (the centroids of a stream pool).
    `single_check_covered`: the caller makes the `sc_predict_batch_single` call, which carries
    the single-cluster test of `min_clusters == 1` -- covered when the condition is one of the
    four that read the affinity.  `affinity_input`: the caller makes the
    `sc_predict_batch_affinities` call -- the `affinity_function` takes no part, and
    predict_affinity's checks have dealt with the options that read embeddings."""
    return _batch.library_covers(self, min_embeddings_met, single_check_covered, affinity_input)

  def _naive_fallback(self) -> bool:
    return (self.fallback_options.fallback_clusterer_type ==
            fallback_clusterer.FallbackClustererType.Naive)

  def _naive_thresholds(self) -> typing.Tuple[float, float]:
    """(threshold, adaptation_threshold) as `NaiveClusterer` holds them -- None adaptation is
    the threshold -- or its ValueError."""
    c = naive_clusterer.NaiveClusterer(
        threshold=self.fallback_options.naive_threshold,
        adaptation_threshold=self.fallback_options.naive_adaptation_threshold)
    return float(c.threshold), float(c.adaptation_threshold)

  def _fallback_condition_covers(self, min_embeddings_met: bool = False,
                                 naive: bool = False) -> bool:
    """Is this clusterer one whose predict() `sc_predict_batch_single_fallback` reproduces?
    `min_clusters == 1` decided by the FallbackClusterer condition with the agglomerative
    fallback, and otherwise what `_library_batch_covers` asks, with cosine k-means.
    `min_embeddings_met` as there.  `naive`: the Naive fallback type is covered as well (the
    caller then makes the `sc_predict_batch_single_naive` call)."""
    return _batch.fallback_condition_covers(self, min_embeddings_met, naive)

  def _batch_kind(self, n: int) -> int:
    """What predict() does with an utterance of n rows (`_lib.BATCH_KIND_*`): the fallback
    clusterer, size reduction first, or the spectral path as it is (reference :229-248)."""
    if n < self.fallback_options.spectral_min_embeddings:
      return _lib.BATCH_KIND_FALLBACK
    if self.max_spectral_size is not None and n > self.max_spectral_size:
      return _lib.BATCH_KIND_REDUCED
    return _lib.BATCH_KIND_SPECTRAL

  def _reduced_batch_covers(self, utterances: typing.Sequence, streams: typing.Optional[int],
                            group: typing.Optional[int], naive: bool = False) -> bool:
    """Is this batch ONE `sc_predict_batch_reduced` call?  A clusterer that
    `_library_batch_covers` but for `max_spectral_size` / `spectral_min_embeddings`, in the
    grouped form, cosine k-means, no constraints (the caller has looked), an agglomerative
    fallback for the utterances that need one, and centroids that are not fallback members
    themselves (predict() recurses on them).  `naive`: fallback utterances may meet the Naive
    type as well (the caller then makes the `sc_predict_batch_reduced_naive` call)."""
    # (nothing to reduce: False, the caller's own answer stands)
    return _batch.reduced_covers(self, utterances, _batch.Form.make(group, streams).grouped,
                                 naive)

  def _multi_stage_batch_covers(self) -> bool:
    """Is this clusterer one whose predict() `sc_predict_batch_multi_stage` reproduces?
    `min_clusters == 1` with `max_spectral_size` and / or `spectral_min_embeddings` above 1, no
    AutoTune, the default affinity and k-means functions, cosine k-means, and centroids that are
    not fallback members themselves.  (The caller has looked at the form of the batch.)"""
    return _batch.multi_stage_covers(self)

  def _multi_stage_struct(self) -> _lib.ScMultiStage:
    """The `sc_multi_stage` of this clusterer (`_multi_stage_batch_covers` holds); the
    ValueError of `NaiveClusterer` for a threshold pair it rejects."""
    options = self.fallback_options
    stage = _lib.ScMultiStage()
    stage.max_spectral_size = int(self.max_spectral_size or 0)
    stage.spectral_min_embeddings = int(options.spectral_min_embeddings)
    stage.fallback_type = options.fallback_clusterer_type.value
    stage.agglomerative_threshold = float(options.agglomerative_threshold)
    if self._naive_fallback():
      stage.naive_threshold, stage.naive_adaptation_threshold = self._naive_thresholds()
    stage.single_condition = options.single_cluster_condition.value
    stage.single_threshold = float(options.single_cluster_affinity_threshold)
    stage.diagonal_offset = int(options.single_cluster_affinity_diagonal_offset)
    return stage

  def _batch_report(self, handle: _lib.Handle, diags, count: int) -> None:
    """`last_batch_diags` / `last_batch_routes` after a library batch call."""
    self.last_batch_diags = list(diags)
    # The library always exports the report (_lib.load() fails without it).  Only a stand-in
    # handle lacks it -- tests/test_host_logic.py drives this method with one that has the two
    # batch calls and nothing else --, and then there is nothing to report.
    report = getattr(handle.lib, "sc_last_batch_routes", None)
    self.last_batch_routes = None
    if report is not None:
      routes = (ctypes.c_int32 * count)()
      handle.check(report(handle.raw, routes, count))
      self.last_batch_routes = [int(r) for r in routes]
