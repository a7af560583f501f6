"""ctypes binding of libspectralcluster_amd.so (include/spectralcluster_amd.h).

The HIP library IS the product path: there is no NumPy fallback.  If the shared
object is missing, or no MI355X is visible, every compute entry point raises.
"""

from __future__ import annotations

import ctypes
import os
import threading
import typing

import numpy as np

SC_MAX_OPS = 16
SC_MAX_BLUR_RADIUS = 32
SC_MAX_EIG = 128
SC_MAX_STAGES = 16

SC_OK = 0
SC_ERR_INVALID = -1
SC_ERR_OOM = -2
SC_ERR_HIP = -3
SC_ERR_NOT_CONVERGED = -4
SC_ERR_UNSUPPORTED = -5
SC_ERR_NON_FINITE = -6

STAGE_NAMES = ("affinity", "refine", "diffuse", "scaling", "eig", "kmeans",
               "total", "blur", "threshold_sym", "matvec", "affinity_gemm",
               "free_quantize", "free_product", "free_scan", "free_stats")

# sc_last_batch_routes: what ran for an utterance of the last batch call
BATCH_ROUTE_SINGLE, BATCH_ROUTE_GROUP_LANCZOS, BATCH_ROUTE_GROUP_JACOBI = range(3)
BATCH_ROUTE_FALLBACK = 3  # sc_predict_batch_reduced: the agglomerative fallback clustered it
# sc_predict_batch_reduced: what an utterance of the batch was
BATCH_KIND_SPECTRAL, BATCH_KIND_REDUCED, BATCH_KIND_FALLBACK = range(3)
DIFFUSE_PATH_NONE, DIFFUSE_PATH_EXPLICIT, DIFFUSE_PATH_FREE, DIFFUSE_PATH_FREE_THEN_EXPLICIT = range(4)

_LIB_NAME = "libspectralcluster_amd.so"
_LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")


class DeviceLibraryError(RuntimeError):
  """The HIP shared library (or a device) is not available."""


class UnsupportedOnDeviceError(NotImplementedError):
  """The requested configuration is outside the device hot path."""


class EigenSolverNotConverged(RuntimeError):
  """The block-Lanczos eigensolver did not reach its tolerance."""


SC_ABI_VERSION = 11


class ScConfig(ctypes.Structure):
  """Mirror of `sc_config`."""
  _fields_ = [
      ("n_ops", ctypes.c_int32),
      ("ops", ctypes.c_int32 * SC_MAX_OPS),
      ("blur_radius", ctypes.c_int32),
      ("blur_weights", ctypes.c_double * (2 * SC_MAX_BLUR_RADIUS + 1)),
      ("p_percentile", ctypes.c_double),
      ("soft_multiplier", ctypes.c_double),
      ("threshold_type", ctypes.c_int32),
      ("binarize", ctypes.c_int32),
      ("preserve_diagonal", ctypes.c_int32),
      ("symmetrize_type", ctypes.c_int32),
      ("laplacian_type", ctypes.c_int32),
      ("min_clusters", ctypes.c_int32),
      ("max_clusters", ctypes.c_int32),
      ("stop_eigenvalue", ctypes.c_double),
      ("eigengap_type", ctypes.c_int32),
      ("row_wise_renorm", ctypes.c_int32),
      ("max_iter", ctypes.c_int32),
      ("eig_value_tol", ctypes.c_double),
      ("eig_vector_tol", ctypes.c_double),
      ("eig_max_cycles", ctypes.c_int32),
      ("constraint_name", ctypes.c_int32),
      ("constraint_before_refinement", ctypes.c_int32),
      ("integration_type", ctypes.c_int32),
      ("constraint_alpha", ctypes.c_double),
      ("kmeans_metric", ctypes.c_int32),
      ("diffuse_mode", ctypes.c_int32),
      ("reserved", ctypes.c_int32 * 4),
  ]


class ScDiag(ctypes.Structure):
  """Mirror of `sc_diag`."""
  _fields_ = [
      ("n", ctypes.c_int32),
      ("n_clusters_raw", ctypes.c_int32),
      ("n_clusters", ctypes.c_int32),
      ("eig_path", ctypes.c_int32),
      ("max_delta", ctypes.c_double),
      ("n_eigenvalues", ctypes.c_int32),
      ("eig_descending", ctypes.c_int32),
      ("eigenvalues", ctypes.c_double * SC_MAX_EIG),
      ("eig_matvec_passes", ctypes.c_int32),
      ("eig_block", ctypes.c_int32),
      ("eig_basis", ctypes.c_int32),
      ("eig_cycles", ctypes.c_int32),
      ("eig_max_residual", ctypes.c_double),
      ("kmeans_iterations", ctypes.c_int32),
      ("symmetry_state", ctypes.c_int32),
      ("eig_host_chain", ctypes.c_int32),
      ("eig_fallback", ctypes.c_int32),
      ("stage_ms", ctypes.c_float * SC_MAX_STAGES),
      ("diffuse_path", ctypes.c_int32),
      ("free_candidates", ctypes.c_int32),
      ("free_overflow_rows", ctypes.c_int32),
      ("free_tiles_run", ctypes.c_int32),
  ]

  def eigenvalue_array(self) -> np.ndarray:
    return np.array(self.eigenvalues[:self.n_eigenvalues], dtype=np.float64)

  def stage_times_ms(self) -> dict:
    return {name: float(self.stage_ms[i]) for i, name in enumerate(STAGE_NAMES)}


# sc_array.dtype / .location
SC_DTYPE_F64, SC_DTYPE_F32, SC_DTYPE_F16, SC_DTYPE_BF16 = range(4)
# label arrays only (sc_cluster_centroids_arrays, sc_labels_egress)
SC_DTYPE_I64, SC_DTYPE_I32 = 4, 5
SC_MEM_HOST, SC_MEM_DEVICE = range(2)
# sc_pool_get: what
SC_POOL_CACHE, SC_POOL_CENTROIDS = range(2)


class ScArray(ctypes.Structure):
  """Mirror of `sc_array`: where a matrix of embeddings is and what it looks like."""
  _fields_ = [
      ("data", ctypes.c_void_p),
      ("dtype", ctypes.c_int32),
      ("location", ctypes.c_int32),
      ("rows", ctypes.c_int64),
      ("cols", ctypes.c_int64),
      ("row_stride", ctypes.c_int64),
      ("col_stride", ctypes.c_int64),
  ]


_c_double_p = ctypes.POINTER(ctypes.c_double)


# sc_stage_front: route, and the slots of sc_front_out.info
SC_FRONT_ROUTE_SINGLE, SC_FRONT_ROUTE_GROUPED, SC_FRONT_ROUTE_SWEEP = range(3)
SC_FRONT_ROUTE_SHORT_SWEEP = 3  # a level of n <= 128: (matrix, p) pairs, one front launch
SC_FRONT_ROUTE_SHORT_WAVE = 4   # a wave of the short route of a batch: up to 64 members of n <= 128
SC_FRONT_INFO_COUNT = 16
FRONT_INFO_NAMES = ("diffuse_path", "symmetric", "folded_rownorm", "free_op", "digits_fused",
                    "blur_kernel", "blur_rows", "free_candidates", "free_overflow_rows",
                    "free_forms_s", "crop_source", "cut_kernel", "written", "launches")
SC_FRONT_INFO_CUT_KERNEL = FRONT_INFO_NAMES.index("cut_kernel")  # 5: k_short_wave_front
SC_FRONT_INFO_LAUNCHES = FRONT_INFO_NAMES.index("launches")      # (the short wave route only)
FRONT_OUTPUTS = ("a0", "cropval", "cut", "a", "s", "rowmax", "rowsum", "c", "p", "t")


class ScFrontOut(ctypes.Structure):
  """Mirror of `sc_front_out`: where sc_stage_front writes one member's front (NULL: not
  wanted) and what it reports about the branches taken."""
  _fields_ = [(name, _c_double_p) for name in FRONT_OUTPUTS] + [
      ("info", ctypes.c_int32 * SC_FRONT_INFO_COUNT)]


# sc_single_check.condition (the values of fallback_clusterer.SingleClusterCondition that read
# the affinity)
SC_SINGLE_GMM_BIC, SC_SINGLE_ALL_AFFINITY, SC_SINGLE_NEIGHBOR_AFFINITY, SC_SINGLE_AFFINITY_STD = \
    range(1, 5)
# sc_multi_stage.single_condition takes those four and the FallbackClusterer condition, which
# reads the embeddings (0: no single-cluster test)
SC_SINGLE_BY_FALLBACK = 5
# sc_batch_single_check: the 8 values per matrix
SINGLE_CHECK_VALUES = ("min", "neighbor_min", "mean", "std", "bic1", "bic2", "lloyd_steps",
                       "em_steps")


class ScSingleCheck(ctypes.Structure):
  """Mirror of `sc_single_check`: the single-cluster test a min_clusters = 1 batch carries."""
  _fields_ = [
      ("condition", ctypes.c_int32),
      ("diagonal_offset", ctypes.c_int32),
      ("threshold", ctypes.c_double),
  ]


class ScMultiStage(ctypes.Structure):
  """Mirror of `sc_multi_stage`: the multi-stage regime of `sc_predict_batch_multi_stage` --
  size reduction, the short-clip fallback and the single-cluster test of min_clusters = 1
  (`single_condition`: 0 none, 1-4 `SC_SINGLE_*`, 5 the FallbackClusterer condition)."""
  _fields_ = [
      ("max_spectral_size", ctypes.c_int32),
      ("spectral_min_embeddings", ctypes.c_int32),
      ("fallback_type", ctypes.c_int32),
      ("agglomerative_threshold", ctypes.c_double),
      ("naive_threshold", ctypes.c_double),
      ("naive_adaptation_threshold", ctypes.c_double),
      ("single_condition", ctypes.c_int32),
      ("single_threshold", ctypes.c_double),
      ("diagonal_offset", ctypes.c_int32),
  ]


class ScConstraintDesc(ctypes.Structure):
  """Mirror of `sc_constraint_desc`: the constraint of one utterance of
  `sc_predict_batch_constraints` (kind 0 none / 2 band / 3 pairs; host pointers)."""
  _fields_ = [
      ("kind", ctypes.c_int32),
      ("count", ctypes.c_int32),
      ("band", ctypes.POINTER(ctypes.c_double)),
      ("rows", ctypes.POINTER(ctypes.c_int32)),
      ("cols", ctypes.POINTER(ctypes.c_int32)),
      ("vals", ctypes.POINTER(ctypes.c_double)),
  ]


# sc_autotune.proxy (the values of autotune.AutoTuneProxy)
SC_AUTOTUNE_PERCENTILE_OVER_NME, SC_AUTOTUNE_PERCENTILE_SQRT_OVER_NME = 1, 2


class ScAutoTune(ctypes.Structure):
  """Mirror of `sc_autotune`: the state of an `AutoTune` object."""
  _fields_ = [
      ("p_min", ctypes.c_double),
      ("p_max", ctypes.c_double),
      ("step", ctypes.c_double),
      ("levels", ctypes.c_int32),
      ("proxy", ctypes.c_int32),
  ]


# sc_autotune_evaluate: (ps, count, ratios_out, user) -> sc_status
AUTOTUNE_EVALUATE = ctypes.CFUNCTYPE(ctypes.c_int, _c_double_p, ctypes.c_int, _c_double_p,
                                     ctypes.c_void_p)

_c_int64_p = ctypes.POINTER(ctypes.c_int64)
_c_int_p = ctypes.POINTER(ctypes.c_int)
_handle_t = ctypes.c_void_p

# name -> (restype, argtypes); every symbol include/spectralcluster_amd.h declares
PROTOTYPES = {
    "sc_abi_version": (ctypes.c_int, []),
    "sc_struct_sizes": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int),
                                       ctypes.POINTER(ctypes.c_int)]),
    "sc_array_layout": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int),
                                       ctypes.POINTER(ctypes.c_int)]),
    "sc_device_count": (ctypes.c_int, []),
    "sc_device_info": (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_int,
                                      ctypes.c_char_p, ctypes.c_int, _c_int_p,
                                      _c_int64_p]),
    "sc_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_handle_t)]),
    "sc_destroy": (ctypes.c_int, [_handle_t]),
    "sc_reserve": (ctypes.c_int, [_handle_t, ctypes.c_int, ctypes.c_int]),
    "sc_last_error": (ctypes.c_char_p, [_handle_t]),
    "sc_synchronize": (ctypes.c_int, [_handle_t]),
    "sc_set_profiling": (ctypes.c_int, [_handle_t, ctypes.c_int]),
    "sc_set_diffuse_mode": (ctypes.c_int, [_handle_t, ctypes.c_int]),
    "sc_set_free_prune": (ctypes.c_int, [_handle_t, ctypes.c_int]),
    "sc_stage_diffuse_rowstats": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int,
                                                 ctypes.c_int, _c_double_p, _c_double_p,
                                                 ctypes.POINTER(ctypes.c_int32)]),
    "sc_stage_block_operator": (ctypes.c_int, [_handle_t, ctypes.c_int,
                                               ctypes.POINTER(ctypes.c_int32),
                                               ctypes.POINTER(_c_double_p),
                                               ctypes.POINTER(_c_double_p),
                                               ctypes.POINTER(_c_double_p),
                                               ctypes.POINTER(_c_double_p),
                                               ctypes.POINTER(_c_double_p),
                                               ctypes.POINTER(_c_double_p), ctypes.c_int]),
    "sc_stage_krylov_state": (ctypes.c_int, [_handle_t, ctypes.POINTER(ctypes.c_int32),
                                             _c_double_p, _c_double_p, _c_double_p, _c_double_p,
                                             _c_double_p]),
    "sc_stage_front": (ctypes.c_int, [_handle_t, ctypes.c_int, ctypes.POINTER(ScConfig),
                                      ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int,
                                      ctypes.POINTER(_c_double_p), _c_double_p, _c_double_p,
                                      ctypes.POINTER(ScFrontOut)]),
    "sc_stage_tridiag": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int, _c_double_p,
                                        _c_double_p, _c_double_p, _c_double_p, _c_double_p,
                                        _c_double_p]),
    "sc_stage_tridiag_values": (ctypes.c_int, [_handle_t, _c_double_p, _c_double_p, ctypes.c_int,
                                               _c_double_p]),
    "sc_stage_td_backtransform": (ctypes.c_int, [_handle_t, _c_double_p, _c_double_p,
                                                 ctypes.c_int, _c_double_p, ctypes.c_int,
                                                 ctypes.c_int]),
    "sc_stage_hessenberg": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int, _c_double_p,
                                           _c_double_p, _c_double_p]),
    "sc_stage_general_ritz": (ctypes.c_int, [_handle_t, _c_double_p, _c_double_p, ctypes.c_int,
                                             ctypes.c_int, _c_double_p, _c_double_p, _c_double_p,
                                             _c_double_p, ctypes.c_int, _c_double_p, _c_double_p,
                                             _c_double_p, _c_double_p, _c_double_p, _c_double_p,
                                             ctypes.POINTER(ctypes.c_int32), ctypes.c_uint64,
                                             _c_double_p]),
    "sc_stage_arnoldi_state": (ctypes.c_int, [_handle_t, ctypes.POINTER(ctypes.c_int32),
                                              _c_double_p, _c_double_p, _c_double_p, _c_double_p,
                                              _c_double_p, _c_double_p]),
    "sc_config_default": (ctypes.c_int, [ctypes.POINTER(ScConfig)]),
    "sc_gaussian_weights": (ctypes.c_int, [ctypes.c_double,
                                           ctypes.POINTER(ctypes.c_int32),
                                           _c_double_p]),
    "sc_predict": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int, ctypes.c_int,
                                  ctypes.POINTER(ScConfig), _c_int64_p,
                                  ctypes.POINTER(ScDiag)]),
    "sc_set_embeddings": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int,
                                         ctypes.c_int]),
    "sc_predict_array": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray),
                                        ctypes.POINTER(ScConfig), _c_int64_p,
                                        ctypes.POINTER(ScDiag)]),
    "sc_set_embeddings_array": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray)]),
    "sc_predict_batch_arrays": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray), ctypes.c_int,
                                               ctypes.POINTER(ScConfig),
                                               ctypes.POINTER(_c_int64_p),
                                               ctypes.POINTER(ScDiag), ctypes.c_int,
                                               ctypes.c_int]),
    "sc_predict_batch_constrained": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray),
                                                    ctypes.POINTER(_c_double_p), ctypes.c_int,
                                                    ctypes.POINTER(ScConfig),
                                                    ctypes.POINTER(_c_int64_p),
                                                    ctypes.POINTER(ScDiag), ctypes.c_int]),
    "sc_constraint_desc_layout": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int),
                                                 ctypes.POINTER(ctypes.c_int)]),
    "sc_predict_batch_constraints": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray),
                                                    ctypes.POINTER(ScConstraintDesc), ctypes.c_int,
                                                    ctypes.POINTER(ScConfig),
                                                    ctypes.POINTER(_c_int64_p),
                                                    ctypes.POINTER(ScDiag), ctypes.c_int]),
    "sc_predict_batch_affinities": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray),
                                                   ctypes.POINTER(ScConstraintDesc), ctypes.c_int,
                                                   ctypes.POINTER(ScConfig),
                                                   ctypes.POINTER(_c_int64_p),
                                                   ctypes.POINTER(ScDiag), ctypes.c_int]),
    "sc_predict_batch_constraint_arrays": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray),
                                                          ctypes.POINTER(ScConstraintDesc),
                                                          ctypes.POINTER(ScArray), ctypes.c_int,
                                                          ctypes.POINTER(ScConfig),
                                                          ctypes.POINTER(_c_int64_p),
                                                          ctypes.POINTER(ScDiag), ctypes.c_int,
                                                          ctypes.c_int]),
    "sc_set_constraint_array": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray)]),
    "sc_stage_constraint_array": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScConfig),
                                                 _c_double_p, ctypes.POINTER(ScArray),
                                                 ctypes.c_int, _c_double_p]),
    "sc_stage_constraint_dense_group": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScConfig),
                                                       ctypes.c_int,
                                                       ctypes.POINTER(ctypes.c_int32),
                                                       ctypes.POINTER(_c_double_p),
                                                       ctypes.POINTER(_c_double_p),
                                                       ctypes.POINTER(_c_double_p)]),
    "sc_stage_gemm_pair_group": (ctypes.c_int, [_handle_t, ctypes.c_int,
                                                ctypes.POINTER(ctypes.c_int32),
                                                ctypes.POINTER(_c_double_p),
                                                ctypes.POINTER(_c_double_p),
                                                ctypes.POINTER(_c_double_p),
                                                ctypes.POINTER(_c_double_p), ctypes.c_int,
                                                ctypes.c_int]),
    "sc_stage_ingest": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray), _c_double_p]),
    "sc_set_affinity_array": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray)]),
    "sc_predict_affinity_array": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray),
                                                 ctypes.POINTER(ScConfig), _c_int64_p,
                                                 ctypes.POINTER(ScDiag)]),
    "sc_stage_affinity_ingest": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray), _c_double_p,
                                                _c_int_p]),
    "sc_stage_affinity_ingest_group": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray),
                                                      ctypes.c_int, ctypes.POINTER(_c_double_p),
                                                      _c_int_p]),
    "sc_compute_affinity": (ctypes.c_int, [_handle_t]),
    "sc_set_affinity": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int]),
    "sc_eig_ncluster": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScConfig),
                                       ctypes.POINTER(ScDiag)]),
    "sc_num_eigenvalues": (ctypes.c_int, [_handle_t]),
    "sc_get_eigenvalues": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int]),
    "sc_num_eigenvectors": (ctypes.c_int, [_handle_t]),
    "sc_get_eigenvectors": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int,
                                           ctypes.c_int]),
    "sc_cluster": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScConfig), ctypes.c_int,
                                  _c_int64_p, ctypes.POINTER(ScDiag)]),
    "sc_set_constraint": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int]),
    "sc_set_constraint_band": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int]),
    "sc_clear_constraint": (ctypes.c_int, [_handle_t]),
    "sc_constraint_info": (ctypes.c_int, [_handle_t, _c_int_p, _c_int_p,
                                          ctypes.POINTER(ctypes.c_size_t),
                                          ctypes.POINTER(ctypes.c_size_t)]),
    "sc_apply_constraint": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScConfig)]),
    "sc_stage_constraint": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScConfig), _c_double_p,
                                           _c_double_p, ctypes.c_int, _c_double_p]),
    "sc_stage_constraint_band": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScConfig),
                                                _c_double_p, _c_double_p, ctypes.c_int,
                                                _c_double_p]),
    "sc_stage_constraint_band_group": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScConfig),
                                                      ctypes.c_int,
                                                      ctypes.POINTER(ctypes.c_int32),
                                                      ctypes.POINTER(_c_double_p),
                                                      ctypes.POINTER(_c_double_p),
                                                      ctypes.POINTER(_c_double_p)]),
    "sc_set_constraint_pairs": (ctypes.c_int, [_handle_t, ctypes.POINTER(ctypes.c_int32),
                                               ctypes.POINTER(ctypes.c_int32), _c_double_p,
                                               ctypes.c_int, ctypes.c_int]),
    "sc_constraint_pairs_info": (ctypes.c_int, [_handle_t, _c_int_p,
                                                ctypes.POINTER(ctypes.c_size_t)]),
    "sc_stage_constraint_pairs": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScConfig),
                                                 _c_double_p, ctypes.POINTER(ctypes.c_int32),
                                                 ctypes.POINTER(ctypes.c_int32), _c_double_p,
                                                 ctypes.c_int, ctypes.c_int, _c_double_p]),
    "sc_stage_constraint_pairs_group": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScConfig),
                                                       ctypes.c_int,
                                                       ctypes.POINTER(ctypes.c_int32),
                                                       ctypes.POINTER(_c_double_p),
                                                       ctypes.POINTER(
                                                           ctypes.POINTER(ctypes.c_int32)),
                                                       ctypes.POINTER(
                                                           ctypes.POINTER(ctypes.c_int32)),
                                                       ctypes.POINTER(_c_double_p),
                                                       ctypes.POINTER(ctypes.c_int32),
                                                       ctypes.POINTER(_c_double_p)]),
    "sc_ahc": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                              ctypes.c_int, ctypes.c_double, _c_int64_p,
                              ctypes.POINTER(ctypes.c_int)]),
    "sc_cluster_centroids": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int, ctypes.c_int,
                                            _c_int64_p, ctypes.c_int, _c_double_p]),
    "sc_batch_ahc": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray), ctypes.c_int,
                                    ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                    ctypes.POINTER(_c_int64_p), ctypes.POINTER(_c_double_p)]),
    "sc_set_reduce_wave_bytes": (ctypes.c_int, [_handle_t, ctypes.c_size_t]),
    "sc_predict_batch_reduced": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray), ctypes.c_int,
                                                ctypes.POINTER(ScConfig), ctypes.c_int,
                                                ctypes.c_int, ctypes.c_double,
                                                ctypes.POINTER(_c_int64_p),
                                                ctypes.POINTER(ScDiag), ctypes.c_int,
                                                ctypes.POINTER(ctypes.c_int32)]),
    "sc_single_check_layout": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int),
                                              ctypes.POINTER(ctypes.c_int)]),
    "sc_predict_batch_single": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray), ctypes.c_int,
                                               ctypes.POINTER(ScConfig),
                                               ctypes.POINTER(ScSingleCheck),
                                               ctypes.POINTER(_c_int64_p),
                                               ctypes.POINTER(ScDiag), ctypes.c_int,
                                               ctypes.POINTER(ctypes.c_int32)]),
    "sc_batch_single_check": (ctypes.c_int, [_handle_t, ctypes.POINTER(_c_double_p), _c_int_p,
                                             ctypes.c_int, ctypes.POINTER(ScSingleCheck),
                                             _c_double_p, ctypes.POINTER(ctypes.c_int32)]),
    "sc_batch_fallback_check": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray), ctypes.c_int,
                                               ctypes.c_double, _c_double_p,
                                               ctypes.POINTER(ctypes.c_int32)]),
    "sc_predict_batch_single_fallback": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray),
                                                        ctypes.c_int, ctypes.POINTER(ScConfig),
                                                        ctypes.c_double,
                                                        ctypes.POINTER(_c_int64_p),
                                                        ctypes.POINTER(ScDiag), ctypes.c_int,
                                                        ctypes.POINTER(ctypes.c_int32)]),
    "sc_batch_naive_cluster": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray), ctypes.c_int,
                                              ctypes.c_double, ctypes.c_double,
                                              ctypes.POINTER(_c_int64_p),
                                              ctypes.POINTER(ctypes.c_int32),
                                              ctypes.POINTER(_c_double_p),
                                              ctypes.POINTER(ctypes.POINTER(ctypes.c_int32))]),
    "sc_batch_naive_check": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray), ctypes.c_int,
                                            ctypes.c_double, ctypes.c_double,
                                            ctypes.POINTER(ctypes.c_int32),
                                            ctypes.POINTER(ctypes.c_int32)]),
    "sc_predict_batch_reduced_naive": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray),
                                                      ctypes.c_int, ctypes.POINTER(ScConfig),
                                                      ctypes.c_int, ctypes.c_int,
                                                      ctypes.c_double, ctypes.c_double,
                                                      ctypes.POINTER(_c_int64_p),
                                                      ctypes.POINTER(ScDiag), ctypes.c_int,
                                                      ctypes.POINTER(ctypes.c_int32)]),
    "sc_predict_batch_single_naive": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray),
                                                     ctypes.c_int, ctypes.POINTER(ScConfig),
                                                     ctypes.c_double, ctypes.c_double,
                                                     ctypes.POINTER(_c_int64_p),
                                                     ctypes.POINTER(ScDiag), ctypes.c_int,
                                                     ctypes.POINTER(ctypes.c_int32)]),
    "sc_multi_stage_layout": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int),
                                             ctypes.POINTER(ctypes.c_int)]),
    "sc_predict_batch_multi_stage": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray),
                                                    ctypes.c_int, ctypes.POINTER(ScConfig),
                                                    ctypes.POINTER(ScMultiStage),
                                                    ctypes.POINTER(_c_int64_p),
                                                    ctypes.POINTER(ScDiag), ctypes.c_int,
                                                    ctypes.POINTER(ctypes.c_int32),
                                                    ctypes.POINTER(ctypes.c_int32)]),
    "sc_pool_create": (ctypes.c_int, [_handle_t, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, ctypes.POINTER(_handle_t)]),
    "sc_pool_destroy": (ctypes.c_int, [_handle_t]),
    "sc_pool_reset": (ctypes.c_int, [_handle_t, ctypes.c_int]),
    "sc_pool_rows": (ctypes.c_int, [_handle_t, ctypes.c_int]),
    "sc_pool_append": (ctypes.c_int, [_handle_t, ctypes.POINTER(ctypes.c_int32),
                                      ctypes.POINTER(ctypes.c_int32), ctypes.c_int,
                                      ctypes.POINTER(ScArray)]),
    "sc_pool_precluster": (ctypes.c_int, [_handle_t, ctypes.POINTER(ctypes.c_int32),
                                          ctypes.c_int, ctypes.POINTER(_c_int64_p)]),
    "sc_pool_centroids": (ctypes.c_int, [_handle_t, ctypes.c_int, ctypes.POINTER(ScArray)]),
    "sc_pool_fallback": (ctypes.c_int, [_handle_t, ctypes.POINTER(ctypes.c_int32), ctypes.c_int,
                                        ctypes.c_double, ctypes.POINTER(_c_int64_p)]),
    "sc_pool_cache": (ctypes.c_int, [_handle_t, ctypes.c_int, ctypes.POINTER(ScArray)]),
    "sc_pool_get": (ctypes.c_int, [_handle_t, ctypes.c_int, ctypes.c_int, _c_double_p]),
    "sc_pool_compress": (ctypes.c_int, [_handle_t, ctypes.c_int]),
    "sc_affinity_stats": (ctypes.c_int, [_handle_t, _c_double_p]),
    "sc_affinity_gmm_bic": (ctypes.c_int, [_handle_t, ctypes.c_int, _c_double_p, _c_double_p]),
    "sc_naive_cluster": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_double, ctypes.c_double, _c_double_p,
                                        ctypes.POINTER(ctypes.c_int32),
                                        ctypes.POINTER(ctypes.c_int32), ctypes.c_int,
                                        _c_int64_p]),
    "sc_run_resident": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScConfig),
                                       _c_int64_p, ctypes.POINTER(ScDiag)]),
    "sc_predict_batch": (ctypes.c_int, [_handle_t, ctypes.POINTER(_c_double_p),
                                        _c_int_p, ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(ScConfig),
                                        ctypes.POINTER(_c_int64_p),
                                        ctypes.POINTER(ScDiag)]),
    "sc_predict_batch_streams": (ctypes.c_int, [_handle_t, ctypes.POINTER(_c_double_p),
                                                _c_int_p, ctypes.c_int, ctypes.c_int,
                                                ctypes.POINTER(ScConfig),
                                                ctypes.POINTER(_c_int64_p),
                                                ctypes.POINTER(ScDiag), ctypes.c_int]),
    "sc_eig_ncluster_sweep": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScConfig), _c_double_p,
                                             ctypes.c_int, ctypes.POINTER(ScDiag)]),
    "sc_set_blur_weights": (ctypes.c_int, [_handle_t, ctypes.c_int, _c_double_p]),
    "sc_sweep_adopt": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScConfig), ctypes.c_int,
                                      ctypes.POINTER(ScDiag)]),
    "sc_predict_batch_grouped": (ctypes.c_int, [_handle_t, ctypes.POINTER(_c_double_p),
                                                _c_int_p, ctypes.c_int, ctypes.c_int,
                                                ctypes.POINTER(ScConfig),
                                                ctypes.POINTER(_c_int64_p),
                                                ctypes.POINTER(ScDiag), ctypes.c_int]),
    "sc_last_batch_routes": (ctypes.c_int, [_handle_t, ctypes.POINTER(ctypes.c_int32),
                                            ctypes.c_int]),
    "sc_stage_affinity": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int,
                                         ctypes.c_int, _c_double_p]),
    "sc_stage_refine": (ctypes.c_int, [_handle_t, ctypes.c_int,
                                       ctypes.POINTER(ScConfig), _c_double_p,
                                       ctypes.c_int, _c_double_p]),
    "sc_stage_laplacian": (ctypes.c_int, [_handle_t, ctypes.c_int, _c_double_p,
                                          ctypes.c_int, _c_double_p]),
    "sc_stage_sym_eig": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int, _c_double_p,
                                        _c_double_p, ctypes.POINTER(ScDiag)]),
    "sc_stage_eig": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int, _c_double_p,
                                        _c_double_p, ctypes.POINTER(ScDiag)]),
    "sc_stage_affinity_array": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray),
                                               ctypes.POINTER(ScArray)]),
    "sc_stage_refine_array": (ctypes.c_int, [_handle_t, ctypes.c_int, ctypes.POINTER(ScConfig),
                                             ctypes.POINTER(ScArray), ctypes.POINTER(ScArray)]),
    "sc_stage_laplacian_array": (ctypes.c_int, [_handle_t, ctypes.c_int, ctypes.POINTER(ScArray),
                                                ctypes.POINTER(ScArray)]),
    "sc_stage_eig_array": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray), ctypes.c_int,
                                          ctypes.c_int, ctypes.POINTER(ScArray),
                                          ctypes.POINTER(ScArray), ctypes.POINTER(ctypes.c_int)]),
    "sc_stage_egress": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.POINTER(ScArray)]),
    "sc_cluster_centroids_arrays": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray),
                                                   ctypes.POINTER(ScArray), ctypes.c_int,
                                                   ctypes.POINTER(ScArray),
                                                   ctypes.POINTER(ctypes.c_int32)]),
    "sc_labels_egress": (ctypes.c_int, [_handle_t, ctypes.POINTER(_c_int64_p), ctypes.c_int,
                                        ctypes.POINTER(ScArray)]),
    "sc_random_state_doubles": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_int,
                                               _c_double_p]),
    "sc_uniform_choice": (ctypes.c_int, [ctypes.c_int, ctypes.c_double]),
    "sc_host_symmetric_eig": (ctypes.c_int, [_c_double_p, ctypes.c_int, _c_double_p,
                                             _c_double_p]),
    "sc_host_symmetric_eig_partial": (ctypes.c_int, [_c_double_p, ctypes.c_int, ctypes.c_int,
                                                     _c_double_p, _c_double_p]),
    "sc_host_tridiag_eigvectors": (ctypes.c_int, [_c_double_p, _c_double_p, ctypes.c_int,
                                                  _c_double_p, ctypes.c_int, _c_double_p]),
    "sc_host_general_eig": (ctypes.c_int, [_c_double_p, ctypes.c_int, ctypes.c_int, _c_double_p,
                                           _c_double_p, _c_double_p, _c_double_p]),
    "sc_host_general_eig_fast": (ctypes.c_int, [_c_double_p, ctypes.c_int, ctypes.c_int, _c_double_p,
                                           _c_double_p, _c_double_p, _c_double_p]),
    "sc_host_hessenberg_eig": (ctypes.c_int, [_c_double_p, _c_double_p, ctypes.c_int, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_int32), _c_double_p,
                                              _c_double_p, _c_double_p, _c_double_p, _c_double_p]),
    "sc_host_value_error_bound": (ctypes.c_int, [_c_double_p, _c_double_p, ctypes.c_int,
                                                 ctypes.c_int, _c_double_p]),
    "sc_host_autotune_ratio": (ctypes.c_int, [ctypes.POINTER(ScAutoTune), ctypes.c_double,
                                              ctypes.c_double, _c_double_p]),
    "sc_host_autotune_search": (ctypes.c_int, [ctypes.POINTER(ScAutoTune), AUTOTUNE_EVALUATE,
                                               ctypes.c_void_p, _c_double_p, _c_int_p,
                                               _c_double_p, ctypes.POINTER(ScAutoTune)]),
    "sc_predict_batch_autotune": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray),
                                                 ctypes.POINTER(_c_double_p), ctypes.c_int,
                                                 ctypes.POINTER(ScConfig),
                                                 ctypes.POINTER(ScAutoTune),
                                                 ctypes.POINTER(_c_int64_p),
                                                 ctypes.POINTER(ScDiag), _c_double_p, ctypes.c_int,
                                                 _c_double_p]),
    "sc_eigengap": (ctypes.c_int, [_c_double_p, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                   _c_int_p, _c_double_p]),
    "sc_stage_kmeans": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, _c_int64_p,
                                       _c_double_p, _c_int_p]),
    "sc_stage_kmeans_metric": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              _c_int64_p, _c_double_p, _c_int_p]),
    "sc_stage_kmeans_trace": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, _c_int_p, _c_double_p,
                                             _c_int_p, _c_int_p, _c_double_p, _c_double_p,
                                             _c_int64_p, _c_double_p, ctypes.c_int, _c_int_p,
                                             _c_double_p, _c_int64_p]),
    "sc_stage_kmeans_trace_group": (ctypes.c_int, [_handle_t, _c_double_p, _c_int_p, _c_int_p,
                                                   ctypes.c_int, ctypes.c_int, _c_double_p,
                                                   _c_int_p, _c_int_p, _c_double_p, _c_double_p,
                                                   _c_int64_p, _c_double_p, ctypes.c_int,
                                                   _c_int_p, _c_double_p, _c_int64_p]),
    "sc_stage_kmeans_trace_metric": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int,
                                                    ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                    ctypes.c_int, _c_int_p, _c_double_p, _c_int_p,
                                                    _c_int_p, _c_double_p, _c_double_p,
                                                    _c_int64_p, _c_double_p, ctypes.c_int,
                                                    _c_int_p, _c_double_p, _c_int64_p]),
    "sc_stage_kmeans_trace_group_metric": (ctypes.c_int, [_handle_t, _c_double_p, _c_int_p,
                                                          _c_int_p, ctypes.c_int, ctypes.c_int,
                                                          ctypes.c_int, _c_double_p, _c_int_p,
                                                          _c_int_p, _c_double_p, _c_double_p,
                                                          _c_int64_p, _c_double_p, ctypes.c_int,
                                                          _c_int_p, _c_double_p, _c_int64_p]),
    "sc_set_batch_any_metric": (ctypes.c_int, [_handle_t, ctypes.c_int]),
    "sc_stage_kmeans_general": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_double, _c_double_p,
                                               _c_int64_p, _c_double_p, _c_int_p]),
    "sc_stage_kmeans_general_array": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray),
                                                     ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                     ctypes.c_double, _c_double_p, _c_int64_p,
                                                     _c_double_p, _c_int_p]),
    "sc_stage_kmeans_metric_array": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray),
                                                    ctypes.c_int, ctypes.c_int, _c_int64_p,
                                                    _c_double_p, _c_int_p]),
    "sc_stage_ingest_columns": (ctypes.c_int, [_handle_t, ctypes.POINTER(ScArray), _c_double_p]),
    "sc_stage_linkage": (ctypes.c_int, [_handle_t, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        _c_int_p, _c_double_p, ctypes.c_int, ctypes.c_double,
                                        _c_int_p, _c_double_p, _c_double_p, _c_int64_p,
                                        ctypes.c_int, ctypes.c_double]),
    "sc_stage_cosine_distances": (ctypes.c_int, [_handle_t, ctypes.c_int, _c_double_p,
                                                 ctypes.c_int, ctypes.c_int, _c_double_p]),
    "sc_comm_available": (ctypes.c_int, []),
    "sc_comm_unique_id": (ctypes.c_int, [ctypes.c_char_p]),
    "sc_comm_init_rank": (ctypes.c_int, [_handle_t, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_char_p, ctypes.POINTER(_handle_t)]),
    "sc_comm_init_all": (ctypes.c_int, [ctypes.POINTER(_handle_t), ctypes.c_int,
                                        ctypes.POINTER(_handle_t)]),
    "sc_comm_destroy": (ctypes.c_int, [_handle_t]),
    "sc_comm_rank": (ctypes.c_int, [_handle_t]),
    "sc_comm_size": (ctypes.c_int, [_handle_t]),
    "sc_comm_last_error": (ctypes.c_char_p, [_handle_t]),
    "sc_comm_broadcast": (ctypes.c_int, [_handle_t, ctypes.c_void_p, ctypes.c_size_t,
                                         ctypes.c_int]),
    "sc_comm_allgather": (ctypes.c_int, [_handle_t, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_size_t]),
    "sc_comm_allreduce_max": (ctypes.c_int, [_handle_t, _c_double_p, ctypes.c_int]),
    "sc_comm_barrier": (ctypes.c_int, [_handle_t]),
}

# ... and the one that returns a pointer (the header test reads the `int` / `const char*` ones)
POINTER_PROTOTYPES = {
    "sc_stream": (ctypes.c_void_p, [_handle_t]),
}

# custom_dist values that run on the device (scipy cdist names)
KMEANS_METRICS = {"cosine": 0, "euclidean": 1, "sqeuclidean": 2, "cityblock": 3,
                  "chebyshev": 4, "correlation": 5, "braycurtis": 6, "canberra": 7,
                  # scipy's cdist without a `p` argument (the reference passes none,
                  # custom_distance_kmeans.py:123-124) takes p = 2: the Euclidean distance
                  "minkowski": 1}
# ... and the aliases scipy.spatial.distance accepts for them (scipy 1.15 _METRIC_INFOS;
# cdist lower-cases the name first)
_KMEANS_METRIC_ALIASES = {
    "cos": "cosine", "e": "euclidean", "eu": "euclidean", "euclid": "euclidean",
    "sqe": "sqeuclidean", "sqeuclid": "sqeuclidean", "c": "cityblock", "cb": "cityblock",
    "cblock": "cityblock", "ch": "chebyshev", "cheb": "chebyshev", "cheby": "chebyshev",
    "chebychev": "chebyshev", "co": "correlation", "m": "minkowski", "mi": "minkowski",
    "pnorm": "minkowski"}


class NotFittedError(ValueError, AttributeError):
  """Same bases as sklearn.exceptions.NotFittedError, which the reference raises for a
  falsy custom_dist."""


def kmeans_metric_code(custom_dist) -> int:
  """sc_config.kmeans_metric for a `custom_dist` argument (reference
  custom_distance_kmeans.py:13-52)."""
  if not custom_dist:
    # reference :33-36 builds an sklearn KMeans and :51 calls .predict() on it without
    # ever fitting it: custom_dist=None / "" always ends in sklearn's NotFittedError
    raise NotFittedError(
        "This KMeans instance is not fitted yet. Call 'fit' with appropriate arguments "
        "before using this estimator.")
  if isinstance(custom_dist, str):
    name = custom_dist.lower()
    name = _KMEANS_METRIC_ALIASES.get(name, name)
    if name in KMEANS_METRICS:
      return KMEANS_METRICS[name]
  raise UnsupportedOnDeviceError(
      "custom_dist=%r: the device path implements %s (and scipy's aliases of those); other "
      "scipy metrics and callables are not on it" % (custom_dist, ", ".join(sorted(KMEANS_METRICS))))


_lib = None
_lib_lock = threading.Lock()


def library_path() -> str:
  return os.environ.get("SPECTRALCLUSTER_AMD_LIB", os.path.join(_LIB_DIR, _LIB_NAME))


def load() -> ctypes.CDLL:
  """Load the shared library (once) and declare every prototype."""
  global _lib
  if _lib is not None:
    return _lib
  with _lib_lock:
    if _lib is not None:
      return _lib
    path = library_path()
    if not os.path.exists(path):
      raise DeviceLibraryError(
          "%s not found: build it with `make -C spectralcluster_amd/csrc` "
          "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is "
          "no CPU fallback for the hot path." % path)
    try:
      lib = ctypes.CDLL(path)
    except OSError as exc:  # missing libamdhip64 etc.
      raise DeviceLibraryError("cannot load %s: %s" % (path, exc)) from exc
    for name, (restype, argtypes) in list(PROTOTYPES.items()) + list(POINTER_PROTOTYPES.items()):
      fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
      fn.restype = restype
      fn.argtypes = argtypes
    if lib.sc_abi_version() != SC_ABI_VERSION:
      raise DeviceLibraryError("ABI version mismatch in %s (rebuild it)" % path)
    cfg_bytes, diag_bytes = ctypes.c_int(0), ctypes.c_int(0)
    lib.sc_struct_sizes(ctypes.byref(cfg_bytes), ctypes.byref(diag_bytes))
    if (cfg_bytes.value != ctypes.sizeof(ScConfig) or
        diag_bytes.value != ctypes.sizeof(ScDiag)):
      raise DeviceLibraryError("sc_config / sc_diag layout mismatch in %s" % path)
    arr_bytes, offsets = ctypes.c_int(0), (ctypes.c_int * len(ScArray._fields_))()
    lib.sc_array_layout(ctypes.byref(arr_bytes), offsets)
    if (arr_bytes.value != ctypes.sizeof(ScArray) or
        list(offsets) != [getattr(ScArray, name).offset for name, _ in ScArray._fields_]):
      raise DeviceLibraryError("sc_array layout mismatch in %s" % path)
    _lib = lib
    return lib


def device_count() -> int:
  return int(load().sc_device_count())


def as_double_p(a: np.ndarray):
  return a.ctypes.data_as(_c_double_p)


def sync_blur_weights(handle, cfg) -> None:
  """A GaussianBlur of sigma > 8 has more weights than `sc_config` holds (radius > 32):
  `refinement.fill_config` leaves them on the config object and they are uploaded to the
  handle here, before the config is used with it (sc_set_blur_weights)."""
  w = getattr(cfg, "_blur_ext", None)
  if w is not None:
    handle.check(handle.lib.sc_set_blur_weights(handle.raw, int(cfg.blur_radius),
                                                as_double_p(w)))


def as_int64_p(a: np.ndarray):
  return a.ctypes.data_as(_c_int64_p)


def as_int32_p(a: np.ndarray):
  return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


class Handle:
  """Owns one `sc_handle` (one device, one stream).  Not thread-safe."""

  def __init__(self, device: int = 0):
    self._lib = load()
    if self._lib.sc_device_count() <= 0:
      raise DeviceLibraryError(
          "no HIP device visible: the hot path runs on an MI355X only "
          "(there is no CPU fallback)")
    h = _handle_t()
    rc = self._lib.sc_create(int(device), ctypes.byref(h))
    if rc != SC_OK:
      raise DeviceLibraryError("sc_create(device=%d) failed with %d" % (device, rc))
    self._h = h
    self.device = int(device)

  def close(self):
    if getattr(self, "_h", None):
      self._lib.sc_destroy(self._h)
      self._h = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # interpreter shutdown
      pass

  @property
  def raw(self):
    return self._h

  @property
  def lib(self):
    return self._lib

  def stream(self) -> int:
    """The handle's hipStream_t as an integer (what `__dlpack__(stream=...)` takes)."""
    return int(self._lib.sc_stream(self._h) or 0)

  def last_error(self) -> str:
    msg = self._lib.sc_last_error(self._h)
    return msg.decode("utf-8", "replace") if msg else ""

  def check(self, rc: int, invalid_exc: typing.Type[Exception] = ValueError):
    """Translate an sc_status into the exception the reference would raise."""
    if rc == SC_OK:
      return
    msg = self.last_error() or "status %d" % rc
    if rc == SC_ERR_INVALID:
      raise invalid_exc(msg)
    if rc == SC_ERR_NON_FINITE:
      raise np.linalg.LinAlgError(msg)   # what np.linalg.eig raises (a ValueError)
    if rc == SC_ERR_UNSUPPORTED:
      raise UnsupportedOnDeviceError(msg)
    if rc == SC_ERR_NOT_CONVERGED:
      raise EigenSolverNotConverged(msg)
    if rc == SC_ERR_OOM:
      raise MemoryError(msg)
    raise DeviceLibraryError(msg)


_default_handles = {}
_scope = threading.local()


class use_device:
  """`with use_device(k):` -- module-level helpers called inside (which take no device
  argument, like the reference's functions) run on device k in this thread.  A
  `SpectralClusterer(device=k)` wraps its predict() in it, so its pre-clustering, fallback
  and single-cluster helpers share its GPU and arena."""

  def __init__(self, device: typing.Optional[int]):
    self.device = device

  def __enter__(self):
    self.previous = getattr(_scope, "device", None)
    if self.device is not None:
      _scope.device = self.device
    return self

  def __exit__(self, *exc):
    _scope.device = self.previous


def default_handle(device: typing.Optional[int] = None) -> Handle:
  """Process-wide handle per device (the enclosing `use_device`, else
  SPECTRALCLUSTER_AMD_DEVICE, else LOCAL_RANK, else 0)."""
  if device is None:
    device = getattr(_scope, "device", None)
  if device is None:
    device = int(os.environ.get("SPECTRALCLUSTER_AMD_DEVICE",
                                os.environ.get("LOCAL_RANK", "0")))
    count = device_count()
    if count > 0:
      device %= count
  if device not in _default_handles:
    _default_handles[device] = Handle(device)
  return _default_handles[device]


_handle_pools = {}


def handle_pool(device: typing.Optional[int], size: int) -> typing.List[Handle]:
  """`size` independent handles (streams) on one device, created once per process.
  Handle 0 of the pool is the device's default handle."""
  first = default_handle(device)
  pool = _handle_pools.setdefault(first.device, [first])
  while len(pool) < size:
    pool.append(Handle(first.device))
  return pool[:size]
