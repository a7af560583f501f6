"""CPU: an affinity the caller holds.  The reference helper the GPU tests compare against
(`_affinity_ref.predict_from_affinity`) is the oracle's predict() from its second line on; the
ValueErrors of `predict_affinity` / `predict_affinity_batch` are raised before any device is
touched; the new entry points are declared, prototyped and exported."""

import os
import re

import numpy as np
import pytest

import spectral_oracle as so
from conftest import golden
from _affinity_ref import eigengap_margin, predict_from_affinity

import spectralcluster_amd as sca
from spectralcluster_amd import _dlpack
from spectralcluster_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sc_set_affinity_array", "sc_predict_affinity_array", "sc_predict_batch_affinities",
               "sc_stage_affinity_ingest", "sc_stage_affinity_ingest_group")


@pytest.mark.parametrize("name", ["e2e_n200_lap4_max7.npz", "e2e_n200_lap0_max7.npz"])
def test_helper_fed_the_cosine_affinity_is_the_oracle_predict_and_the_golden(name):
  g = golden(name)
  n, d, k, seed, lap, max_clusters = [int(v) for v in g["params"]]
  x = so.blobs(n, d, k, seed)
  cfg = so.icassp2018_config(laplacian_type=lap, max_clusters=max_clusters,
                             p_percentile=float(g["p_percentile"]))
  want = so.predict(x, cfg)
  dump = {}
  got = predict_from_affinity(so.affinity(x), cfg, dump=dump)
  assert np.array_equal(got, want)
  assert so.adjusted_rand_index(got, g["labels"]) == 1.0
  assert dump["n_clusters"] == max(int(g["n_clusters_raw"]), cfg.min_clusters or 0)
  # the decision these labels hang on is no near tie
  assert eigengap_margin(dump["eigenvalues"], cfg, descend=lap in (0, 1)) > 0.05
  # a float32 affinity is widened, not rounded again
  a32 = so.affinity(x).astype(np.float32)
  assert np.array_equal(predict_from_affinity(a32, cfg),
                        predict_from_affinity(a32.astype(np.float64), cfg))


def test_helper_runs_the_autotune_search_and_the_constraint_like_the_oracle():
  x, _, scores = so.turn_blobs(120, 16, 3, seed=5, noise=1.0)
  cfg = so.turntodiarize_config()
  q = so.constraint_matrix_diagonals(scores, 1)
  want = so.predict(x, cfg, constraint_matrix=q, autotune=so.TURNTODIARIZE_AUTOTUNE)
  got = predict_from_affinity(so.affinity(x), cfg, q, so.TURNTODIARIZE_AUTOTUNE)
  assert np.array_equal(got, want)


def test_not_2d_and_not_square_raise_without_a_device():
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=5)
  with pytest.raises(ValueError, match="2-dimensional"):
    c.predict_affinity(np.zeros(9))
  with pytest.raises(ValueError, match="2-dimensional"):
    c.predict_affinity(np.zeros((3, 3, 3)))
  with pytest.raises(ValueError, match="square"):
    c.predict_affinity(np.zeros((4, 5)))
  with pytest.raises(ValueError, match="affinity 1 must be a square"):
    c.predict_affinity_batch([np.eye(4), np.zeros((4, 5), dtype=np.float32)])
  with pytest.raises(TypeError):
    c.predict_affinity([[1.0, 0.0], [0.0, 1.0]])


def test_the_options_that_read_embeddings_raise_and_name_the_option():
  a = np.eye(30)
  few = sca.SpectralClusterer(fallback_options=sca.FallbackOptions(spectral_min_embeddings=40))
  with pytest.raises(ValueError, match="spectral_min_embeddings"):
    few.predict_affinity(a)
  reduced = sca.SpectralClusterer(min_clusters=2, max_clusters=5, max_spectral_size=20)
  with pytest.raises(ValueError, match="max_spectral_size"):
    reduced.predict_affinity(a)
  single = sca.SpectralClusterer(
      min_clusters=1, max_clusters=5,
      fallback_options=sca.FallbackOptions(
          single_cluster_condition=sca.SingleClusterCondition.FallbackClusterer))
  with pytest.raises(ValueError, match="FallbackClusterer"):
    single.predict_affinity(a)
  for c in (few, reduced, single):  # ... for every matrix of a batch, before anything runs
    with pytest.raises(ValueError):
      c.predict_affinity_batch([a, a])


def test_batch_checks_the_constraint_list_before_anything_runs():
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=5)
  with pytest.raises(ValueError, match="as long as the batch"):
    c.predict_affinity_batch([np.eye(4)], constraint_matrices=[None, None])
  constrained = sca.SpectralClusterer(
      min_clusters=2, max_clusters=5,
      constraint_options=sca.ConstraintOptions(
          constraint_name=sca.ConstraintName.AffinityIntegration,
          apply_before_refinement=True, integration_type=sca.IntegrationType.Max))
  with pytest.raises(ValueError):  # predict()'s error for a ConstraintMatrix of another size
    constrained.predict_affinity_batch([np.eye(6), np.eye(6)],
                                       [None, sca.ConstraintMatrix([0.0] * 5, 1)])
  with pytest.raises(ValueError):
    constrained.predict_affinity_batch([np.eye(6)], [sca.PairwiseConstraints(7)])


def test_a_numpy_view_is_described_with_its_strides_on_the_affinity_path_only():
  big = np.arange(64, dtype=np.float32).reshape(8, 8)
  for view in (big.T, big[::2, ::2], big[1:5, 1:5]):
    src = _dlpack.describe(view, None, strided=True)
    a = src.array
    assert (a.rows, a.cols) == view.shape and a.dtype == _lib.SC_DTYPE_F32
    assert (a.row_stride, a.col_stride) == tuple(s // 4 for s in view.strides)
    assert a.data == view.ctypes.data
    packed = _dlpack.describe(view, None)  # the embeddings paths: made contiguous
    assert (packed.array.row_stride, packed.array.col_stride) == (view.shape[1], 1)
  flipped = _dlpack.describe(big[::-1], None, strided=True)  # negative stride: a host copy
  assert (flipped.array.row_stride, flipped.array.col_stride) == (8, 1)
  ints = _dlpack.describe(np.eye(3, dtype=np.int32), None, strided=True)  # promoted
  assert ints.array.dtype == _lib.SC_DTYPE_F64


def test_new_symbols_are_declared_prototyped_exported_and_listed():
  header = open(os.path.join(ROOT, "include", "spectralcluster_amd.h")).read()
  declared = set(re.findall(r"^(?:int|const char\*)\s+(sc_[a-z0-9_]+)\s*\(", header, flags=re.M))
  integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
  lib = _lib.load()
  for name in NEW_SYMBOLS:
    assert name in declared, name
    assert name in _lib.PROTOTYPES, name
    assert hasattr(lib, name), name
    assert "`%s`" % name in integration, name
  assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)
  assert lib.sc_abi_version() == _lib.SC_ABI_VERSION == 11  # functions were only added


def test_entry_points_reject_a_null_handle():
  lib = _lib.load()
  assert lib.sc_set_affinity_array(None, None) == _lib.SC_ERR_INVALID
  assert lib.sc_predict_affinity_array(None, None, None, None, None) == _lib.SC_ERR_INVALID
  assert lib.sc_predict_batch_affinities(None, None, None, 0, None, None, None,
                                         16) == _lib.SC_ERR_INVALID
  assert lib.sc_stage_affinity_ingest(None, None, None, None) == _lib.SC_ERR_INVALID
  assert lib.sc_stage_affinity_ingest_group(None, None, 1, None, None) == _lib.SC_ERR_INVALID
