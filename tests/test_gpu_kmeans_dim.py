"""k-means on embeddings of any width (`run_kmeans` with dim != n_clusters, `CustomKMeans`) on
the device: the general form of kmeans_general.hip behind sc_stage_kmeans_general.

Checks: the reference's own 1000 x 6 known answers, the real reference's goldens
(tests/golden/kmeans_dim.npz, tools/make_kmeans_dim_golden.py) label for label, the new entry
against the dim == k goldens of the predict() form, large inputs against the oracle computed
live, determinism and the errors.

Small-problem threshold: the row passes run one workgroup per KG_ROWS = 64 rows, so an input of
at most 64 rows runs them on a single workgroup and every larger one on several (the general
form has no separate single-workgroup kernel); test_both_sides_of_the_one_workgroup_threshold
covers 64 and 65 rows.
"""

import ctypes

import numpy as np
import pytest
from scipy.spatial.distance import cdist

import spectral_oracle as so
from conftest import golden

import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import custom_distance_kmeans as ckm

pytestmark = pytest.mark.gpu

K = {"a": 4, "b": 5, "c": 6, "d": 8}
METRICS = ("cosine", "euclidean", "sqeuclidean", "cityblock", "chebyshev", "correlation",
           "braycurtis", "canberra", "minkowski")


def general(e, k, metric, max_iter=300, tol=0.001, init=None):
  """sc_stage_kmeans_general through ctypes: (labels, centroids, passes)."""
  e = np.ascontiguousarray(e, dtype=np.float64)
  n, dim = e.shape
  labels = np.empty(n, dtype=np.int64)
  cent = np.empty((k, dim), dtype=np.float64)
  iters = ctypes.c_int(0)
  code = _lib.kmeans_metric_code(metric)
  if init is not None:
    init = np.ascontiguousarray(init, dtype=np.float64)
  h = _lib.default_handle()
  h.check(h.lib.sc_stage_kmeans_general(
      h.raw, _lib.as_double_p(e), n, dim, k, max_iter, code, tol,
      None if init is None else _lib.as_double_p(init), _lib.as_int64_p(labels),
      _lib.as_double_p(cent), ctypes.byref(iters)))
  return labels, cent, iters.value


# --- 1. the reference's known answers (tests/custom_distance_kmeans_test.py:46-72) ----------
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_reference_1000by6_known_answer(metric, seed):
  matrix = np.array([[1.0, 0.0, 0.0, 0.0, 0.0, 0.0]] * 400 +
                    [[0.0, 1.0, 0.0, 0.0, 0.0, 0.0]] * 300 +
                    [[0.0, 0.0, 2.0, 0.0, 0.0, 0.0]] * 200 +
                    [[0.0, 0.0, 0.0, 1.0, 0.0, 0.0]] * 100)
  noisy = np.random.RandomState(seed).rand(1000, 6) * 2 - 1
  matrix = matrix + noisy * 0.1
  labels = ckm.run_kmeans(matrix, n_clusters=4, max_iter=300, custom_dist=metric)
  expected = np.array([0] * 400 + [1] * 300 + [2] * 200 + [3] * 100)
  assert np.array_equal(so.ordered_labels(labels), expected)


# --- 2. run_kmeans goldens of the real reference -------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_run_kmeans_vs_reference_golden(tag):
  g = golden("kmeans_dim.npz")
  e = g["e_" + tag].astype(np.float64)
  assert e.shape[1] != K[tag]
  for metric in METRICS:
    key = "labels_%s_%s" % (tag, metric)
    if key not in g:
      continue
    got = ckm.run_kmeans(e, K[tag], metric, 300)
    assert got.dtype == np.int64
    assert np.array_equal(got, g[key]), metric


# --- 3. CustomKMeans goldens: labels, centroids, the caller's array updated in place ----------
@pytest.mark.parametrize("tag", ["a", "b"])
def test_custom_kmeans_vs_reference_golden(tag):
  g = golden("kmeans_dim.npz")
  e = g["e_" + tag]
  runs = [(m, 0.001, "ck_%s_%s" % (tag, m)) for m in METRICS]
  runs.append(("cosine", 0.2, "ck_%s_cosine_tol02" % tag))
  for metric, tol, key in runs:
    cent = g["init_" + tag].copy()
    km = ckm.CustomKMeans(n_clusters=K[tag], centroids=cent, tol=tol, custom_dist=metric)
    got = km.predict(e)
    assert km.centroids is cent
    assert np.array_equal(got, g[key + "_labels"]), key
    np.testing.assert_allclose(cent, g[key + "_cent"], rtol=1e-12, atol=1e-13, err_msg=key)


# --- 4. centroids=None: random rows, then the reference's UnboundLocalError or its labels -----
def test_custom_kmeans_without_centroids_moves_the_rng_like_the_reference():
  g = golden("kmeans_dim.npz")
  for i in range(4):
    tag, k, metric, seed = str(g["none_%d_case" % i]).split(",")
    e = g["e_" + tag]
    np.random.seed(int(seed))
    km = ckm.CustomKMeans(n_clusters=int(k), custom_dist=metric)
    exc = str(g["none_%d_exc" % i])
    if exc:
      with pytest.raises(UnboundLocalError):
        km.predict(e)
      assert exc == "UnboundLocalError"
    else:
      assert np.array_equal(km.predict(e), g["none_%d_labels" % i])
    assert km.centroids.shape == (int(k), e.shape[1])
    assert np.random.rand() == float(g["none_%d_next_rand" % i])


# --- 5. the new entry with dim == k against the predict() form's goldens ----------------------
@pytest.mark.parametrize("tag,k", [("a", 4), ("b", 8), ("c", 2), ("d", 20)])
def test_general_entry_on_square_kmeans_golden(tag, k):
  g = golden("kmeans.npz")
  labels, _, _ = general(g["e_" + tag], k, "cosine")
  assert np.array_equal(labels, g["labels_" + tag])


@pytest.mark.parametrize("metric", ["euclidean", "sqeuclidean", "cityblock", "chebyshev",
                                    "correlation", "braycurtis", "canberra", "minkowski"])
def test_general_entry_on_square_metric_goldens(metric):
  g = golden("kmeans_metrics.npz")
  for tag, k in (("a", 4), ("b", 7), ("c", 2)):
    if metric == "correlation" and k == 2:
      # a row-centred 2-vector is (d, -d): every correlation distance is 0 or 2 up to rounding
      # (the same exclusion as test_gpu_stages.py's golden test of the metric)
      continue
    labels, _, _ = general(g["e_" + tag], k, metric)
    assert np.array_equal(labels, g["labels_%s_%s" % (tag, metric)]), (tag, metric)


# --- 6. large inputs against the oracle, computed live -------------------------------------
@pytest.mark.parametrize("n,dim,k,metric,seed", [
    (8192, 256, 20, "cosine", 40), (8192, 256, 20, "euclidean", 41),
    (20000, 64, 10, "euclidean", 42),
    (3000, 160, 150, "cosine", 43),   # k * dim * 8 B = 192 KB: more than a CU's LDS
])
def test_large_vs_oracle(n, dim, k, metric, seed):
  e = so.blobs(n, dim, k, seed=seed, noise=0.5)
  got = ckm.run_kmeans(e, k, metric, 300)
  assert np.array_equal(got, so.run_kmeans_metric(e, k, 300, metric))


@pytest.mark.parametrize("n", [64, 65])
@pytest.mark.parametrize("metric", ["cosine", "correlation", "cityblock"])
def test_both_sides_of_the_one_workgroup_threshold(n, metric):
  e = so.blobs(n, 9, 3, seed=n, noise=0.2)
  got = ckm.run_kmeans(e, 3, metric, 300)
  assert np.array_equal(got, so.run_kmeans_metric(e, 3, 300, metric))


def test_custom_kmeans_wide_centroids_vs_oracle_loop():
  """Given centroids, k * dim beyond LDS, every metric's loop against scipy's cdist."""
  rng = np.random.default_rng(44)
  e = so.blobs(2000, 300, 40, seed=44, noise=0.4)
  init = e[rng.choice(2000, 40, replace=False)] + 0.01
  for metric in ("cosine", "euclidean", "cityblock", "correlation"):
    cent = init.copy()
    got = ckm.CustomKMeans(40, centroids=cent, max_iter=20, custom_dist=metric).predict(e)
    ref = init.copy()
    prev, n = 0, e.shape[0]
    for it in range(21):
      d = cdist(e, ref, metric=metric)
      lab = d.argmin(axis=1)
      m = np.mean(d[np.arange(n), lab])
      if (m <= prev and m >= 0.999 * prev) or it == 20:
        break
      prev = m
      for c in range(40):
        mem = np.where(lab == c)[0]
        if mem.any():
          ref[c] = np.mean(e[mem], axis=0)
    assert np.array_equal(got, lab), metric
    np.testing.assert_allclose(cent, ref, rtol=1e-12, atol=1e-13, err_msg=metric)


# --- 7. determinism --------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "correlation"])
def test_two_calls_are_bit_identical(metric):
  e = so.blobs(8192, 256, 20, seed=45, noise=0.6)
  l1, c1, i1 = general(e, 20, metric)
  l2, c2, i2 = general(e, 20, metric)
  assert i1 == i2
  assert np.array_equal(l1, l2)
  assert c1.tobytes() == c2.tobytes()


# --- 8. errors -------------------------------------------------------------------------
def test_errors():
  g = golden("kmeans_dim.npz")
  e = g["e_a"]
  with pytest.raises(sca.UnsupportedOnDeviceError):
    ckm.run_kmeans(e, 4, "mahalanobis", 10)
  with pytest.raises(sca.UnsupportedOnDeviceError):
    ckm.run_kmeans(e, 4, lambda u, v: 0.0, 10)
  for falsy in (None, ""):
    with pytest.raises(_lib.NotFittedError):
      ckm.run_kmeans(e, 4, falsy, 10)
  with pytest.raises(ValueError):
    ckm.run_kmeans(e, 4, "cosine", 0)
  with pytest.raises(ValueError):
    ckm.run_kmeans(e[:3], 4, "cosine", 10)
  cent = g["init_a"].copy()
  with pytest.raises(sca.UnsupportedOnDeviceError):
    ckm.CustomKMeans(4, centroids=cent, custom_dist="mahalanobis").predict(e)
  with pytest.raises(sca.UnsupportedOnDeviceError):
    ckm.CustomKMeans(4, centroids=cent.astype(np.float32)).predict(e)
  with pytest.raises(ValueError, match="should be >= n_clusters"):
    ckm.CustomKMeans(4, centroids=cent).predict(e[:3])
  with pytest.raises(ValueError, match="does not match the number of clusters"):
    ckm.CustomKMeans(3, centroids=cent).predict(e)
  assert np.array_equal(cent, g["init_a"])
  # the C entry's own checks
  h = _lib.default_handle()
  x = np.ascontiguousarray(e)
  lab = np.empty(1000, dtype=np.int64)
  it = ctypes.c_int(0)
  for n, dim, k, max_iter, metric in ((1000, 6, 4, 0, 0), (3, 6, 4, 10, 0), (1000, 0, 4, 10, 0),
                                      (1000, 6, 0, 10, 0)):
    rc = h.lib.sc_stage_kmeans_general(h.raw, _lib.as_double_p(x), n, dim, k, max_iter, metric,
                                       0.001, None, _lib.as_int64_p(lab), None, ctypes.byref(it))
    assert rc == _lib.SC_ERR_INVALID
  rc = h.lib.sc_stage_kmeans_general(h.raw, _lib.as_double_p(x), 1000, 6, 4, 10, 8, 0.001, None,
                                     _lib.as_int64_p(lab), None, ctypes.byref(it))
  assert rc == _lib.SC_ERR_UNSUPPORTED
