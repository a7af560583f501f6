"""k-means on embeddings whose width differs from the cluster count, host side (no GPU):

* the oracle -- `spectral_oracle.sklearn_init_centroids` for the seeds, then the reference's
  custom loop on scipy's cdist -- reproduces the real reference's labels in
  tests/golden/kmeans_dim.npz (tools/make_kmeans_dim_golden.py), which makes it the live checker
  of the large GPU cases in tests/test_gpu_kmeans_dim.py;
* `custom_distance_kmeans.CustomKMeans` has the reference dataclass's fields and validates its
  input with the reference's messages before it touches a device.
"""

import dataclasses

import numpy as np
import pytest
from scipy.spatial.distance import cdist

import spectral_oracle as so
from conftest import golden

import spectralcluster_amd as sca
from spectralcluster_amd import custom_distance_kmeans as ckm

K = {"a": 4, "b": 5, "c": 6, "d": 8}


def custom_loop(e, cent, metric, max_iter, tol=0.001):
  """reference custom_distance_kmeans.py:118-141 on a copy of `cent`: (labels, centroids)."""
  n = e.shape[0]
  cent = cent.copy()
  prev = 0
  labels = None
  for it in range(max_iter + 1):
    dist = cdist(e, cent, metric=metric)
    labels = dist.argmin(axis=1)
    mean_d = np.mean(dist[np.arange(n), labels])
    if (mean_d <= prev and mean_d >= (1 - tol) * prev) or it == max_iter:
      break
    prev = mean_d
    for c in range(cent.shape[0]):
      members = np.where(labels == c)[0]
      if members.any():
        cent[c] = np.mean(e[members], axis=0)
  return labels, cent


def _label_keys():
  return sorted(f for f in golden("kmeans_dim.npz") if f.startswith("labels_"))


@pytest.mark.parametrize("key", _label_keys())
def test_oracle_reproduces_reference_labels(key):
  g = golden("kmeans_dim.npz")
  _, tag, metric = key.split("_", 2)
  e = g["e_" + tag].astype(np.float64)
  assert e.shape[1] != K[tag]
  labels, _ = custom_loop(e, so.sklearn_init_centroids(e, K[tag]), metric, 300)
  assert np.array_equal(labels, g[key])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_oracle_loop_reproduces_reference_custom_kmeans(tag):
  g = golden("kmeans_dim.npz")
  for metric in ("cosine", "euclidean", "correlation", "canberra"):
    labels, cent = custom_loop(g["e_" + tag], g["init_" + tag], metric, 10)
    assert np.array_equal(labels, g["ck_%s_%s_labels" % (tag, metric)])
    np.testing.assert_allclose(cent, g["ck_%s_%s_cent" % (tag, metric)], rtol=1e-12,
                               atol=1e-13)


def test_golden_stays_small():
  import os
  path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmeans_dim.npz")
  assert os.path.getsize(path) <= 1 << 20


def test_custom_kmeans_fields_match_the_reference():
  fields = [(f.name, f.default) for f in dataclasses.fields(ckm.CustomKMeans)]
  assert [name for name, _ in fields] == ["n_clusters", "centroids", "max_iter", "tol",
                                         "custom_dist"]
  assert [default for _, default in fields] == [None, None, 10, 0.001, "cosine"]
  km = ckm.CustomKMeans(3)
  assert (km.n_clusters, km.centroids, km.max_iter, km.tol, km.custom_dist) == (
      3, None, 10, 0.001, "cosine")
  # not lifted to the package level (the reference does not export it either)
  assert not hasattr(sca, "CustomKMeans")


def test_custom_kmeans_validation_before_any_device_call():
  e = np.arange(24, dtype=np.float64).reshape(8, 3)
  with pytest.raises(ValueError, match=r"^Number of iterations should be a positive number, "
                     r"got 0 instead$"):
    ckm.CustomKMeans(2, max_iter=0).predict(e)
  with pytest.raises(ValueError, match=r"^n_samples=8 should be >= n_clusters=9$"):
    ckm.CustomKMeans(9).predict(e)
  with pytest.raises(ValueError, match=r"^The shape of the initial centroids \(\(3, 3\)\)"
                     r"does not match the number of clusters 2$"):
    ckm.CustomKMeans(2, centroids=np.zeros((3, 3))).predict(e)
  with pytest.raises(ValueError, match=r"^The number of features of the initial centroids 4"
                     r"does not match the number of features of the data 3\.$"):
    ckm.CustomKMeans(2, centroids=np.zeros((2, 4))).predict(e)
  # the reference's order: max_iter before the sample count before the centroid shapes
  with pytest.raises(ValueError, match="Number of iterations"):
    ckm.CustomKMeans(9, centroids=np.zeros((3, 4)), max_iter=-1).predict(e)
  with pytest.raises(ValueError, match="n_samples=8"):
    ckm.CustomKMeans(9, centroids=np.zeros((3, 4))).predict(e)
  # a 1-D input fails the shape unpacking, as in the reference
  with pytest.raises(ValueError):
    ckm.CustomKMeans(2).predict(np.zeros(5))


def test_custom_kmeans_device_limits_raise_before_any_device_call():
  e = np.arange(24, dtype=np.float64).reshape(8, 3)
  cent = e[:2].copy()
  with pytest.raises(sca.UnsupportedOnDeviceError):
    ckm.CustomKMeans(2, centroids=cent, custom_dist="mahalanobis").predict(e)
  with pytest.raises(sca.UnsupportedOnDeviceError):
    ckm.CustomKMeans(2, centroids=cent, custom_dist=lambda u, v: 0.0).predict(e)
  with pytest.raises(sca.UnsupportedOnDeviceError, match="float64"):
    ckm.CustomKMeans(2, centroids=cent.astype(np.float32)).predict(e)
  # scipy's cdist errors for a metric that is neither a name nor a function, and for ""
  with pytest.raises(TypeError):
    ckm.CustomKMeans(2, centroids=cent, custom_dist=None).predict(e)
  with pytest.raises(ValueError, match="Unknown Distance Metric"):
    ckm.CustomKMeans(2, centroids=cent, custom_dist="").predict(e)
  assert np.array_equal(cent, e[:2])  # untouched
