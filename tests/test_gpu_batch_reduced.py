"""GPU: size reduction and the too-few-embeddings fallback of a whole batch in one library call
(sc_batch_ahc, sc_predict_batch_reduced).

The batched agglomerative clustering is compared with LIVE sklearn (`so.agglomerative`), label
numbering included, the centroids with `np.mean` bit for bit, and predict_batch with the oracle's
composite of the reference's own steps (spectral_clusterer.py:170-199) and with outputs of the real
reference (tests/golden/size_reduction.npz, fallback.npz).

Labels are compared for equality although the distances come from an fp64 GEMM and sklearn's from
pdist: for every (n, d, n_clusters or threshold) below, sklearn's labels on pdist equal its labels
on 1 - clip(Xn Xn^T) from a NumPy product (metric="precomputed"), so a last-bit difference in a
distance moves no merge.  The sizes sit around the LDS kernel's bound (128), the 128-row GEMM tile
and the 1024-thread stride of the chain.
"""

import functools

import numpy as np
import pytest
import torch

import spectral_oracle as so
from conftest import golden

import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import fallback_clusterer as fb
from spectralcluster_amd import utils

pytestmark = pytest.mark.gpu

COMPLETE_N = (2, 3, 17, 64, 65, 127, 128, 129, 300, 777, 1023, 1024, 1025, 1500)
AVERAGE_N = (2, 3, 5, 33, 63, 64, 65, 96, 127, 128, 129, 199)


@functools.lru_cache(maxsize=None)
def complete_input(n, d):
  x = so.blobs(n, d, 4, seed=1000 * d + n)
  x.setflags(write=False)
  return x


@functools.lru_cache(maxsize=None)
def complete_reference(n, d, k):
  """sklearn's labels and np.mean's centroids, computed once and shared"""
  x = complete_input(n, d)
  labels = so.agglomerative(x, n_clusters=k, linkage="complete")
  return labels, so.get_cluster_centroids(x, labels)


@functools.lru_cache(maxsize=None)
def average_input(n, d):
  x = so.blobs(n, d, 3, seed=2000 * d + n)
  x.setflags(write=False)
  return x


def icassp_options(sigma=1):
  return sca.RefinementOptions(
      gaussian_blur_sigma=sigma, p_percentile=0.95, thresholding_soft_multiplier=0.01,
      thresholding_type=sca.ThresholdType.RowMax,
      refinement_sequence=sca.ICASSP2018_REFINEMENT_SEQUENCE)


def assert_complete_batch(d, k):
  ns = [n for n in COMPLETE_N if n > k]
  labels, centroids = utils.cosine_agglomerative_clustering_batch(
      [complete_input(n, d) for n in ns], n_clusters=k, return_centroids=True)
  assert len(labels) == len(centroids) == len(ns)
  for n, lab, cen in zip(ns, labels, centroids):
    want_labels, want_centroids = complete_reference(n, d, k)
    assert lab.dtype == np.int64 and np.array_equal(lab, want_labels), (n, d, k)
    assert cen.shape == (k, d) and np.array_equal(cen, want_centroids), (n, d, k)


# --- 1: the batched AHC against live sklearn -----------------------------------------------
@pytest.mark.parametrize("k", [2, 40, 100, 128, 129])
@pytest.mark.parametrize("d", [3, 16, 24])
def test_batch_ahc_complete_linkage_vs_sklearn(d, k):
  assert_complete_batch(d, k)
  # labels alone: the same call without the centroid step
  ns = [n for n in COMPLETE_N if n > k][:4]
  got = utils.cosine_agglomerative_clustering_batch([complete_input(n, d) for n in ns],
                                                    n_clusters=k)
  for n, lab in zip(ns, got):
    assert np.array_equal(lab, complete_reference(n, d, k)[0])


# --- 2: average linkage cut at a threshold: 129 and 199 take the global-memory chain, the
#        rest the LDS kernel, in the same call ------------------------------------------------
@pytest.mark.parametrize("threshold", [0.3, 0.5])
@pytest.mark.parametrize("d", [3, 16])
def test_batch_ahc_average_linkage_by_threshold_vs_sklearn(d, threshold):
  xs = [average_input(n, d) for n in AVERAGE_N]
  got, centroids = utils.cosine_agglomerative_clustering_batch(
      xs, linkage="average", distance_threshold=threshold, return_centroids=True)
  for n, x, lab, cen in zip(AVERAGE_N, xs, got, centroids):
    want = so.agglomerative(x, linkage="average", distance_threshold=threshold)
    assert np.array_equal(lab, want), (n, d, threshold)
    assert np.array_equal(cen, so.get_cluster_centroids(x, want)), (n, d, threshold)


# --- 3: waves ---------------------------------------------------------------------------------
def test_batch_ahc_in_several_waves_and_a_member_beyond_the_budget(handle):
  """10 MiB per wave at d = 16, k = 40: the distance matrix of 1500 rows alone is 1500 x 1504 x
  8 B = 17.2 MiB (that member runs sc_ahc's own path inside the call), those of 1025, 1024 and
  1023 rows are 8.1 MiB each (a wave each), and 777 rows and below (4.7 MiB + ...) share the
  last: four waves and a single member."""
  assert handle.lib.sc_set_reduce_wave_bytes(handle.raw, 10 << 20) == _lib.SC_OK
  try:
    assert_complete_batch(16, 40)
  finally:
    assert handle.lib.sc_set_reduce_wave_bytes(handle.raw, 0) == _lib.SC_OK
  assert_complete_batch(16, 40)


# --- 4: mixed inputs --------------------------------------------------------------------------
def test_batch_ahc_mixed_sources_equal_the_widened_float64_arrays():
  a = so.blobs(300, 16, 4, seed=11)
  b = so.blobs(129, 16, 4, seed=12).astype(np.float32)
  c = torch.from_numpy(so.blobs(200, 16, 4, seed=13)).to(torch.float16)
  wide = so.blobs(150, 40, 4, seed=14)
  view = wide[:, 3:35:2]  # 16 columns, a column stride of 2
  widened = [a, b.astype(np.float64), c.to(torch.float64).numpy(), np.ascontiguousarray(view)]
  want, want_centroids = utils.cosine_agglomerative_clustering_batch(
      widened, n_clusters=40, return_centroids=True)
  got, got_centroids = utils.cosine_agglomerative_clustering_batch(
      [a, b, c.cuda(), view], n_clusters=40, return_centroids=True)
  for i in range(4):
    assert np.array_equal(got[i], want[i]), i
    assert np.array_equal(got_centroids[i], want_centroids[i]), i
    assert np.array_equal(want[i], so.agglomerative(widened[i], n_clusters=40)), i


# --- 5: end to end against the oracle ---------------------------------------------------------
def composite(x, mss):
  """the reference's steps (spectral_clusterer.py:170-199) on the oracle"""
  if x.shape[0] <= mss:
    return so.predict(x, so.icassp2018_config())
  pre = so.agglomerative(x, mss)
  return so.chain_labels(pre, so.predict(so.get_cluster_centroids(x, pre),
                                         so.icassp2018_config()))


def assert_reduced_batch(c, utts, mss):
  got = c.predict_batch(utts)
  kinds = [1 if u.shape[0] > mss else 0 for u in utts]
  assert c.last_batch_reduced == kinds
  assert len(c.last_batch_routes) == len(utts) and 0 not in c.last_batch_routes
  for u, lab, kind, diag in zip(utts, got, kinds, c.last_batch_diags):
    assert lab.dtype == (np.float64 if kind else np.int64)
    assert lab.shape == (u.shape[0],)
    assert so.adjusted_rand_index(lab.astype(int), composite(u, mss).astype(int)) == 1.0
    assert diag.n == min(u.shape[0], mss)  # the spectral run's: the centroids' when reduced
  return got


def test_predict_batch_with_size_reduction_vs_the_oracle_and_the_reference_golden():
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=7, max_spectral_size=200,
                            refinement_options=icassp_options())
  utts = [so.blobs(n, 32, 5, seed) for n, seed in
          ((150, 40), (200, 41), (201, 42), (333, 43), (700, 44), (1500, 91))]
  got = assert_reduced_batch(c, utts, 200)
  assert c.last_batch_reduced == [0, 0, 1, 1, 1, 1]
  want = golden("size_reduction.npz")["labels_a"]
  assert so.adjusted_rand_index(got[5].astype(int), want.astype(int)) == 1.0


def test_predict_batch_with_reduction_to_the_short_route():
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=7, max_spectral_size=100,
                            refinement_options=icassp_options())
  utts = [so.blobs(n, 16, 3, seed) for n, seed in ((129, 50), (300, 51), (640, 52), (1025, 53))]
  assert_reduced_batch(c, utts, 100)
  assert c.last_batch_reduced == [1, 1, 1, 1]
  assert c.last_batch_routes == [_lib.BATCH_ROUTE_GROUP_JACOBI] * 4  # 100 centroids each


# --- 6: the fallback in the batch -------------------------------------------------------------
def fallback_clusterer(**kwargs):
  """the clusterer of tests/test_gpu_fallback.py"""
  return sca.SpectralClusterer(
      refinement_options=sca.RefinementOptions(
          gaussian_blur_sigma=1, p_percentile=0.95,
          refinement_sequence=sca.ICASSP2018_REFINEMENT_SEQUENCE),
      fallback_options=fb.FallbackOptions(
          spectral_min_embeddings=100,
          fallback_clusterer_type=fb.FallbackClustererType.Agglomerative,
          agglomerative_threshold=0.4), **kwargs)


def test_predict_batch_with_fallback_members():
  c = fallback_clusterer()
  utts = [so.blobs(80, 16, 3, 103, noise=0.2), so.blobs(150, 16, 3, 60), so.blobs(2, 16, 2, 61)]
  got = c.predict_batch(utts)
  assert [g.dtype for g in got] == [np.int64] * 3
  assert np.array_equal(got[0], golden("fallback.npz")["predict_few"])
  assert np.array_equal(got[2], so.agglomerative(utts[2], linkage="average",
                                                 distance_threshold=0.4))
  want = so.predict(utts[1], so.icassp2018_config(min_clusters=None, max_clusters=None))
  assert so.adjusted_rand_index(got[1], want) == 1.0
  assert c.last_batch_reduced == [2, 0, 2]
  routes = c.last_batch_routes
  assert routes[0] == routes[2] == _lib.BATCH_ROUTE_FALLBACK == 3 and routes[1] != 0
  assert c.last_batch_diags[0].n == 0 and c.last_batch_diags[1].n == 150
  for u, lab in zip(utts, got):  # ... which is what predict() gives
    assert np.array_equal(lab, c.predict(u))


# --- 7: errors --------------------------------------------------------------------------------
def test_errors_before_any_launch_and_what_stays_the_loop():
  x = so.blobs(50, 8, 2, seed=1)
  with pytest.raises(ValueError, match="relatively big"):
    sca.SpectralClusterer(max_clusters=7, max_spectral_size=7).predict_batch([x[:7], x])
  c = fallback_clusterer()
  with pytest.raises(ValueError) as single:
    c.predict(x[:1])
  with pytest.raises(ValueError) as batch:
    c.predict_batch([x, x[:1]])
  assert str(batch.value) == str(single.value)
  with pytest.raises(ValueError, match="same d"):
    c.predict_batch([x, so.blobs(50, 9, 2, seed=2)])
  # the Naive fallback is not in the batch: predict() per member
  naive = sca.SpectralClusterer(
      min_clusters=2, max_clusters=7, refinement_options=icassp_options(),
      fallback_options=fb.FallbackOptions(spectral_min_embeddings=60))
  utts = [x, so.blobs(120, 8, 3, seed=3)]
  got = naive.predict_batch(utts)
  assert naive.last_batch_routes == [0, 0]
  for u, lab in zip(utts, got):
    assert np.array_equal(lab, naive.predict(u))


def test_a_zero_row_names_its_utterance_and_leaves_the_handle_usable():
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=7, max_spectral_size=100,
                            refinement_options=icassp_options())
  utts = [so.blobs(n, 16, 3, seed) for n, seed in ((129, 50), (300, 51), (90, 54))]
  bad = utts[1].copy()
  bad[17] = 0.0
  with pytest.raises(ValueError, match="utterance 1"):
    c.predict_batch([utts[0], bad, utts[2]])
  with pytest.raises(ValueError, match="utterance 1"):
    utils.cosine_agglomerative_clustering_batch([utts[0], bad], n_clusters=40)
  assert_reduced_batch(c, utts, 100)


# --- 8: sc_ahc's own guard --------------------------------------------------------------------
def test_single_ahc_refuses_a_zero_row_and_is_unchanged_for_finite_rows():
  g = golden("size_reduction.npz")
  bad = g["x_1000by6"].copy()
  bad[123] = 0.0
  with pytest.raises(ValueError, match="zero or non-finite row"):
    utils.cosine_agglomerative_clustering(bad, n_clusters=100)
  nan = g["x_1000by6"][:50].copy()
  nan[7, 2] = np.nan
  with pytest.raises(ValueError, match="zero or non-finite row"):
    utils.cosine_agglomerative_clustering(nan, linkage="average", distance_threshold=0.4)
  got = utils.cosine_agglomerative_clustering(g["x_1000by6"], n_clusters=100)
  assert np.array_equal(got, g["ahc_1000by6"])


# --- 9: the order of the batch does not matter -------------------------------------------------
def test_permuting_the_batch_permutes_the_results():
  c = sca.SpectralClusterer(
      min_clusters=2, max_clusters=7, max_spectral_size=100,
      refinement_options=icassp_options(),
      fallback_options=fb.FallbackOptions(
          spectral_min_embeddings=50,
          fallback_clusterer_type=fb.FallbackClustererType.Agglomerative,
          agglomerative_threshold=0.4))
  utts = [so.blobs(n, 16, 3, seed) for n, seed in
          ((30, 70), (80, 71), (129, 72), (300, 73), (49, 74), (100, 75), (640, 76))]
  got = c.predict_batch(utts)
  kinds, routes = list(c.last_batch_reduced), list(c.last_batch_routes)
  assert kinds == [2, 0, 1, 1, 2, 0, 1]
  order = [4, 6, 0, 3, 5, 1, 2]
  again = c.predict_batch([utts[i] for i in order])
  assert c.last_batch_reduced == [kinds[i] for i in order]
  assert c.last_batch_routes == [routes[i] for i in order]
  for pos, i in enumerate(order):
    assert again[pos].dtype == got[i].dtype and np.array_equal(again[pos], got[i]), i
