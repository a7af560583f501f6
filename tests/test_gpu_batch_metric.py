"""GPU: predict_batch(..., batch_any_metric=True) under a custom_dist other than cosine takes the
short route (n <= 128) and the lockstep groups (128 < n < 4096) as a cosine batch does, and gives
predict()'s labels; without the flag the batch is what it was (routes all 0, predict()'s labels
bit for bit).  Well-separated blobs (noise 0.1 in d = 16): no assignment or stop-rule decision of
the k-means is near a tie, which is what equal labels between the batch's chain and predict()'s
single-workgroup kernel need."""
import numpy as np
import pytest

import spectralcluster_amd as sca
from oracle import spectral_oracle as so
from spectralcluster_amd import fallback_clusterer as fb
from spectralcluster_amd import utils

pytestmark = pytest.mark.gpu

NS = [20, 64, 128, 129, 300]
ROUTES = [2, 2, 2, 1, 1]
METRICS = ["euclidean", "cityblock", "correlation"]


def batch():
  return [so.blobs(n, 16, 3 + i % 2, seed=4100 + i, noise=0.1) for i, n in enumerate(NS)]


def icassp(**kw):
  return sca.SpectralClusterer(
      min_clusters=kw.pop("min_clusters", 2), max_clusters=7,
      refinement_options=sca.configs.icassp2018_refinement_options, **kw)


def assert_predicts_labels(got, want_of, utts):
  for i, (lab, u) in enumerate(zip(got, utts)):
    want = want_of(i, u)
    assert lab.shape == want.shape, i
    assert np.array_equal(utils.enforce_ordered_labels(lab),
                          utils.enforce_ordered_labels(want)), (i, u.shape)


@pytest.mark.parametrize("metric", METRICS)
def test_the_flag_routes_a_metric_batch_like_a_cosine_one(metric):
  utts = batch()
  c = icassp(custom_dist=metric)
  got = c.predict_batch(utts, group=16, batch_any_metric=True)
  assert c.last_batch_routes == ROUTES, c.last_batch_routes
  assert_predicts_labels(got, lambda i, u: c.predict(u), utts)
  # the same list gives the same results, and the permission does not outlive the call
  again = c.predict_batch(utts, group=16, batch_any_metric=True)
  for a, b in zip(got, again):
    assert np.array_equal(a, b)
  c.predict_batch(utts, group=16)
  assert c.last_batch_routes == [0] * len(NS)


@pytest.mark.parametrize("metric", METRICS)
def test_without_the_flag_nothing_changes(metric):
  utts = batch()
  c = icassp(custom_dist=metric)
  got = c.predict_batch(utts, group=16)
  assert c.last_batch_routes == [0] * len(NS)
  for u, lab in zip(utts, got):
    assert np.array_equal(lab, c.predict(u))


def test_constrained_batch():
  """Speaker-turn bands, AffinityIntegration after the Turn-to-Diarize refinement (a symmetric
  operator: the configuration tests/test_gpu_batch_constrained.py routes for cosine)."""
  def clusterer(metric):
    return sca.SpectralClusterer(
        min_clusters=2, max_clusters=7, custom_dist=metric,
        laplacian_type=sca.LaplacianType.GraphCut, row_wise_renorm=True,
        refinement_options=sca.RefinementOptions(
            p_percentile=0.9, thresholding_type=sca.ThresholdType.Percentile,
            thresholding_with_binarization=True, thresholding_preserve_diagonal=True,
            symmetrize_type=sca.SymmetrizeType.Average,
            refinement_sequence=sca.TURNTODIARIZE_REFINEMENT_SEQUENCE),
        constraint_options=sca.ConstraintOptions(
            constraint_name=sca.ConstraintName.AffinityIntegration,
            apply_before_refinement=False, integration_type=sca.IntegrationType.Max))
  utts, cms = [], []
  for n in NS:
    x, _, scores = so.turn_blobs(n, 24, 3, seed=500 + n, noise=0.3)
    utts.append(x)
    cms.append(sca.ConstraintMatrix([float(v) for v in scores], 1))
  cosine = clusterer("cosine")
  cosine.predict_batch(utts, group=16, constraint_matrices=cms)
  assert cosine.last_batch_routes == ROUTES, cosine.last_batch_routes
  c = clusterer("euclidean")
  got = c.predict_batch(utts, group=16, constraint_matrices=cms, batch_any_metric=True)
  assert c.last_batch_routes == ROUTES, c.last_batch_routes
  assert_predicts_labels(got, lambda i, u: c.predict(u, cms[i]), utts)
  c.predict_batch(utts, group=16, constraint_matrices=cms)
  assert c.last_batch_routes == [0] * len(NS)


def test_min_clusters_1_batch():
  utts = batch() + [so.blobs(90, 16, 1, seed=4200, noise=0.1)]
  c = icassp(custom_dist="euclidean", min_clusters=1, fallback_options=fb.FallbackOptions(
      single_cluster_condition=fb.SingleClusterCondition.AllAffinity,
      single_cluster_affinity_threshold=0.75))
  got = c.predict_batch(utts, group=16, batch_any_metric=True)
  assert c.last_batch_routes == ROUTES + [2], c.last_batch_routes
  assert len(c.last_batch_single) == len(utts)
  assert_predicts_labels(got, lambda i, u: c.predict(u), utts)
  c.predict_batch(utts, group=16)
  assert c.last_batch_routes == [0] * len(utts) and c.last_batch_single is None


def test_predict_affinity_batch():
  utts = batch()
  mats = [utils.compute_affinity_matrix(u) for u in utts]
  c = icassp(custom_dist="euclidean")
  got = c.predict_affinity_batch(mats, batch_any_metric=True)
  assert c.last_batch_routes == ROUTES, c.last_batch_routes
  assert_predicts_labels(got, lambda i, u: c.predict_affinity(mats[i]), utts)
  c.predict_affinity_batch(mats)
  assert c.last_batch_routes == [0] * len(NS)
