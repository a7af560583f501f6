"""CPU: the metric trace of tests/_kmeans_metric_ref.py is right -- its float64 labels are
spectral_oracle.run_kmeans_metric's (scipy's cdist inside sklearn's seeds) on every input of
tests/test_gpu_kmeans_metric_chain.py and on the kmeans_metrics.npz goldens, its distances are
scipy's -- and every input meets the conditions the GPU test relies on: decision margins, the cap
on rows too close to a tie.  An input that fails is replaced, never exempted.  No GPU call."""

import numpy as np
import pytest

import _kmeans_metric_ref as mr
import _kmeans_ref as kr
import spectral_oracle as so
from conftest import golden

PAIRS = [(m, c) for m in mr.METRICS for c in mr.cases_of(m)]
IDS = ["%s-%s" % (m, c) for m, c in PAIRS]


@pytest.mark.parametrize("metric,case", PAIRS, ids=IDS)
def test_trace_labels_are_run_kmeans_metric(metric, case):
  e = np.array(kr.overlap_input(case))
  ref, plain, _ = mr.metric_reference(case, metric)
  want = so.run_kmeans_metric(e, case[1], 300, metric)
  assert np.array_equal(plain["labels"], want)
  assert np.array_equal(ref["labels"], want)
  assert ref["iterations"] == plain["iterations"]


@pytest.mark.parametrize("metric", mr.METRICS)
def test_trace_against_the_metric_goldens(metric):
  g = golden("kmeans_metrics.npz")
  for tag in "abc":
    e = g["e_" + tag]
    k = e.shape[1]
    if metric == "correlation" and k == 2:
      continue  # (every distance is 0 or 2 up to rounding: mr.cases_of)
    for dtype in (np.float64, kr.LD):
      t = mr.trace_metric(e, k, metric, 300, dtype)
      assert np.array_equal(t["labels"], g["labels_%s_%s" % (tag, metric)]), (tag, dtype)


@pytest.mark.parametrize("metric,case", PAIRS, ids=IDS)
def test_distances_are_scipys(metric, case):
  """Bound: a distance is a sum of k non-negative terms (or, for correlation, 1 - a quotient of
  such sums of magnitude <= 1), each term rounded a few times; two orders of adding them differ
  by at most k eps relative to the sum, the terms themselves by a few eps -- 4 k eps of
  max(|d|, 1)."""
  from scipy.spatial.distance import cdist
  e = np.array(kr.overlap_input(case))
  k = case[1]
  plain = mr.metric_reference(case, metric)[1]
  for p in (plain["passes"][0], plain["passes"][-1]):
    got = mr.metric_cdist(e, p["centroids"], metric)
    want = cdist(e, p["centroids"], metric=metric)
    bound = 4 * k * np.finfo(np.float64).eps * np.maximum(np.abs(want), 1.0)
    assert np.all(np.abs(got - want) <= bound), float(np.max(np.abs(got - want) / bound))


@pytest.mark.parametrize("metric,case", PAIRS, ids=IDS)
def test_inputs_meet_the_margin_and_cap_conditions(metric, case):
  ref, plain, tol = mr.metric_reference(case, metric)
  assert kr.decision_margin(ref) >= kr.MARGIN
  assert np.array_equal(ref["seeds"], plain["seeds"])
  assert ref["iterations"] == plain["iterations"]
  for a, b in zip(ref["passes"], plain["passes"]):
    assert np.array_equal(a["labels"], b["labels"])
  for unsure in kr.uncertain_rows(ref, tol["mean_dist"][0]):
    assert np.mean(unsure) <= kr.LABEL_CAP
  # the tolerances come from the two host computations alone and are of rounding size relative
  # to the quantity (a squared Euclidean distance of k = 32 columns is of order 10^2)
  for name, (t, yard) in tol.items():
    scale = max(1.0, float(np.max(np.abs(np.asarray(ref[name], dtype=np.float64)))))
    assert 0.0 < t < 1e-12 * scale and yard <= t, (name, t, yard)


def test_the_traces_run_few_and_many_passes():
  counts = [mr.metric_reference(c, m)[0]["iterations"] for m, c in PAIRS]
  assert min(counts) <= 4 and max(counts) >= 9, counts


def test_max_iter_cuts_the_euclidean_run():
  case = mr.MAX_ITER_CASE
  full = mr.metric_reference(case, "euclidean")[0]
  assert full["iterations"] > 6
  assert kr.decision_margin(full) >= kr.MARGIN
  for max_iter in (1, 2, 5):
    cut = mr.metric_reference(case, "euclidean", max_iter)[0]
    assert cut["iterations"] == max_iter + 1
    assert np.array_equal(cut["labels"], full["passes"][max_iter]["labels"])
