"""CPU: the traced k-means reference of tests/_kmeans_ref.py is right (against sklearn itself,
against spectral_oracle.run_kmeans and the kmeans.npz goldens), and every input that
tests/test_gpu_kmeans_kernels.py commits meets the conditions that test relies on: decision
margins, the cap on rows too close to a tie, pass-count coverage, exactness of the exact-arithmetic
inputs in any summation order.  No GPU call is made."""

import numpy as np
import pytest

import _kmeans_ref as kr
import spectral_oracle as so
from conftest import golden


def _sklearn_centers(e, k):
  from sklearn.cluster import KMeans
  return KMeans(n_clusters=k, init="k-means++", max_iter=1, random_state=0,
                n_init="auto").fit(e).cluster_centers_


SKLEARN_CASES = [(129, 3, 3.0, 1), (300, 9, 3.0, 1), (700, 21, 1.0, 1), (300, 33, 1.0, 1),
                 kr.ROW0_ALONE_CASE, kr.EMPTY_CLUSTER_CASE]


@pytest.mark.parametrize("case", SKLEARN_CASES, ids=str)
def test_trace_seeding_is_sklearns(case):
  e = kr.overlap_input(case)
  k = case[1]
  want = _sklearn_centers(np.array(e), k)
  plain = kr.trace(e, k, 300, np.float64)
  # the float64 trace spells sklearn's arithmetic; BLAS may add a dot product in another order
  np.testing.assert_allclose(plain["lloyd_centroids"], want, rtol=0, atol=1e-12)
  ref = kr.overlap_reference(case)[0]
  np.testing.assert_allclose(ref["lloyd_centroids"].astype(np.float64), want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", kr.all_overlap_cases(), ids=str)
def test_trace_labels_are_run_kmeans(case):
  e = kr.overlap_input(case)
  k = case[1]
  ref, plain, _ = kr.overlap_reference(case)
  want = so.run_kmeans(np.array(e), k, 300)
  assert np.array_equal(plain["labels"], want)
  assert np.array_equal(ref["labels"], want)
  assert np.array_equal(plain["lloyd_centroids"], so.sklearn_init_centroids(np.array(e), k))


def test_trace_against_the_kmeans_goldens():
  g = golden("kmeans.npz")
  for tag in "abcd":
    e = g["e_" + tag]
    k = e.shape[1]
    for dtype in (np.float64, kr.LD):
      t = kr.trace(e, k, 300, dtype)
      np.testing.assert_allclose(t["lloyd_centroids"].astype(np.float64), g["centers_" + tag],
                                 rtol=0, atol=1e-12)
      assert np.array_equal(t["labels"], g["labels_" + tag])


@pytest.mark.parametrize("case", kr.all_overlap_cases(), ids=str)
def test_committed_inputs_meet_the_margin_and_cap_conditions(case):
  ref, plain, tol = kr.overlap_reference(case)
  # every seeding, Lloyd-assignment and stop-rule decision is MARGIN away from the other outcome
  # (float64 reordering noise is of order n * 1e-16)
  assert kr.decision_margin(ref) >= kr.MARGIN
  # ... so the plain float64 oracle takes the same decisions
  assert np.array_equal(ref["seeds"], plain["seeds"])
  assert ref["iterations"] == plain["iterations"]
  for a, b in zip(ref["rounds"], plain["rounds"]):
    assert np.array_equal(a["candidates"], b["candidates"]) and a["winner"] == b["winner"]
  # rows closer to a tie than the distance tolerance: at most 1 % in any pass
  for unsure in kr.uncertain_rows(ref, tol["mean_dist"][0]):
    assert np.mean(unsure) <= kr.LABEL_CAP
  # the tolerances come from the two host computations alone and are of rounding size
  for name, (t, yard) in tol.items():
    assert 0.0 < t < 1e-12 and yard <= t, (name, t, yard)


def test_pass_count_coverage():
  """Reference pass counts <= 4, 5-8 and >= 9 all occur, for the chain and in one group."""
  counts = [kr.overlap_reference(c)[0]["iterations"] for c in kr.OVERLAP_CASES]
  assert any(c <= 4 for c in counts)
  assert any(5 <= c <= 8 for c in counts)
  assert any(c >= 9 for c in counts)
  group = [kr.overlap_reference(c)[0]["iterations"] for c in kr.GROUP_MEMBERS]
  # the members finish in different enqueues of the grouped chain (passes 0 | 1-3 | 4-7 | ...)
  assert len({(c + 3) // 4 for c in group}) >= 3, group


def test_custom_loop_cases_are_what_they_claim():
  ref = kr.overlap_reference(kr.ROW0_ALONE_CASE)[0]
  assert ref["row0_alone"] and kr.ROW0_ALONE_CASE[0] <= 200
  ref = kr.overlap_reference(kr.EMPTY_CLUSTER_CASE)[0]
  assert ref["empty_in_loop"] and kr.EMPTY_CLUSTER_CASE[0] <= 200
  full = kr.overlap_reference(kr.MAX_ITER_CASE)[0]
  assert kr.MAX_ITER_CASE[2] == 3.0 and full["iterations"] > 9  # every max_iter below cuts it short
  for max_iter in (1, 2, 3, 4, 5, 8):
    cut = kr.trace(kr.overlap_input(kr.MAX_ITER_CASE), kr.MAX_ITER_CASE[1], max_iter)
    assert cut["iterations"] == max_iter + 1
    assert np.array_equal(cut["labels"], full["passes"][max_iter]["labels"])
    assert np.array_equal(cut["centroids"], full["passes"][max_iter]["centroids"])


@pytest.mark.parametrize("name", sorted(kr.EXACT_CASES))
def test_exact_inputs_are_exact_in_any_order(name):
  """Through the Lloyd step the trace of an exact-arithmetic input has the same bits whatever the
  order of its sums (rows permuted in every sum over rows, columns permuted in every dot
  product) and whatever the precision."""
  e = kr.exact_input(name)
  n, k = e.shape
  assert np.all(e == np.round(e)) and np.all(e.sum(axis=0) == 0)
  assert not np.any(np.all(e == 0, axis=1))  # the cosine distance takes no zero row
  base = kr.trace(e, k, 300, np.float64)
  rng = np.random.default_rng(5)
  cols = rng.permutation(k)
  variants = [kr.trace(e, k, 300, np.float64, row_order=rng.permutation(n)),
              kr.trace(e, k, 300, np.float64, row_order=np.arange(n)[::-1]),
              kr.trace(e, k, 300, kr.LD)]
  permuted = kr.trace(e[:, cols], k, 300, np.float64, row_order=rng.permutation(n))
  permuted["lloyd_centroids"] = permuted["lloyd_centroids"][:, np.argsort(cols)]
  permuted["col_means"] = permuted["col_means"][np.argsort(cols)]
  for t in variants + [permuted]:
    assert np.array_equal(t["seeds"], base["seeds"])
    assert np.array_equal(t["col_means"].astype(np.float64), base["col_means"])
    assert np.all(base["col_means"] == 0)
    for a, b in zip(t["rounds"], base["rounds"]):
      assert np.array_equal(a["candidates"], b["candidates"]) and a["winner"] == b["winner"]
      assert np.array_equal(a["trial_potentials"].astype(np.float64), b["trial_potentials"])
    assert np.array_equal(t["lloyd_labels"], base["lloyd_labels"])
    if t["lloyd_centroids"].dtype == np.float64:  # (a quotient rounds once per precision)
      assert np.array_equal(t["lloyd_centroids"], base["lloyd_centroids"])


def test_zero_potential_inputs_reach_the_corner():
  for name in ("zero_potential_60x4", "zero_potential_64x4", "zero_potential_260x9"):
    e = kr.exact_input(name)
    t = kr.trace(e, e.shape[1], 300, np.float64)
    assert t["rounds"][-1]["pot"] == 0.0                  # exactly zero potential
    assert np.all(t["rounds"][-1]["candidates"] == 0)      # searchsorted(zeros, 0) = 0
    assert len(set(t["seeds"].tolist())) < e.shape[1] or \
        len(np.unique(e[t["seeds"]], axis=0)) < e.shape[1]  # two centres coincide ...
    assert len(np.unique(t["lloyd_labels"])) < e.shape[1]  # ... and one has no member
  e = kr.exact_input("dup_row0_rowlast_200x5")
  assert np.sum(np.all(e == e[0], axis=1)) > 1 and np.sum(np.all(e == e[-1], axis=1)) > 1
