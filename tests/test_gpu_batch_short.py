"""The short route of a grouped batch: utterances of n <= 128 share one dense Jacobi launch, a
workgroup per utterance (up to WIDTH utterances per launch), then the lockstep k-means of the
grouped route.  The kernel body, its arguments and the stages before it are the single call's,
so every utterance gets the eigenvalues and the labels of its own predict() call."""
import numpy as np
import pytest

import spectralcluster_amd as sca
from oracle import spectral_oracle as so
from spectralcluster_amd import _lib

pytestmark = pytest.mark.gpu

# Members of one Jacobi launch: kShortWidth of sc_internal.h as shipped.  A library built with the
# other width (SC_SHORT_WIDTH=16) cuts the same batches into more waves: 2 * WIDTH + 5 members are
# 2 full waves + 5 at 64 and 8 full waves + 5 at 16, WIDTH + 5 are 1 + 5 and 4 + 5 -- several
# waves, the last one partial, and more than the two arena banks, either way.
WIDTH = 64
JACOBI = 1  # SC_EIG_PATH_DENSE_JACOBI
LAPS = [None, sca.LaplacianType.GraphCut]


def icassp(**kw):
  return sca.SpectralClusterer(
      min_clusters=kw.pop("min_clusters", 2), max_clusters=kw.pop("max_clusters", 7),
      refinement_options=sca.configs.icassp2018_refinement_options, **kw)


def assert_same_as_single_calls(c, utts, got, routes=None, eig=True):
  diags = c.last_batch_diags
  if routes is not None:
    assert c.last_batch_routes == routes, c.last_batch_routes
  for i, u in enumerate(utts):
    want = c.predict(u)
    assert np.array_equal(got[i], want), (i, u.shape)
    if not eig:
      continue
    one = c.last_diag
    assert diags[i].n_clusters == one.n_clusters, i
    assert diags[i].n_clusters_raw == one.n_clusters_raw, i
    w, w1 = diags[i].eigenvalue_array(), one.eigenvalue_array()
    assert w.shape == w1.shape, i
    # Jacobi resolves every eigenvalue to n eps |A| ~ 1e-14 |A|; with the front and the kernel
    # body shared the difference is 0
    assert np.max(np.abs(w - w1)) <= 1e-10 * np.max(np.abs(w1)), (i, u.shape)
    # ... and 0 is what the shared front, kernel body and LDS carve-up give: no a * b + c is
    # contracted in one kernel and not in the other
    assert np.array_equal(w, w1), (i, u.shape, float(np.max(np.abs(w - w1))))


# m <= 96 keeps the vector accumulator in LDS, m >= 97 in global memory; odd m pads to m + 1;
# m <= 64 puts two pair rows on a wave
BOUNDARY_SIZES = [10, 17, 31, 63, 64, 65, 95, 96, 97, 98, 127, 128]


@pytest.mark.parametrize("lap", LAPS)
def test_every_boundary_of_the_kernel(lap):
  utts = [so.blobs(n, 24, k, seed=10 * n + k) for n in BOUNDARY_SIZES for k in (2, 3, 5)]
  c = icassp(laplacian_type=lap, max_clusters=7 if lap is None else 12)
  got = c.predict_batch(utts, group=16)
  assert c.last_batch_routes == [_lib.BATCH_ROUTE_GROUP_JACOBI] * len(utts)
  assert all(d.eig_path == JACOBI for d in c.last_batch_diags)
  assert_same_as_single_calls(c, utts, got)


def test_more_members_than_one_launch_and_uneven_waves():
  rng = np.random.default_rng(5)
  ns = [int(n) for n in rng.integers(12, 49, 2 * WIDTH + 3)] + [128, 97]
  utts = [so.blobs(n, 16, 2 + i % 3, seed=7000 + i) for i, n in enumerate(ns)]
  c = icassp()
  a = c.predict_batch(utts, group=16)
  assert c.last_batch_routes == [2] * len(utts)
  wa = [d.eigenvalue_array().copy() for d in c.last_batch_diags]
  assert_same_as_single_calls(c, utts, a, eig=False)
  b = c.predict_batch(utts, group=16)
  wb = [d.eigenvalue_array().copy() for d in c.last_batch_diags]
  rev = c.predict_batch(utts[::-1], group=3)[::-1]
  assert c.last_batch_routes == [2] * len(utts)
  for i in range(len(utts)):
    assert np.array_equal(a[i], b[i]) and np.array_equal(a[i], rev[i]), i
    assert np.array_equal(wa[i], wb[i]), i


def test_mixed_batch_reports_every_route():
  sizes = [60, 128, 129, 4100, 300, 17, 2047]
  utts = [so.blobs(n, 32, 3, seed=n) for n in sizes]
  c = icassp()
  got = c.predict_batch(utts, group=8)
  assert c.last_batch_routes == [2, 2, 1, 0, 1, 2, 1]
  for u, lab in zip(utts, got):
    assert np.array_equal(lab, c.predict(u))


ORACLE_SEED = 9100


def oracle_utterances():
  rng = np.random.default_rng(ORACLE_SEED)
  ns = rng.integers(20, 129, 24)
  ks = rng.integers(2, 6, 24)
  return [so.blobs(int(n), 32, int(k), seed=ORACLE_SEED + i) for i, (n, k) in enumerate(zip(ns, ks))]


@pytest.mark.parametrize("lap", LAPS)
def test_short_route_against_the_oracle(lap):
  """(seeds chosen so that no utterance's eigengap decision is a near tie in the oracle)"""
  utts = oracle_utterances()
  maxc = 7 if lap is None else 12
  code = so.LAPLACIAN_NONE if lap is None else so.LAPLACIAN_GRAPH_CUT
  c = icassp(laplacian_type=lap, max_clusters=maxc)
  got = c.predict_batch(utts, group=16)
  assert c.last_batch_routes == [2] * len(utts)
  for i, u in enumerate(utts):
    dump = {}
    want = so.predict(u, so.icassp2018_config(laplacian_type=code, max_clusters=maxc), dump)
    # the single call first: a failure says whether the route or the path is at fault
    assert so.adjusted_rand_index(c.predict(u), want) == 1.0, ("single call", i)
    assert so.adjusted_rand_index(got[i], want) == 1.0, ("short route", i)
    idx = so.consumed_eigen_indices(u.shape[0], maxc, lap is None, dump["eigenvalues"], 1e-2)
    w = c.last_batch_diags[i].eigenvalue_array()[idx]
    ref = dump["eigenvalues"][idx]
    assert np.max(np.abs(w - ref) / np.maximum(np.abs(ref), 1e-12)) < 1e-6, i


def groups_of_identical_rows(n, groups, seed):
  """`groups` runs of exactly identical embeddings (shares 3 : 2 or 5 : 3 : 2): the affinity has
  rank `groups`, every other eigenvalue of it is an exact multiple one"""
  rng = np.random.default_rng(seed)
  centres = np.eye(groups, 24) + 0.2 * rng.random((groups, 24))
  shares = {2: (0.6, 0.4), 3: (0.5, 0.3, 0.2)}[groups]
  counts = [int(round(s * n)) for s in shares[:-1]]
  counts.append(n - sum(counts))
  return np.vstack([np.tile(c, (m, 1)) for c, m in zip(centres, counts)])


def rows_repeated_three_times(n, k, seed):
  return np.repeat(so.blobs((n + 2) // 3, 24, k, seed=seed), 3, axis=0)[:n]


DEGENERATE_SIZES = [40, 96, 97, 128]


def degenerate_utterances():
  """exact duplicates at both accumulator placements of the kernel, ordinary members between
  them"""
  utts = []
  for n in DEGENERATE_SIZES:
    utts += [groups_of_identical_rows(n, 2, seed=n), so.blobs(n - 3, 24, 3, seed=8000 + n),
             groups_of_identical_rows(n, 3, seed=n + 1), rows_repeated_three_times(n, 3, seed=n + 2)]
  return utts


@pytest.mark.parametrize("lap", LAPS)
def test_exact_duplicates_on_the_short_route(lap):
  """predict_batch takes no matrix: spectra with exact multiplicities reach the kernel as
  embeddings with exact duplicates.  Same labels and eigenvalues as each member's own predict(),
  and the oracle's clustering."""
  utts = degenerate_utterances()
  maxc = 7 if lap is None else 12
  code = so.LAPLACIAN_NONE if lap is None else so.LAPLACIAN_GRAPH_CUT
  c = icassp(laplacian_type=lap, max_clusters=maxc)
  got = c.predict_batch(utts, group=16)
  assert c.last_batch_routes == [_lib.BATCH_ROUTE_GROUP_JACOBI] * len(utts)
  assert all(d.eig_path == JACOBI for d in c.last_batch_diags)
  assert_same_as_single_calls(c, utts, got)
  for i, u in enumerate(utts):
    want = so.predict(u, so.icassp2018_config(laplacian_type=code, max_clusters=maxc))
    assert so.adjusted_rand_index(got[i], want) == 1.0, (i, u.shape)


def option_utterances(seed, count=7, d=16):
  rng = np.random.default_rng(seed)
  return [so.blobs(int(n), d, int(k), seed=100 * seed + i)
          for i, (n, k) in enumerate(zip(rng.integers(20, 129, count), rng.integers(2, 6, count)))]


def expected_routes(c):
  return [2 if d.n_clusters <= 32 else 0 for d in c.last_batch_diags]


def test_row_wise_renorm_and_min_clusters():
  utts = option_utterances(21)
  c = icassp(row_wise_renorm=True, min_clusters=4)
  got = c.predict_batch(utts, group=16)
  assert_same_as_single_calls(c, utts, got, routes=[2] * len(utts))
  assert all(d.n_clusters >= 4 for d in c.last_batch_diags)


@pytest.mark.parametrize("lap", [sca.LaplacianType.Unnormalized, sca.LaplacianType.RandomWalk])
def test_the_other_laplacians(lap):
  utts = option_utterances(61)
  c = icassp(laplacian_type=lap, max_clusters=10)
  got = c.predict_batch(utts, group=16)
  assert_same_as_single_calls(c, utts, got, routes=expected_routes(c))
  assert 2 in c.last_batch_routes


def test_percentile_sequence_without_blur():
  opts = sca.RefinementOptions(
      p_percentile=0.9, thresholding_soft_multiplier=0.01,
      thresholding_type=sca.ThresholdType.Percentile,
      refinement_sequence=[sca.RefinementName.RowWiseThreshold, sca.RefinementName.Symmetrize,
                           sca.RefinementName.Diffuse, sca.RefinementName.RowWiseNormalize])
  utts = option_utterances(71)
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=7, refinement_options=opts)
  got = c.predict_batch(utts, group=8)
  assert_same_as_single_calls(c, utts, got, routes=[2] * len(utts))


def test_full_spectrum_request_is_eligible():
  """max_clusters=None with a Laplacian reads every eigenvalue: Jacobi returns them all anyway"""
  utts = [so.blobs(90, 16, 3, seed=90), so.blobs(41, 16, 2, seed=41)]
  c = icassp(laplacian_type=sca.LaplacianType.GraphCut, max_clusters=None)
  got = c.predict_batch(utts, group=16)
  assert_same_as_single_calls(c, utts, got, routes=expected_routes(c))
  assert all(d.eig_path == JACOBI for d in c.last_batch_diags)


def test_more_clusters_than_the_kmeans_chain_holds_leaves_the_route():
  utts = [so.blobs(100, 16, 3, seed=100), so.blobs(70, 16, 3, seed=70)]
  c = icassp(min_clusters=40)
  got = c.predict_batch(utts, group=16)
  assert c.last_batch_routes == [0, 0]
  for i, u in enumerate(utts):
    assert np.array_equal(got[i], c.predict(u))
    assert c.last_batch_diags[i].n_clusters == 40 == c.last_diag.n_clusters


def test_non_symmetric_front_leaves_the_route():
  opts = sca.RefinementOptions(
      p_percentile=0.92, refinement_sequence=[sca.RefinementName.RowWiseThreshold,
                                              sca.RefinementName.RowWiseNormalize])
  utts = [so.blobs(80, 16, 3, seed=80), so.blobs(33, 16, 2, seed=33)]
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=7, refinement_options=opts)
  got = c.predict_batch(utts, group=16)
  assert c.last_batch_routes == [0, 0]
  for u, lab in zip(utts, got):
    assert np.array_equal(lab, c.predict(u))


def test_non_finite_member_raises_like_predict():
  """a zero embedding row: NaN cosine, np.linalg.eig raises in the reference; the front sets the
  member's flag word, the batch fails with the single call's error"""
  utts = option_utterances(31, count=WIDTH + 5)
  bad = utts[2].copy()
  bad[7] = 0.0
  c = icassp()
  with pytest.raises(Exception) as single:
    c.predict(bad)
  with pytest.raises(type(single.value)):
    c.predict_batch(utts[:2] + [bad] + utts[3:], group=16)
  # the handle (and its member arenas) stay usable
  ok = c.predict_batch(utts, group=16)
  assert_same_as_single_calls(c, utts[:6], ok[:6], eig=False)
  assert c.last_batch_routes == [2] * len(utts)


def test_forms_that_are_not_routed():
  utts = option_utterances(41, count=5)
  c = icassp()
  for kw in ({"group": 1}, {"streams": 4}):
    got = c.predict_batch(utts, **kw)
    assert c.last_batch_routes == [0] * len(utts), kw
    for u, lab in zip(utts, got):
      assert np.array_equal(lab, c.predict(u))
  c = icassp(custom_dist="euclidean")
  got = c.predict_batch(utts, group=16)
  assert c.last_batch_routes == [0] * len(utts)
  for u, lab in zip(utts, got):
    assert np.array_equal(lab, c.predict(u))
  c = icassp(constraint_options=sca.ConstraintOptions(
      constraint_name=sca.ConstraintName.AffinityIntegration, apply_before_refinement=False,
      integration_type=sca.IntegrationType.Max))
  qs = [np.eye(u.shape[0]) for u in utts]
  got = c.predict_batch(utts, group=16, constraint_matrices=qs)
  assert c.last_batch_routes == [0] * len(utts)
  for u, q, lab in zip(utts, qs, got):
    assert np.array_equal(lab, c.predict(u, q))
