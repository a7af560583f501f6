"""GPU: predict_batch(..., autotune_from_entry_state=True) -- every utterance of an AutoTune batch
searched from the state the AutoTune object has when the call is entered.

Inputs: so.blobs(n, 32, 3, seed=1000 + n), n drawn from {3, 17, 33, 64, 96, 97, 112, 128, 200,
333} with repeats; on the CPU oracle every one of these sizes has its best proxy value at least
15 % below the runner-up under both searches, so no winner is a near tie.  The two searches:
Turn-to-Diarize (the preset: 0.40-0.95, step 0.05, one level; a speaker-turn ConstraintMatrix for
every second utterance) and ICASSP2018 + GraphCut (max_clusters=8, 0.55-0.95, step 0.05, two
levels).  The reference of every utterance is predict(u, c) on a deep copy of the clusterer.

The batch is ONE `sc_predict_batch_autotune` call: routes are 2 for n <= 128 and 1 above.
"""

import copy

import numpy as np
import pytest

import spectral_oracle as so
import spectralcluster_amd as sca
from spectralcluster_amd import _lib

pytestmark = pytest.mark.gpu

SIZES = (128, 3, 200, 17, 96, 333, 33, 97, 64, 112, 128, 96, 97, 17, 200, 3, 112, 64, 33, 333,
         128, 97, 96, 112)
SEARCHES = ("ttd", "icassp")
AUTOTUNE = {"ttd": (0.40, 0.95, 0.05, 1), "icassp": (0.55, 0.95, 0.05, 2)}


def embeddings(n):
  return so.blobs(n, 32, 3, seed=1000 + n)


def turn_scores(n):
  """Speaker-turn scores: a turn (score 1.5 .. 20) at about a fifth of the boundaries."""
  rng = np.random.default_rng(2000 + n)
  scores = np.where(rng.random(n) < 0.2, rng.uniform(1.5, 20.0, n), 0.0)
  scores[0] = 0.0
  return [float(s) for s in scores]


def clusterer_for(search):
  if search == "ttd":
    return copy.deepcopy(sca.configs.turntodiarize_clusterer)
  return sca.SpectralClusterer(
      min_clusters=2, max_clusters=8,
      refinement_options=copy.deepcopy(sca.configs.icassp2018_refinement_options),
      laplacian_type=sca.LaplacianType.GraphCut, autotune=sca.AutoTune(*AUTOTUNE["icassp"]))


def batch_for(search):
  us = [embeddings(n) for n in SIZES]
  if search == "ttd":
    cs = [sca.ConstraintMatrix(turn_scores(n), 1) if i % 2 == 0 else None
          for i, n in enumerate(SIZES)]
  else:
    cs = [None] * len(SIZES)
  return us, cs


def autotune_state(at):
  return (at.p_percentile_min, at.p_percentile_max, at.search_step, at.search_level, at.proxy)


_REFERENCE = {}


def reference(search):
  """Per utterance: predict(u, c) on a deep copy of the clusterer -> (labels, best_p,
  n_clusters, last value evaluated).  Computed once, never modified."""
  if search not in _REFERENCE:
    us, cs = batch_for(search)
    out = []
    for u, c in zip(us, cs):
      fresh = clusterer_for(search)
      labels = fresh.predict(u, c)
      labels.setflags(write=False)
      out.append((labels, fresh.last_best_p, len(np.unique(labels)),
                  fresh.refinement_options.p_percentile))
    _REFERENCE[search] = out
  return _REFERENCE[search]


@pytest.mark.parametrize("search", SEARCHES)
def test_batch_matches_a_fresh_clusterer_per_utterance(search):
  us, cs = batch_for(search)
  clusterer = clusterer_for(search)
  before = autotune_state(clusterer.autotune)
  entry = clusterer.autotune
  got = clusterer.predict_batch(us, constraint_matrices=cs, autotune_from_entry_state=True)
  want = reference(search)
  assert len(got) == len(us)
  assert clusterer.autotune is entry and autotune_state(entry) == before  # left as found
  assert clusterer.last_batch_best_p == [w[1] for w in want]
  assert clusterer.last_batch_routes == [
      _lib.BATCH_ROUTE_GROUP_JACOBI if n <= 128 else _lib.BATCH_ROUTE_GROUP_LANCZOS for n in SIZES]
  assert len(clusterer.last_batch_diags) == len(us)
  for n, diag, (_, _, ref_k, _) in zip(SIZES, clusterer.last_batch_diags, want):
    assert diag.n == n and diag.n_clusters == ref_k
  for n, labels, (ref_labels, _, ref_k, _) in zip(SIZES, got, want):
    assert labels.shape == (n,) and labels.dtype == np.int64
    assert len(np.unique(labels)) == ref_k
    assert so.adjusted_rand_index(labels, ref_labels) == 1.0
  # the last value evaluated for the last utterance (reference spectral_clusterer.py:277)
  assert clusterer.refinement_options.p_percentile == want[-1][3]
  # the same batch twice: identical results
  again = clusterer.predict_batch(us, constraint_matrices=cs, autotune_from_entry_state=True)
  assert clusterer.last_batch_best_p == [w[1] for w in want]
  assert clusterer.last_batch_routes == [
      _lib.BATCH_ROUTE_GROUP_JACOBI if n <= 128 else _lib.BATCH_ROUTE_GROUP_LANCZOS for n in SIZES]
  for a, b in zip(got, again):
    assert np.array_equal(a, b)


@pytest.mark.parametrize("search", SEARCHES)
def test_three_utterances_against_the_oracle(search):
  """The oracle's autotune_search + run_kmeans on unconstrained utterances: a short one on each
  side of m = 96 and one of the Lanczos sizes."""
  lo, hi, step, levels = AUTOTUNE[search]
  if search == "ttd":
    ocfg = so.turntodiarize_config()
  else:
    ocfg = so.icassp2018_config(max_clusters=8, laplacian_type=so.LAPLACIAN_GRAPH_CUT)
  sizes = (64, 112, 200)
  us = [embeddings(n) for n in sizes]
  clusterer = clusterer_for(search)
  got = clusterer.predict_batch(us, autotune_from_entry_state=True)
  assert clusterer.last_batch_routes == [2, 2, 1]
  for n, u, labels, best_p in zip(sizes, us, got, clusterer.last_batch_best_p):
    dump = {}
    want = so.predict(u, ocfg, dump, autotune=(lo, hi, step, levels, True))
    assert best_p == dump["best_p"], (n, best_p, dump["best_p"])
    assert so.adjusted_rand_index(labels, want) == 1.0, n


def test_flag_false_is_the_loop_of_today():
  """Without the flag utterance i + 1 is searched on the grid utterance i left narrowed."""
  us, cs = batch_for("icassp")
  us, cs = us[:6], cs[:6]
  clusterer = clusterer_for("icassp")
  got = clusterer.predict_batch(us, constraint_matrices=cs)
  assert clusterer.last_batch_routes == [_lib.BATCH_ROUTE_SINGLE] * len(us)
  loop = clusterer_for("icassp")
  want = [loop.predict(u) for u in us]
  for a, b in zip(got, want):
    assert np.array_equal(a, b)
  assert autotune_state(clusterer.autotune) == autotune_state(loop.autotune)
  assert autotune_state(clusterer.autotune) != autotune_state(clusterer_for("icassp").autotune)
  # a clusterer without AutoTune ignores the flag
  plain = sca.SpectralClusterer(
      min_clusters=2, max_clusters=7,
      refinement_options=sca.configs.icassp2018_refinement_options)
  a = plain.predict_batch(us, autotune_from_entry_state=True)
  routes = list(plain.last_batch_routes)
  b = plain.predict_batch(us)
  assert routes == plain.last_batch_routes and any(r != 0 for r in routes)
  for x, y in zip(a, b):
    assert np.array_equal(x, y)


def test_errors_are_raised_before_anything_runs():
  us, cs = batch_for("ttd")
  us, cs = us[:4], cs[:4]
  clusterer = clusterer_for("ttd")
  ran = []
  clusterer.predict = lambda u, c=None: ran.append(1)  # (any utterance that starts is recorded)
  clusterer._autotune_library_batch = lambda *a: ran.append(2)  # (... and the library call)
  bad = list(cs)
  bad[2] = sca.ConstraintMatrix(turn_scores(SIZES[2] + 1), 1)  # one value too many
  with pytest.raises(ValueError):
    clusterer.predict_batch(us, constraint_matrices=bad, autotune_from_entry_state=True)
  with pytest.raises(ValueError):
    clusterer.predict_batch(us, constraint_matrices=cs[:3], autotune_from_entry_state=True)
  clusterer.refinement_options.refinement_sequence = [sca.RefinementName.Symmetrize]
  with pytest.raises(ValueError, match="RowWiseThreshold"):
    clusterer.predict_batch(us, constraint_matrices=cs, autotune_from_entry_state=True)
  assert not ran


def test_a_dense_constraint_in_the_batch():
  """A dense ndarray among the entries: the same per-utterance form; that utterance is what
  predict(u, dense) on a fresh clusterer gives."""
  us, cs = batch_for("ttd")
  us, cs = us[:4], cs[:4]
  dense = list(cs)
  dense[0] = so.constraint_matrix_diagonals(turn_scores(SIZES[0]), 1)
  clusterer = clusterer_for("ttd")
  got = clusterer.predict_batch(us, constraint_matrices=dense, autotune_from_entry_state=True)
  assert clusterer.last_batch_routes == [_lib.BATCH_ROUTE_SINGLE] * 4
  fresh = clusterer_for("ttd")
  first = fresh.predict(us[0], dense[0])
  assert clusterer.last_batch_best_p[0] == fresh.last_best_p
  assert np.array_equal(got[0], first)
  want = reference("ttd")[:4]
  assert clusterer.last_batch_best_p[1:] == [w[1] for w in want[1:]]
  for labels, (ref_labels, _, _, _) in zip(got, want):  # (band or dense: the same partition)
    assert so.adjusted_rand_index(labels, ref_labels) == 1.0
