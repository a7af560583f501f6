"""GPU: a grouped batch that carries one speaker-turn band per utterance
(`sc_predict_batch_constrained`, through `predict_batch(us, constraint_matrices=cs)`), and the
grouped ConstraintPropagation chain on its own (`sc_stage_constraint_band_group`).

Reference of every check: the CPU oracle fed the DENSE matrix
`so.constraint_matrix_diagonals(scores, 1)`.  `CP_TOL` and `max_err` are the single route's
(test_gpu_constraints.py).  The inputs of the end-to-end tests were checked with the oracle
alone: every cluster count is 2 or 3, every decision is stable under 1e-9 relative perturbations
of the embeddings, and the constrained `max_delta` differs from the unconstrained one by at least
7e-4 relative, so a batch that dropped its constraints would miss the 1e-5 assertion.
"""

import copy
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

import spectral_oracle as so
from test_gpu_constraints import CP_TOL, max_err, toy_refinement

import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import constraint as con

pytestmark = pytest.mark.gpu

SIZES = (20, 64, 127, 128, 129, 150, 257, 400, 513, 700, 1000)
ROUTES = [2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1]
# (name, before refinement, alpha, integration type)
CP_BEFORE = (so.CONSTRAINT_PROPAGATION, True, 0.4, None)
CP_AFTER = (so.CONSTRAINT_PROPAGATION, False, 0.6, None)
AI_AFTER = (so.CONSTRAINT_AFFINITY_INTEGRATION, False, 0.6, so.INTEGRATION_MAX)


def make_clusterer(variant):
  name, before, alpha, kind = variant
  options = toy_refinement()
  options.p_percentile = 0.9
  return sca.SpectralClusterer(
      min_clusters=2, max_clusters=7, refinement_options=options,
      laplacian_type=sca.LaplacianType.GraphCut, row_wise_renorm=True,
      constraint_options=sca.ConstraintOptions(
          constraint_name=sca.ConstraintName(name), apply_before_refinement=before,
          integration_type=None if kind is None else sca.IntegrationType(kind),
          constraint_propagation_alpha=alpha))


@functools.lru_cache(maxsize=None)
def utterance(n, seed, noise):
  x, _, scores = so.turn_blobs(n, 24, 3, seed=seed, noise=noise)
  x.setflags(write=False)
  return x, tuple(float(s) for s in scores)


@functools.lru_cache(maxsize=None)
def oracle(n, seed, noise, variant, constrained=True):
  """(labels, n_clusters, max_delta) of the CPU oracle; computed once per input and shared."""
  name, before, alpha, kind = variant
  x, scores = utterance(n, seed, noise)
  cfg = so.turntodiarize_config(p_percentile=0.9, laplacian_type=so.LAPLACIAN_GRAPH_CUT,
                                row_wise_renorm=True)
  cfg = dataclasses.replace(
      cfg, min_clusters=2, max_clusters=7,
      constraint_name=name if constrained else so.CONSTRAINT_NONE, apply_before_refinement=before,
      constraint_propagation_alpha=alpha,
      integration_type=so.INTEGRATION_MAX if kind is None else kind)
  dump = {}
  q = so.constraint_matrix_diagonals(list(scores), 1) if constrained else None
  labels = so.predict(np.array(x), cfg, dump, constraint_matrix=q)
  labels.setflags(write=False)
  return labels, int(dump["n_clusters"]), float(dump["max_delta"])


def batch_inputs(cases):
  """cases: (n, seed, noise) -> embeddings and ConstraintMatrix lists."""
  us = [np.array(utterance(*c)[0]) for c in cases]
  cs = [sca.ConstraintMatrix(list(utterance(*c)[1]), 1) for c in cases]
  return us, cs


def check_against_oracle(clusterer, got, cases, variant):
  for i, c in enumerate(cases):
    want, k, delta = oracle(*c, variant)
    diag = clusterer.last_batch_diags[i]
    print("n=%d seed=%d: oracle k %d max_delta %.9g, device k %d max_delta %.9g" % (
        c[0], c[1], k, delta, diag.n_clusters, diag.max_delta))
    assert diag.n_clusters == k
    np.testing.assert_allclose(diag.max_delta, delta, rtol=1e-5)
    assert so.adjusted_rand_index(got[i], want) == 1.0


CLEAN = tuple((n, 500 + n, 0.8) for n in SIZES)


def info_kind(handle):
  kind = ctypes.c_int(-1)
  handle.check(handle.lib.sc_constraint_info(handle.raw, ctypes.byref(kind), None, None, None))
  return kind.value


# --- 1. the grouped chain against the oracle -----------------------------------------------
def chain_input(n):
  if n > 2:
    x, _, scores = so.turn_blobs(n, 16, 3, seed=n)
  else:
    x, scores = so.blobs(n, 4, 1, seed=n), np.zeros(n)
  return so.affinity(x), [float(s) for s in scores]


def run_chain(ns, alpha, idle=()):
  """sc_stage_constraint_band_group on the inputs of `chain_input`; members listed in `idle`
  get a NULL band.  Returns (outs, affinities, score lists); idle outs keep their fill."""
  count = len(ns)
  cfg = _lib.ScConfig()
  _lib.load().sc_config_default(cfg)
  cfg.constraint_name = sca.ConstraintName.ConstraintPropagation.value
  cfg.constraint_before_refinement = 1
  cfg.constraint_alpha = float(alpha)
  affs, scores, bands, outs = [], [], [], []
  for n in ns:
    a, sc = chain_input(n) if n > 0 else (np.zeros((0, 0)), [])
    affs.append(np.ascontiguousarray(a))
    scores.append(sc)
    bands.append(np.ascontiguousarray(np.concatenate(
        [sca.ConstraintMatrix(sc, 1).band(), [0.0]]) if n > 0 else np.zeros(1)))
    outs.append(np.full((n, n), -7.0))
  dp = ctypes.POINTER(ctypes.c_double)
  ap = (dp * count)(*[_lib.as_double_p(a) if a.size else None for a in affs])
  bp = (dp * count)(*[None if (z in idle or ns[z] == 0) else _lib.as_double_p(bands[z])
                      for z in range(count)])
  op = (dp * count)(*[_lib.as_double_p(o) if o.size else None for o in outs])
  handle = _lib.default_handle()
  handle.check(handle.lib.sc_stage_constraint_band_group(
      handle.raw, cfg, count, (ctypes.c_int32 * count)(*ns), ap, bp, op))
  return outs, affs, scores


CHAIN_GROUPS = {
    "one": [1],
    "tiny": [2, 17],
    "tile-edge": [127, 128, 129],
    "mixed": [129, 1, 300, 0, 128, 257, 2, 255],
    "sixteen": list(range(130, 146)),
    "five-tiles": [513],
}


@pytest.mark.parametrize("alpha", [0.4, 0.6])
@pytest.mark.parametrize("group", sorted(CHAIN_GROUPS))
def test_grouped_chain_vs_oracle(group, alpha):
  ns = CHAIN_GROUPS[group]
  outs, affs, scores = run_chain(ns, alpha)
  for z, n in enumerate(ns):
    if n == 0:
      continue
    q = so.constraint_matrix_diagonals(scores[z], 1)
    assert not np.isnan(outs[z]).any()  # (the padding was NaN: nothing outside a matrix was read)
    err = max_err(outs[z], so.constraint_propagation(affs[z], q, alpha))
    single = con.ConstraintPropagation(alpha).adjust_affinity(
        affs[z], sca.ConstraintMatrix(scores[z], 1))
    print("n=%d alpha=%g grouped vs oracle %.3e; vs the single route: max |diff| %.3e" % (
        n, alpha, err, float(np.max(np.abs(outs[z] - single)))))
    assert err < CP_TOL


def test_grouped_chain_idle_members_alpha_zero_and_unsupported_alpha():
  ns = [40, 33, 0, 150]
  outs, affs, scores = run_chain(ns, 0.4, idle=(1,))
  assert np.all(outs[1] == -7.0)  # NULL band with n > 1: idle, its output untouched
  for z in (0, 3):
    q = so.constraint_matrix_diagonals(scores[z], 1)
    assert max_err(outs[z], so.constraint_propagation(affs[z], q, 0.4)) < CP_TOL
  # alpha = 0: T = I, F = Q
  outs, affs, scores = run_chain([60, 129], 0.0)
  for z in range(2):
    q = so.constraint_matrix_diagonals(scores[z], 1)
    assert max_err(outs[z], so.constraint_propagation(affs[z], q, 0.0)) < 1e-15
  with pytest.raises(sca.UnsupportedOnDeviceError):
    run_chain([60], 1.0)


# --- 2. batch end to end -------------------------------------------------------------------
@pytest.mark.parametrize("variant", [CP_BEFORE, CP_AFTER], ids=["before-0.4", "after-0.6"])
def test_constrained_batch_vs_oracle(variant):
  us, cs = batch_inputs(CLEAN)
  clusterer = make_clusterer(variant)
  got = clusterer.predict_batch(us, constraint_matrices=cs)
  assert clusterer.last_batch_routes == ROUTES
  check_against_oracle(clusterer, got, CLEAN, variant)


# --- 3. labels that depend on the constraints ------------------------------------------------
NOISY = tuple((n, seed, 1.4) for n, seed in (
    (100, 1800), (100, 1803), (200, 2800), (200, 2801), (200, 2802), (300, 3801), (300, 3802),
    (300, 3803), (500, 5800), (500, 5801)))


def test_constrained_batch_labels_depend_on_the_constraints():
  """The unconstrained oracle labels every one of these ten differently (ARI 0.943 .. 0.992
  against the constrained ones)."""
  us, cs = batch_inputs(NOISY)
  clusterer = make_clusterer(CP_BEFORE)
  got = clusterer.predict_batch(us, constraint_matrices=cs)
  assert clusterer.last_batch_routes == [2, 2, 1, 1, 1, 1, 1, 1, 1, 1]
  for i, c in enumerate(NOISY):
    want, _, _ = oracle(*c, CP_BEFORE)
    assert so.adjusted_rand_index(got[i], want) == 1.0


# --- 4. AffinityIntegration -------------------------------------------------------------------
def test_constrained_batch_affinity_integration_equals_predict():
  us, cs = batch_inputs(CLEAN)
  clusterer = make_clusterer(AI_AFTER)
  got = clusterer.predict_batch(us, constraint_matrices=cs)
  assert clusterer.last_batch_routes == ROUTES
  fresh = make_clusterer(AI_AFTER)
  for i, (u, c) in enumerate(zip(us, cs)):
    want = fresh.predict(u, c)
    assert clusterer.last_batch_diags[i].n_clusters == fresh.last_diag.n_clusters
    assert so.adjusted_rand_index(got[i], want) == 1.0


# --- 5. mixed and unrouted forms ------------------------------------------------------------
def test_members_without_a_constraint_and_forms_that_stay_the_loop():
  us, cs = batch_inputs(CLEAN)
  clusterer = make_clusterer(CP_BEFORE)
  plain = clusterer.predict_batch(us)
  mixed = list(cs)
  for i in (1, 4, 7, 10):
    mixed[i] = None
  got = clusterer.predict_batch(us, constraint_matrices=mixed)
  assert clusterer.last_batch_routes == ROUTES
  for i, c in enumerate(CLEAN):
    if mixed[i] is None:
      np.testing.assert_array_equal(got[i], plain[i])
    else:
      assert so.adjusted_rand_index(got[i], oracle(*c, CP_BEFORE)[0]) == 1.0
  # one dense matrix: the per-call loop, exactly predict(u, c)
  few = [0, 4, 6]
  dense = [cs[i] for i in few]
  dense[1] = cs[4].compute_diagonals()
  got = clusterer.predict_batch([us[i] for i in few], constraint_matrices=dense)
  assert clusterer.last_batch_routes == [0, 0, 0]
  for g, i, c in zip(got, few, dense):
    np.testing.assert_array_equal(g, clusterer.predict(us[i], c))
  # the Turn-to-Diarize preset tunes p_percentile per utterance: the loop
  preset = copy.deepcopy(sca.configs.turntodiarize_clusterer)
  preset.predict_batch([us[i] for i in few], constraint_matrices=[cs[i] for i in few])
  assert preset.last_batch_routes == [0, 0, 0]


# --- 6. more members than a launch holds ----------------------------------------------------
SHORT_WAVE = tuple((n, 500 + n, 0.8) for n in [40 + (88 * i) // 19 for i in range(20)])
TWO_GROUPS = tuple((n, 500 + n, 0.8) for n in range(130, 310, 10))


@pytest.mark.parametrize("cases,route", [(SHORT_WAVE, 2), (TWO_GROUPS, 1)],
                         ids=["20-short", "18-lanczos"])
def test_more_members_than_a_launch_holds(cases, route):
  us, cs = batch_inputs(cases)
  clusterer = make_clusterer(CP_BEFORE)
  got = clusterer.predict_batch(us, constraint_matrices=cs, group=16)
  assert clusterer.last_batch_routes == [route] * len(cases)
  for i, c in enumerate(cases):
    assert so.adjusted_rand_index(got[i], oracle(*c, CP_BEFORE)[0]) == 1.0


# --- 7. state ---------------------------------------------------------------------------------
def test_no_constraint_outlives_a_constrained_batch():
  us, cs = batch_inputs(CLEAN)
  clusterer = make_clusterer(CP_BEFORE)
  before = clusterer.predict_batch(us)
  first = clusterer.predict_batch(us, constraint_matrices=cs)
  assert info_kind(clusterer._handle()) == 0
  after = clusterer.predict_batch(us)
  for b, a in zip(before, after):
    np.testing.assert_array_equal(b, a)
  second = clusterer.predict_batch(us, constraint_matrices=cs)
  for f, s in zip(first, second):
    np.testing.assert_array_equal(f, s)


# --- 8. errors --------------------------------------------------------------------------------
def test_constrained_batch_errors_leave_the_clusterer_usable():
  us, cs = batch_inputs(CLEAN)
  clusterer = make_clusterer(CP_BEFORE)
  wrong = list(cs)
  wrong[3] = sca.ConstraintMatrix([0.0] * (SIZES[3] - 1), 1)
  with pytest.raises(ValueError, match="same shape"):
    clusterer.predict_batch(us, constraint_matrices=wrong)
  with pytest.raises(ValueError, match="as long as the batch"):
    clusterer.predict_batch(us, constraint_matrices=cs[:2])
  got = clusterer.predict_batch(us, constraint_matrices=cs)
  assert clusterer.last_batch_routes == ROUTES
  check_against_oracle(clusterer, got, CLEAN, CP_BEFORE)


# --- 9. members that run as single calls keep their band ---------------------------------------
def test_members_on_the_single_call_path_carry_their_band():
  """The C entry with a k-means metric the grouped routes do not take (Python keeps such a batch
  in its loop): every member is a single call inside the batch, each with its own band resident
  -- the path banded members also take when the chain's work matrices do not fit."""
  few = (CLEAN[1], CLEAN[5], CLEAN[6])
  us, cs = batch_inputs(few)
  clusterer = make_clusterer(CP_BEFORE)
  clusterer.custom_dist = "euclidean"
  want = [clusterer.predict(u, c) for u, c in zip(us, cs)]
  count = len(us)
  handle = clusterer._handle()
  arrays = (_lib.ScArray * count)()
  for i, u in enumerate(us):
    arrays[i].data = u.ctypes.data
    arrays[i].rows, arrays[i].cols = u.shape
    arrays[i].row_stride, arrays[i].col_stride = u.shape[1], 1
    arrays[i].dtype, arrays[i].location = _lib.SC_DTYPE_F64, _lib.SC_MEM_HOST
  bands = [np.ascontiguousarray(c.band()) for c in cs]
  dp = ctypes.POINTER(ctypes.c_double)
  bp = (dp * count)(*[_lib.as_double_p(b) for b in bands])
  labels = [np.empty(u.shape[0], dtype=np.int64) for u in us]
  lp = (ctypes.POINTER(ctypes.c_int64) * count)(*[_lib.as_int64_p(l) for l in labels])
  handle.check(handle.lib.sc_predict_batch_constrained(
      handle.raw, arrays, bp, count, clusterer.build_config(), lp, None, 16))
  routes = (ctypes.c_int32 * count)()
  handle.check(handle.lib.sc_last_batch_routes(handle.raw, routes, count))
  assert list(routes) == [0, 0, 0]
  for g, w in zip(labels, want):
    np.testing.assert_array_equal(g, w)
  assert info_kind(handle) == 0
  assert handle.lib.sc_predict_batch_constrained(
      handle.raw, arrays, bp, count, clusterer.build_config(), lp, None, 1) == _lib.SC_ERR_INVALID
