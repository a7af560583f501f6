"""GPU: the banded form of the speaker-turn constraint.  A `ConstraintMatrix` handed to the
library travels as its n - 1 band values (`sc_set_constraint_band`), ConstraintPropagation
forms T Q with one streaming pass (`k_cp_band_product`) and AffinityIntegration reads the
band; no (n, n) constraint buffer exists.

Reference of every check: the CPU oracle fed the DENSE matrix
`so.constraint_matrix_diagonals(scores, 1)` (or the reference's own goldens, which were
produced from exactly that matrix).  `CP_TOL` and `max_err` are the dense suite's
(test_gpu_constraints.py: condition number of I - alpha A_norm); AffinityIntegration is
elementwise, hence bit-exact.
"""

import copy
import ctypes
import dataclasses

import numpy as np
import pytest

import spectral_oracle as so
from conftest import golden
from test_gpu_constraints import CP_TOL, max_err, toy_refinement

import spectralcluster_amd as sca
from spectralcluster_amd import _lib, multigpu
from spectralcluster_amd import constraint as con

pytestmark = pytest.mark.gpu


def info(handle):
  kind, n = ctypes.c_int(-1), ctypes.c_int(-1)
  band_bytes, dense_bytes = ctypes.c_size_t(0), ctypes.c_size_t(0)
  handle.check(handle.lib.sc_constraint_info(
      handle.raw, ctypes.byref(kind), ctypes.byref(n), ctypes.byref(band_bytes),
      ctypes.byref(dense_bytes)))
  return kind.value, n.value, band_bytes.value, dense_bytes.value


# --- ConstraintPropagation, band in ------------------------------------------------------
@pytest.mark.parametrize("n,alpha", [(1, 0.6), (2, 0.6), (17, 0.4), (129, 0.6), (300, 0.4),
                                     (1000, 0.6), (2049, 0.4)])
def test_constraint_propagation_band_vs_oracle(n, alpha):
  x, _, scores = so.turn_blobs(n, 16, 3, seed=n) if n > 2 else (
      so.blobs(n, 4, 1, seed=n), None, np.zeros(n))
  a = so.affinity(x)
  q = so.constraint_matrix_diagonals(list(scores), 1)
  got = con.ConstraintPropagation(alpha).adjust_affinity(a, sca.ConstraintMatrix(list(scores), 1))
  err = max_err(got, so.constraint_propagation(a, q, alpha))
  print("n=%d alpha=%g band vs oracle: %.3e" % (n, alpha, err))
  assert err < CP_TOL
  # what the dense route gives for the same input (reported, not asserted)
  dense = con.ConstraintPropagation(alpha).adjust_affinity(a, q)
  print("n=%d band vs dense route: max |diff| %.3e, bit-equal %s" % (
      n, float(np.max(np.abs(got - dense))), np.array_equal(got, dense)))


def test_constraint_propagation_band_alpha_zero_and_unsupported_alpha():
  x = so.blobs(60, 8, 3, seed=5)
  a = so.affinity(x)
  scores = [0, 0, 5, 0, 0.5, 0] * 10
  q = so.constraint_matrix_diagonals(scores, 1)
  cm = sca.ConstraintMatrix(scores, 1)
  # alpha = 0: T = I, F = Q
  got = con.ConstraintPropagation(0.0).adjust_affinity(a, cm)
  assert max_err(got, so.constraint_propagation(a, q, 0.0)) < 1e-15
  with pytest.raises(sca.UnsupportedOnDeviceError):
    con.ConstraintPropagation(1.0).adjust_affinity(a, cm)


@pytest.mark.parametrize("alpha", [0.4, 0.6])
def test_constraint_propagation_band_general_affinity(alpha):
  """A non-symmetric affinity: the transposed route (T^T through launch_transpose, then the
  band product)."""
  a = golden("constraint_ops_n40.npz")["a_gen"]
  assert not np.array_equal(a, a.T)
  band = np.random.default_rng(40).integers(-1, 2, size=39).astype(np.float64)
  assert set(band) == {-1.0, 0.0, 1.0}
  # the turn scores that give this band: no turn (+1), a confident one (-1), a weak one (0)
  scores = [0.0] + [{1.0: 0.0, -1.0: 2.0, 0.0: 0.5}[b] for b in band]
  cm = sca.ConstraintMatrix(scores, 1)
  assert np.array_equal(cm.band(), band)
  q = so.constraint_matrix_diagonals(scores, 1)
  got = con.ConstraintPropagation(alpha).adjust_affinity(a, cm)
  err = max_err(got, so.constraint_propagation(a, q, alpha))
  print("general affinity, alpha=%g: %.3e" % (alpha, err))
  assert err < CP_TOL


# --- AffinityIntegration, band in ---------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 40, 300, 1000])
def test_affinity_integration_band_is_bit_exact(n):
  x, _, scores = so.turn_blobs(n, 16, 3, seed=n) if n > 2 else (
      so.blobs(n, 4, 1, seed=n), None, np.zeros(n))
  a = so.affinity(x)
  if n >= 40:
    a[5, 6] = np.nan    # on the band
    a[9, 11] = np.nan   # next to it
    a[30, 2] = np.nan   # far from it
  q = so.constraint_matrix_diagonals(list(scores), 1)
  cm = sca.ConstraintMatrix(list(scores), 1)
  got = con.AffinityIntegration(con.IntegrationType.Max).adjust_affinity(a, cm)
  assert np.array_equal(got, np.maximum(a, q), equal_nan=True)
  assert np.array_equal(np.isnan(got), np.isnan(a))
  got = con.AffinityIntegration(con.IntegrationType.Average).adjust_affinity(a, cm)
  assert np.array_equal(got, 0.5 * (a + q), equal_nan=True)
  assert np.array_equal(np.isnan(got), np.isnan(a))


# --- Turn-to-Diarize preset end to end -----------------------------------------------------
@pytest.mark.parametrize("n", [120, 300, 700])
def test_turntodiarize_band_vs_reference_golden(n):
  g = golden("turntodiarize_n%d.npz" % n)
  x, _, scores = so.turn_blobs(n, int(g["d"]), int(g["k"]), int(g["seed"]))
  band_clusterer = copy.deepcopy(sca.configs.turntodiarize_clusterer)
  labels = band_clusterer.predict(x, sca.ConstraintMatrix(list(scores), 1))
  assert so.adjusted_rand_index(labels, g["labels"]) == 1.0
  dense_clusterer = copy.deepcopy(sca.configs.turntodiarize_clusterer)
  dense_clusterer.predict(x, sca.ConstraintMatrix(list(scores), 1).compute_diagonals())
  assert band_clusterer.last_best_p == dense_clusterer.last_best_p


@pytest.mark.parametrize("n,noise", [(400, 1.0), (1200, 1.2)])
def test_turntodiarize_band_noisy_vs_oracle(n, noise):
  x, _, scores = so.turn_blobs(n, 24, 4, seed=n + 1, noise=noise)
  q = so.constraint_matrix_diagonals(list(scores), 1)
  want = so.predict(x, so.turntodiarize_config(), constraint_matrix=q,
                    autotune=so.TURNTODIARIZE_AUTOTUNE)
  band_clusterer = copy.deepcopy(sca.configs.turntodiarize_clusterer)
  got = band_clusterer.predict(x, sca.ConstraintMatrix(list(scores), 1))
  assert so.adjusted_rand_index(got, want) == 1.0
  dense_clusterer = copy.deepcopy(sca.configs.turntodiarize_clusterer)
  dense_clusterer.predict(x, q)
  assert band_clusterer.last_best_p == dense_clusterer.last_best_p


# --- randomised sweep over constraint configurations --------------------------------------
def _band_fuzz_cases():
  rng = np.random.default_rng(505)
  cases = []
  for i in range(20):
    n = int(rng.integers(30, 600))
    k = int(rng.integers(2, 5))
    name = int(rng.choice([so.CONSTRAINT_AFFINITY_INTEGRATION, so.CONSTRAINT_PROPAGATION]))
    before = bool(rng.integers(0, 2))
    kind = int(rng.choice([so.INTEGRATION_MAX, so.INTEGRATION_AVERAGE]))
    alpha = float(rng.choice([0.2, 0.4, 0.6, 0.8]))
    seq = str(rng.choice(["ttd", "icassp_nonorm"]))
    lap = int(rng.choice([0, 4]))
    cases.append((i, n, k, name, before, kind, alpha, seq, lap))
  return cases


@pytest.mark.parametrize("case", _band_fuzz_cases(), ids=lambda c: "bfuzz%d" % c[0])
def test_fuzz_band_constraints_vs_oracle(case):
  """No case returns early: every one of the 20 has an oracle max_delta >= 1.06 and is stable
  under 1e-9 relative perturbations of the embeddings (checked with the oracle alone)."""
  i, n, k, name, before, kind, alpha, seq, lap = case
  x, _, scores = so.turn_blobs(n, 24, k, seed=9000 + i, noise=0.8)
  q = so.constraint_matrix_diagonals(list(scores), 1)
  if seq == "ttd":
    ocfg = so.turntodiarize_config(p_percentile=0.9, laplacian_type=lap, row_wise_renorm=False)
    options = toy_refinement()
    options.p_percentile = 0.9
  else:
    ocfg = so.icassp2018_config(sequence=so.ICASSP2018_SEQUENCE[:-1], laplacian_type=lap)
    options = sca.RefinementOptions(gaussian_blur_sigma=1, p_percentile=0.95,
                                    refinement_sequence=sca.ICASSP2018_REFINEMENT_SEQUENCE[:-1])
  ocfg = dataclasses.replace(ocfg, min_clusters=2, max_clusters=7, constraint_name=name,
                             apply_before_refinement=before, integration_type=kind,
                             constraint_propagation_alpha=alpha)
  dump = {}
  want = so.predict(x, ocfg, dump, constraint_matrix=q)
  clusterer = sca.SpectralClusterer(
      min_clusters=2, max_clusters=7, refinement_options=options,
      laplacian_type=sca.LaplacianType(lap) if lap else None,
      constraint_options=sca.ConstraintOptions(
          constraint_name=sca.ConstraintName(name), apply_before_refinement=before,
          integration_type=sca.IntegrationType(kind), constraint_propagation_alpha=alpha))
  got = clusterer.predict(x, sca.ConstraintMatrix(list(scores), 1))
  diag = clusterer.last_diag
  print("case %d: n=%d oracle max_delta %.6g device %.6g" % (i, n, dump["max_delta"],
                                                            diag.max_delta))
  assert diag.n_clusters == dump["n_clusters"]
  np.testing.assert_allclose(diag.max_delta, dump["max_delta"], rtol=1e-5)
  assert so.adjusted_rand_index(got, want) == 1.0


# --- state of the handle -------------------------------------------------------------------
def test_band_only_handle_never_holds_a_dense_constraint(monkeypatch):
  n = 1200
  x, _, scores = so.turn_blobs(n, 24, 4, seed=n + 1, noise=1.2)
  device = _lib.default_handle().device
  fresh = _lib.Handle(device)
  monkeypatch.setitem(_lib._default_handles, device, fresh)
  try:
    assert info(fresh) == (0, 0, 0, 0)
    clusterer = copy.deepcopy(sca.configs.turntodiarize_clusterer)
    assert clusterer._handle() is fresh
    cm = sca.ConstraintMatrix(list(scores), 1)
    clusterer.predict(x, cm)
    kind, qn, band_bytes, dense_bytes = info(fresh)
    assert (kind, qn) == (2, n)
    assert 0 < band_bytes <= 8 * n
    assert dense_bytes == 0
    # band -> dense -> none -> band.  (Labels are compared elsewhere, on fresh copies of the
    # preset: AutoTune leaves its last p_percentile in the clusterer, like the reference, so
    # repeated calls of ONE clusterer do not search the same grid.)
    clusterer.predict(x, cm.compute_diagonals())
    kind, qn, _, dense_bytes = info(fresh)
    assert (kind, qn) == (1, n) and dense_bytes >= 8 * n * n
    clusterer.predict(x)
    assert info(fresh)[:2] == (0, 0)
    clusterer.predict(x, cm)
    assert info(fresh)[:2] == (2, n)
  finally:
    monkeypatch.undo()
    fresh.close()


def test_band_does_not_leak_into_the_next_call():
  x, _, scores = so.turn_blobs(150, 16, 3, seed=3, noise=1.0)
  clusterer = sca.SpectralClusterer(
      min_clusters=2, max_clusters=7, refinement_options=toy_refinement(),
      constraint_options=copy.deepcopy(sca.configs.turntodiarize_constraint_options),
      laplacian_type=sca.LaplacianType.GraphCut, row_wise_renorm=True)
  first = clusterer.predict(x)
  clusterer.predict(x, sca.ConstraintMatrix(list(scores), 1))
  assert info(clusterer._handle())[0] == 2
  again = clusterer.predict(x)
  np.testing.assert_array_equal(first, again)
  clusterer.predict(x, sca.ConstraintMatrix(list(scores), 1))
  batch = clusterer.predict_batch([x, x], streams=1)
  np.testing.assert_array_equal(batch[0], first)
  np.testing.assert_array_equal(batch[1], first)
  clusterer.predict(x, sca.ConstraintMatrix(list(scores), 1))
  batch = clusterer.predict_batch([x, x])  # (grouped: equal to the solver's tolerance)
  assert so.adjusted_rand_index(batch[0], first) == 1.0
  assert so.adjusted_rand_index(batch[1], first) == 1.0
  assert info(clusterer._handle())[0] == 0
  # without constraint_options a ConstraintMatrix is inert, like a dense matrix
  plain = sca.SpectralClusterer(
      min_clusters=2, max_clusters=7, refinement_options=toy_refinement(),
      laplacian_type=sca.LaplacianType.GraphCut, row_wise_renorm=True)
  np.testing.assert_array_equal(plain.predict(x, sca.ConstraintMatrix(list(scores), 1)), first)


# --- errors ----------------------------------------------------------------------------------
def test_band_errors():
  x = so.blobs(50, 8, 2, seed=1)
  clusterer = copy.deepcopy(sca.configs.turntodiarize_clusterer)
  with pytest.raises(ValueError, match="same shape"):
    clusterer.predict(x, sca.ConstraintMatrix([0.0] * 49, 1))
  with pytest.raises(ValueError, match="same shape"):
    clusterer._compute_eigenvectors_ncluster(so.affinity(x), sca.ConstraintMatrix([0.0] * 51, 1))
  with pytest.raises(ValueError, match="same shape"):
    con.ConstraintPropagation(0.4).adjust_affinity(so.affinity(x),
                                                   sca.ConstraintMatrix([0.0] * 49, 1))
  with pytest.raises(ValueError, match="same shape"):
    con.AffinityIntegration(con.IntegrationType.Max).adjust_affinity(
        so.affinity(x), sca.ConstraintMatrix([0.0] * 49, 1))
  with pytest.raises(RuntimeError):
    sca.SpectralClusterer(max_spectral_size=20).predict(x, sca.ConstraintMatrix([0.0] * 50, 1))
  bad_alpha = copy.deepcopy(sca.configs.turntodiarize_clusterer)
  bad_alpha.constraint_options.constraint_operator.alpha = 1.0
  with pytest.raises(sca.UnsupportedOnDeviceError):
    bad_alpha.predict(x, sca.ConstraintMatrix([0.0] * 50, 1))
  # the C entry points check their arguments
  handle = _lib.default_handle()
  assert handle.lib.sc_set_constraint_band(handle.raw, None, 0) != _lib.SC_OK
  assert handle.lib.sc_set_constraint_band(handle.raw, None, 5) != _lib.SC_OK
  handle.check(handle.lib.sc_set_constraint_band(handle.raw, None, 1))
  assert info(handle)[:2] == (2, 1)
  handle.check(handle.lib.sc_clear_constraint(handle.raw))


# --- the after-refinement branch, eigenvectors and all ----------------------------------------
def test_compute_eigenvectors_ncluster_band_equals_dense():
  x, _, scores = so.turn_blobs(200, 16, 3, 17)
  opts = toy_refinement()
  opts.p_percentile = 0.9
  clusterer = sca.SpectralClusterer(
      max_clusters=6, refinement_options=opts,
      constraint_options=sca.ConstraintOptions(
          constraint_name=sca.ConstraintName.AffinityIntegration,
          apply_before_refinement=False, integration_type=sca.IntegrationType.Max),
      laplacian_type=sca.LaplacianType.GraphCut, row_wise_renorm=True)
  a = so.affinity(x)
  cm = sca.ConstraintMatrix(list(scores), 1)
  _, k_band, delta_band = clusterer._compute_eigenvectors_ncluster(a, cm)
  assert clusterer.last_diag.symmetry_state == 1  # a band keeps the matrix symmetric
  _, k_dense, delta_dense = clusterer._compute_eigenvectors_ncluster(a, cm.compute_diagonals())
  assert k_band == k_dense
  np.testing.assert_allclose(delta_band, delta_dense, rtol=1e-9)


# --- batches and the distributed AutoTune -----------------------------------------------------
def test_predict_batch_with_constraint_matrices_equals_per_call_predict():
  inputs = [so.turn_blobs(n, 24, 3, seed=70 + n, noise=1.0) for n in (150, 260, 90, 400)]
  us = [x for x, _, _ in inputs]
  cs = [sca.ConstraintMatrix(list(inputs[0][2]), 1),
        so.constraint_matrix_diagonals(list(inputs[1][2]), 1),
        None,
        sca.ConstraintMatrix(list(inputs[3][2]), 1)]
  clusterer = sca.SpectralClusterer(
      min_clusters=2, max_clusters=7, refinement_options=toy_refinement(),
      constraint_options=copy.deepcopy(sca.configs.turntodiarize_constraint_options),
      laplacian_type=sca.LaplacianType.GraphCut, row_wise_renorm=True)
  want = [clusterer.predict(u, c) for u, c in zip(us, cs)]
  got = clusterer.predict_batch(us, constraint_matrices=cs)
  assert len(got) == len(want)
  for g, w in zip(got, want):
    np.testing.assert_array_equal(g, w)
  # the constraints did something: the unconstrained batch differs somewhere or equals -- either
  # way it must be what predict(u) gives
  free = clusterer.predict_batch(us, streams=1)
  for f, u in zip(free, us):
    np.testing.assert_array_equal(f, clusterer.predict(u))
  with pytest.raises(ValueError, match="as long as the batch"):
    clusterer.predict_batch(us, constraint_matrices=cs[:2])


def test_predict_autotune_distributed_takes_a_constraint_matrix():
  x, _, scores = so.turn_blobs(400, 24, 4, seed=401, noise=1.0)
  cm = sca.ConstraintMatrix(list(scores), 1)
  serial = copy.deepcopy(sca.configs.turntodiarize_clusterer)
  want = serial.predict(x, cm)
  sharded = copy.deepcopy(sca.configs.turntodiarize_clusterer)
  got = multigpu.predict_autotune_distributed(multigpu.LocalComm(), sharded, x,
                                              constraint_matrix=cm)
  np.testing.assert_array_equal(got, want)
  assert sharded.last_best_p == serial.last_best_p
  assert info(sharded._handle())[0] == 2
