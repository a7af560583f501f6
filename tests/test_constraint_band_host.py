"""CPU: the banded form of the speaker-turn constraint (reference constraint.py:167-207).
`ConstraintMatrix.band()` holds exactly what `compute_diagonals()` puts on the first
off-diagonals, and the library exports the band entry points next to the dense ones.  No
compute call is made (there is no GPU here)."""

import os
import re

import numpy as np
import pytest

import spectral_oracle as so
import spectralcluster_amd as sca
from spectralcluster_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND_SYMBOLS = ("sc_set_constraint_band", "sc_stage_constraint_band", "sc_constraint_info")


def _scores(n, thr, seed):
  """Turn scores with 0, values below, equal to and above `thr` (cycled, then shuffled)."""
  kinds = [0.0, 0.5 * thr, thr, 1.5 * thr, 0.0, 20.0 * thr, np.nextafter(thr, np.inf)]
  s = np.array([kinds[i % len(kinds)] for i in range(n)])
  np.random.default_rng(seed).shuffle(s)
  return s


@pytest.mark.parametrize("thr", [1, 0.25, 3.5])
@pytest.mark.parametrize("n", [0, 1, 2, 7, 1000])
def test_band_is_the_first_off_diagonal_of_compute_diagonals(n, thr):
  s = _scores(n, thr, seed=n)
  if n == 1000:
    present = set(np.sign(s[1:] - thr)) | ({"zero"} if (s[1:] == 0).any() else set())
    assert present == {-1.0, 0.0, 1.0, "zero"}  # below, equal, above, and no turn at all
  want = so.constraint_matrix_diagonals(list(s), thr)
  cm = sca.ConstraintMatrix(list(s), thr)
  band = cm.band()
  assert band.dtype == np.float64 and band.shape == (max(n - 1, 0),)
  assert np.array_equal(band, np.diagonal(want, 1))
  assert np.array_equal(band, np.diagonal(want, -1))
  q = cm.compute_diagonals()
  assert q.dtype == np.float64 and q.shape == (n, n)
  assert np.array_equal(q, want)
  # the band is all there is to the matrix
  rebuilt = np.zeros((n, n))
  idx = np.arange(max(n - 1, 0))
  rebuilt[idx, idx + 1] = band
  rebuilt[idx + 1, idx] = band
  assert np.array_equal(rebuilt, want)


def test_band_takes_arrays_and_lists_alike():
  s = _scores(50, 1, seed=50)
  assert np.array_equal(sca.ConstraintMatrix(s, 1).band(), sca.ConstraintMatrix(list(s), 1).band())


def test_negative_scores_still_raise():
  with pytest.raises(ValueError, match="larger or equal to 0"):
    sca.ConstraintMatrix([0, 1, -0.5, 2], 1)
  with pytest.raises(ValueError):
    so.constraint_matrix_diagonals([0, 1, -0.5, 2], 1)


def test_library_exports_the_band_entry_points():
  header = open(os.path.join(ROOT, "include", "spectralcluster_amd.h")).read()
  declared = set(re.findall(r"^(?:int|const char\*)\s+(sc_[a-z0-9_]+)\s*\(", header, flags=re.M))
  lib = _lib.load()
  for name in BAND_SYMBOLS:
    assert name in declared, name
    assert name in _lib.PROTOTYPES, name
    assert hasattr(lib, name), name
  assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)
  # additions only: the structs are the parent's (ABI 9: the test entry of the refinement front)
  assert lib.sc_abi_version() == _lib.SC_ABI_VERSION == 11


def test_check_input_reads_a_constraint_matrix_as_its_n_by_n_shape():
  op = sca.constraint.ConstraintPropagation(0.4)
  op.check_input(np.zeros((5, 5)), sca.ConstraintMatrix([0] * 5, 1))
  with pytest.raises(ValueError, match="same shape"):
    op.check_input(np.zeros((5, 5)), sca.ConstraintMatrix([0] * 4, 1))
  with pytest.raises(ValueError, match="square"):
    op.check_input(np.zeros((5, 4)), sca.ConstraintMatrix([0] * 5, 1))


def test_predict_batch_checks_the_length_of_constraint_matrices():
  clusterer = sca.SpectralClusterer()
  with pytest.raises(ValueError, match="as long as the batch"):
    clusterer.predict_batch([np.zeros((4, 2))], constraint_matrices=[None, None])
