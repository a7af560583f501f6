"""CPU: `PairwiseConstraints`, a constraint matrix given as must-link / cannot-link pairs.  The
class is host-side bookkeeping: `to_dense()` is the matrix it stands for, `entries()` what travels
to the device (`sc_set_constraint_pairs`).  The library exports the entry-list entry points next
to the dense and banded ones.  No compute call is made (there is no GPU here)."""

import ctypes
import os
import re

import numpy as np
import pytest

import spectral_oracle as so
import spectralcluster_amd as sca
from spectralcluster_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_SYMBOLS = ("sc_set_constraint_pairs", "sc_constraint_pairs_info",
                "sc_stage_constraint_pairs", "sc_stage_constraint_pairs_group",
                "sc_constraint_desc_layout", "sc_predict_batch_constraints")


def _example():
  return sca.PairwiseConstraints(
      7, must_link=[(0, 3), (5, 5)], cannot_link=[(6, 1)],
      pairs=[(2, 4), (3, 3), (4, 0)], values=[0.25, -2.0, 1e-3])


def test_to_dense_is_the_plain_loop():
  pc = _example()
  want = np.zeros((7, 7))
  for (i, j), v in (((0, 3), 1.0), ((5, 5), 1.0), ((6, 1), -1.0), ((2, 4), 0.25),
                    ((3, 3), -2.0), ((4, 0), 1e-3)):
    want[i, j] = v
    want[j, i] = v
  q = pc.to_dense()
  assert q.dtype == np.float64 and q.shape == (7, 7)
  assert np.array_equal(q, want)
  assert np.array_equal(q, q.T)
  empty = sca.PairwiseConstraints(4)
  assert np.array_equal(empty.to_dense(), np.zeros((4, 4)))
  assert sca.PairwiseConstraints(0).to_dense().shape == (0, 0)


def test_entries_order_twins_adjacent_and_one_entry_per_diagonal_pair():
  rows, cols, vals = _example().entries()
  assert rows.dtype == np.int32 and cols.dtype == np.int32 and vals.dtype == np.float64
  assert rows.flags.c_contiguous and cols.flags.c_contiguous and vals.flags.c_contiguous
  # must_link, cannot_link, pairs -- in the order given; (i, j) then (j, i); a diagonal pair once
  assert list(zip(rows, cols, vals)) == [
      (0, 3, 1.0), (3, 0, 1.0), (5, 5, 1.0), (6, 1, -1.0), (1, 6, -1.0), (2, 4, 0.25),
      (4, 2, 0.25), (3, 3, -2.0), (4, 0, 1e-3), (0, 4, 1e-3)]
  rows, cols, vals = sca.PairwiseConstraints(3).entries()
  assert rows.shape == cols.shape == vals.shape == (0,)
  assert rows.dtype == np.int32 and vals.dtype == np.float64
  # the entries are all there is to the matrix
  pc = _example()
  rebuilt = np.zeros((7, 7))
  rows, cols, vals = pc.entries()
  rebuilt[rows, cols] = vals
  assert np.array_equal(rebuilt, pc.to_dense())


def test_from_dense_round_trip_and_symmetry_check():
  q = _example().to_dense()
  back = sca.PairwiseConstraints.from_dense(q)
  assert back.n == 7
  assert np.array_equal(back.to_dense(), q)
  assert len(back.entries()[0]) == np.count_nonzero(q)
  assert np.array_equal(sca.PairwiseConstraints.from_dense(np.zeros((3, 3))).to_dense(),
                        np.zeros((3, 3)))
  bad = q.copy()
  bad[1, 2] = 0.5
  with pytest.raises(ValueError, match="symmetric"):
    sca.PairwiseConstraints.from_dense(bad)
  with pytest.raises(ValueError, match="square"):
    sca.PairwiseConstraints.from_dense(np.zeros((3, 4)))


def test_construction_errors():
  with pytest.raises(ValueError, match=r"outside \[0, n\)"):
    sca.PairwiseConstraints(5, must_link=[(0, 5)])
  with pytest.raises(ValueError, match=r"outside \[0, n\)"):
    sca.PairwiseConstraints(5, cannot_link=[(-1, 2)])
  with pytest.raises(ValueError, match=r"outside \[0, n\)"):
    sca.PairwiseConstraints(5, pairs=[(1, 7)], values=[1.0])
  for v in (np.nan, np.inf, -np.inf):
    with pytest.raises(ValueError, match="finite"):
      sca.PairwiseConstraints(5, pairs=[(1, 2)], values=[v])
  with pytest.raises(ValueError, match="together"):
    sca.PairwiseConstraints(5, pairs=[(1, 2)])
  with pytest.raises(ValueError, match="together"):
    sca.PairwiseConstraints(5, values=[1.0])
  with pytest.raises(ValueError, match="same length"):
    sca.PairwiseConstraints(5, pairs=[(1, 2), (2, 3)], values=[1.0])
  # an unordered pair listed twice, across all arguments and in either direction
  with pytest.raises(ValueError, match="twice"):
    sca.PairwiseConstraints(5, must_link=[(1, 2), (1, 2)])
  with pytest.raises(ValueError, match="twice"):
    sca.PairwiseConstraints(5, must_link=[(1, 2)], cannot_link=[(2, 1)])
  with pytest.raises(ValueError, match="twice"):
    sca.PairwiseConstraints(5, cannot_link=[(3, 3)], pairs=[(3, 3)], values=[0.5])
  # (1, 2) and (2, 1 + n) must not collide, nor (0, 4) with (1, 0): distinct pairs pass
  sca.PairwiseConstraints(5, must_link=[(0, 4), (1, 0), (4, 4), (0, 0)])


def test_it_is_not_a_sequence_and_converts_to_its_dense_matrix():
  pc = _example()
  assert not hasattr(pc, "__len__")
  assert np.array_equal(np.asarray(pc), pc.to_dense())
  assert np.asarray(pc).shape == (7, 7)
  assert np.asarray(pc, dtype=np.float32).dtype == np.float32


def test_check_input_reads_it_as_its_n_by_n_shape():
  for op in (sca.constraint.ConstraintPropagation(0.4),
             sca.constraint.AffinityIntegration(sca.IntegrationType.Max)):
    op.check_input(np.zeros((5, 5)), sca.PairwiseConstraints(5, must_link=[(0, 1)]))
    with pytest.raises(ValueError, match="affinity and constraint matrix must have the same shape"):
      op.check_input(np.zeros((5, 5)), sca.PairwiseConstraints(4, must_link=[(0, 1)]))
    with pytest.raises(ValueError, match="affinity must be a square matrix"):
      op.check_input(np.zeros((5, 4)), sca.PairwiseConstraints(5))
    with pytest.raises(ValueError, match="affinity must be 2-dimensional"):
      op.check_input(np.zeros(5), sca.PairwiseConstraints(5))


@pytest.mark.parametrize("n", [1, 2, 7, 300])
def test_a_band_written_as_pairs_is_compute_diagonals(n):
  kinds = [0.0, 0.5, 1.0, 1.5, 0.0, 20.0]
  scores = [kinds[i % len(kinds)] for i in range(n)]
  cm = sca.ConstraintMatrix(scores, 1)
  band = cm.band()
  at = np.flatnonzero(band)
  pc = sca.PairwiseConstraints(n, pairs=np.stack([at, at + 1], axis=1), values=band[at])
  assert np.array_equal(pc.to_dense(), cm.compute_diagonals())
  assert np.array_equal(pc.to_dense(), so.constraint_matrix_diagonals(scores, 1))


def test_library_exports_the_pair_entry_points():
  header = open(os.path.join(ROOT, "include", "spectralcluster_amd.h")).read()
  declared = set(re.findall(r"^(?:int|const char\*)\s+(sc_[a-z0-9_]+)\s*\(", header, flags=re.M))
  lib = _lib.load()
  for name in PAIR_SYMBOLS:
    assert name in declared, name
    assert name in _lib.PROTOTYPES, name
    assert hasattr(lib, name), name
  assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)
  # additions only: no struct or signature of the parent changes
  assert lib.sc_abi_version() == _lib.SC_ABI_VERSION == 11
  assert "PairwiseConstraints" in sca.__all__
  assert sca.PairwiseConstraints is sca.constraint.PairwiseConstraints


def test_constraint_desc_mirror_has_the_header_layout():
  lib = _lib.load()
  size = ctypes.c_int(0)
  offsets = (ctypes.c_int * 6)()
  assert lib.sc_constraint_desc_layout(ctypes.byref(size), offsets) == 0
  assert size.value == ctypes.sizeof(_lib.ScConstraintDesc)
  names = ("kind", "count", "band", "rows", "cols", "vals")
  assert [f[0] for f in _lib.ScConstraintDesc._fields_] == list(names)
  assert list(offsets) == [getattr(_lib.ScConstraintDesc, name).offset for name in names]
  assert lib.sc_constraint_desc_layout(None, None) == 0
  assert _lib.ScConstraintDesc().kind == 0  # a zeroed descriptor: no constraint


def test_predict_batch_checks_pair_constraints_before_anything_runs():
  clusterer = sca.SpectralClusterer()
  with pytest.raises(ValueError, match="as long as the batch"):
    clusterer.predict_batch([np.zeros((4, 2))],
                            constraint_matrices=[sca.PairwiseConstraints(4), None])


def test_entry_points_reject_a_null_handle():
  lib = _lib.load()
  assert lib.sc_predict_batch_constraints(None, None, None, 0, None, None, None,
                                          16) == _lib.SC_ERR_INVALID
  count, nbytes = ctypes.c_int(-1), ctypes.c_size_t(1)
  assert lib.sc_set_constraint_pairs(None, None, None, None, 0, 4) == _lib.SC_ERR_INVALID
  assert lib.sc_constraint_pairs_info(None, ctypes.byref(count),
                                      ctypes.byref(nbytes)) == _lib.SC_ERR_INVALID
  assert lib.sc_stage_constraint_pairs(None, None, None, None, None, None, 0, 4,
                                       None) == _lib.SC_ERR_INVALID
  assert lib.sc_stage_constraint_pairs_group(None, None, 1, None, None, None, None, None, None,
                                             None) == _lib.SC_ERR_INVALID
