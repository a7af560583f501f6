"""CPU: the reference of the linkage kernel tests (tests/_linkage_ref.py) pinned before a GPU is
involved -- against scipy's linkage (heights included, exactly) and sklearn's labels -- and what
its inputs exercise, asserted: tied scans, ties the previous chain element wins, chains as long as
the problem, and that each tie rule of the loop changes the merge list when it is flipped."""

import os
import re

import numpy as np
import pytest
from scipy.cluster.hierarchy import linkage
from scipy.spatial.distance import pdist, squareform
from sklearn.cluster import AgglomerativeClustering

import _linkage_ref as lr
from spectralcluster_amd import _lib

SMALL = (2, 3, 4, 17, 63, 64, 65, 127, 128)
CHAIN_ONLY = (129, 257, 1023, 1024, 1025, 2049)
TIE_SIZES = (17, 63, 64, 65, 127, 128, 129, 257)  # where the tie coverage is asserted
METHODS = (lr.COMPLETE, lr.AVERAGE)


def test_stage_entries_are_declared_prototyped_and_exported():
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  header = open(os.path.join(root, "include", "spectralcluster_amd.h")).read()
  declared = set(re.findall(r"^int\s+(sc_[a-z0-9_]+)\s*\(", header, flags=re.M))
  lib = _lib.load()
  for name in ("sc_stage_linkage", "sc_stage_cosine_distances"):
    assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
  for form, name in enumerate(("SINGLE", "BATCH", "BATCH_LDS", "POOL", "POOL_LDS", "CHAIN_VERDICT",
                               "LDS_VERDICT")):
    assert re.search(r"#define\s+SC_LINKAGE_FORM_%s\s+%d\b" % (name, form), header), name
  # NULL handle: an error code, no crash
  assert lib.sc_stage_linkage(None, 0, 2, 0, None, None, 0, 0.0, None, None, None, None, 0,
                              0.0) == _lib.SC_ERR_INVALID
  assert lib.sc_stage_cosine_distances(None, 0, None, 0, 0, None) == _lib.SC_ERR_INVALID


def plain_distances(kind, n):
  d = lr.distances(lr.cosines(kind, n)).copy()
  np.fill_diagonal(d, 0.0)
  return d


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", sorted(lr.BUILDERS))
@pytest.mark.parametrize("n", SMALL + CHAIN_ONLY)
def test_port_is_scipy_linkage(n, kind, method):
  z, _ = lr.reference(kind, n, method)
  want = linkage(squareform(plain_distances(kind, n), checks=False), lr.METHOD_NAMES[method])
  got = lr.label(z, n)
  assert got.tobytes() == want.tobytes()
  assert np.all(z[:, 0] < z[:, 1])


def test_inputs_are_what_they_claim():
  for n in SMALL + CHAIN_ONLY:
    for kind in lr.EXACT_KINDS + ("cont",):
      c = lr.cosines(kind, n)
      assert np.array_equal(c, c.T), (kind, n)
      off = c[~np.eye(n, dtype=bool)]
      if kind != "clip":  # the padding's cosine 1 is below every distance of the matrix
        assert off.max() < 1.0 and off.min() >= -1.0, (kind, n)
    for kind in ("q1", "q3", "q8", "chain"):  # c = 1 - d without rounding
      c = lr.cosines(kind, n)
      assert np.array_equal(1.0 - (1.0 - c), c)
    c = lr.cosines("clip", n)
    if n >= 17:
      assert (c > 1.0).any() and (c < -1.0).any()
      d = lr.distances(c)
      assert d.min() == 0.0 and d.max() == 2.0
    assert lr.reference("cont", n, lr.AVERAGE)[1]["ties"] == 0


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("levels", (3, 8))
@pytest.mark.parametrize("n", TIE_SIZES)
def test_quantised_inputs_exercise_the_tie_rules(n, levels, method):
  kind = "q%d" % levels
  z, stats = lr.reference(kind, n, method)
  assert stats["ties"] >= 10 and stats["prev_ties"] >= 1, stats
  d = lr.distances(lr.cosines(kind, n))
  for mutant in ({"tie": "last"}, {"prefer_prev": False}, {"start": "last"}):
    zm, _ = lr.nn_chain(d, method, **mutant)
    assert zm.tobytes() != z.tobytes(), mutant


@pytest.mark.parametrize("n", (17, 65, 128))
def test_everything_ties_input(n):
  for method in METHODS:
    z, stats = lr.reference("q1", n, method)
    assert stats["ties"] >= n - 2 and stats["prev_ties"] == 0
    assert np.all(z[:, 2] == 0.125)


@pytest.mark.parametrize("n", SMALL + CHAIN_ONLY)
def test_long_chain_reaches_n(n):
  for method in METHODS:
    assert lr.reference("chain", n, method)[1]["max_chain"] == n
  assert lr.distances(lr.cosines("chain", n)).max() < 1.0


def sklearn_labels(d, method, **how):
  model = AgglomerativeClustering(metric="precomputed", linkage=lr.METHOD_NAMES[method], **how)
  return model.fit_predict(d)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind,n", [("q3", 17), ("q8", 65), ("q3", 128), ("q8", 257),
                                    ("clip", 64), ("chain", 129), ("cont", 127)])
def test_cut_is_sklearn(kind, n, method):
  z, _ = lr.reference(kind, n, method)
  d = plain_distances(kind, n)
  for k in (1, 2, 7, n):
    want = sklearn_labels(d, method, n_clusters=k)
    assert np.array_equal(lr.cut(z, n, n_clusters=k), want), k
  heights = np.unique(z[:, 2])
  for t in (heights[0], heights[len(heights) // 2], heights[-1], heights[-1] + 1.0):
    want = sklearn_labels(d, method, n_clusters=None, distance_threshold=float(t))
    assert np.array_equal(lr.cut(z, n, distance_threshold=float(t)), want), t


def test_verdict_record():
  z = np.array([[0, 1, 0.25, 2], [2, 3, 0.5, 2], [1, 3, 0.375, 4]])
  assert lr.verdict_record(z, 0.375).tolist() == [0.5, 0.0]
  assert lr.verdict_record(z, 0.25).tolist() == [0.25, 0.0]
  assert lr.verdict_record(z, np.nextafter(0.5, 1.0)).tolist() == [0.5, 1.0]


@pytest.mark.parametrize("n,d", [(65, 24), (300, 24)])
def test_duplicates_inputs(n, d):
  x, pairs = lr.duplicates(n, d)
  assert n // 5 <= len(pairs) <= n // 2
  for copy, original in pairs:
    assert np.array_equal(x[copy], x[original]) and copy != original
    assert n <= 128 or copy // 128 != original // 128
  dist = squareform(pdist(x, "cosine"))  # scipy: equal rows, equal distances
  for copy, original in pairs:
    assert np.array_equal(np.delete(dist[:, copy], [copy, original]),
                          np.delete(dist[:, original], [copy, original]))
