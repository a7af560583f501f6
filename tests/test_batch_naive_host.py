"""CPU: the Naive fallback inside the batch calls (sc_batch_naive_cluster, sc_batch_naive_check,
sc_predict_batch_reduced_naive, sc_predict_batch_single_naive) is exported and prototyped, and
SpectralClusterer.predict_batch routes to the two _naive calls exactly when
`batch_naive_fallback` asks for it -- driven with a stand-in handle, no device.  The NumPy
reference of the GPU tests (tests/_naive_ref.py) is checked here against real reference output."""

import os
import re

import numpy as np
import pytest
import spectral_oracle as so
from conftest import golden

import _batch_fake
import _naive_ref
import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import fallback_clusterer as fb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sc_batch_naive_cluster", "sc_batch_naive_check", "sc_predict_batch_reduced_naive",
               "sc_predict_batch_single_naive")


def test_new_symbols_are_declared_prototyped_and_exported():
  header = open(os.path.join(ROOT, "include", "spectralcluster_amd.h")).read()
  declared = set(re.findall(r"^int\s+(sc_[a-z0-9_]+)\s*\(", header, flags=re.M))
  lib = _lib.load()
  for name in NEW_SYMBOLS:
    assert name in declared, name
    assert name in _lib.PROTOTYPES, name
    assert hasattr(lib, name), name
  assert lib.sc_abi_version() == 11 and _lib.SC_ABI_VERSION == 11  # functions were only added
  # NULL handle: an error code, no crash
  assert lib.sc_batch_naive_cluster(None, None, 0, 0.5, 0.5, None, None, None,
                                    None) == _lib.SC_ERR_INVALID
  assert lib.sc_batch_naive_check(None, None, 0, 0.5, 0.5, None, None) == _lib.SC_ERR_INVALID
  assert lib.sc_predict_batch_reduced_naive(None, None, 0, None, 0, 1, 0.5, 0.5, None, None, 16,
                                            None) == _lib.SC_ERR_INVALID
  assert lib.sc_predict_batch_single_naive(None, None, 0, None, 0.5, 0.5, None, None, 16,
                                           None) == _lib.SC_ERR_INVALID


def test_the_reference_restatement_reproduces_the_golden_walks():
  g = golden("fallback.npz")
  x = so.blobs(300, 16, 4, 101, noise=0.6)
  for key, threshold, adaptation in (("t5", 0.5, None), ("t7a9", 0.7, 0.9)):
    labels, counts, centroids, margin = _naive_ref.naive_walk(x, threshold, adaptation)
    assert margin > 1e-9
    assert np.array_equal(labels, g["naive_" + key])
    assert np.array_equal(counts, g["naive_counts_" + key])
    np.testing.assert_allclose(centroids, g["naive_cent_" + key], rtol=1e-13, atol=0)


def test_every_grid_case_is_decisive():
  margins, found = [], []
  for x, threshold, adaptation in _naive_ref.grid():
    labels, counts, _, margin = _naive_ref.naive_walk(x, threshold, adaptation)
    margins.append(margin)
    found.append(len(counts))
  assert min(margins) > 1e-9
  assert min(found) == 1 and max(found) > 4  # one centroid and many both occur


class FakeLib:
  """Records the batch calls; writes label 1, classifies / judges as the library does."""

  def __init__(self):
    self.calls = []

  def _reduced(self, name, arrays, count, mss, min_embeddings, lp, kinds, **extra):
    rows = [int(arrays[i].rows) for i in range(count)]
    for i, n in enumerate(rows):
      kinds[i] = 2 if n < min_embeddings else (1 if mss > 0 and n > mss else 0)
      for r in range(n):
        lp[i][r] = 1
    self.calls.append(dict(name=name, rows=rows, mss=mss, min_embeddings=min_embeddings, **extra))
    return 0

  def sc_predict_batch_reduced(self, raw, arrays, count, cfg, mss, min_embeddings, threshold,
                               lp, diags, group, kinds):
    return self._reduced("reduced", arrays, count, mss, min_embeddings, lp, kinds,
                         threshold=threshold, group=group)

  def sc_predict_batch_reduced_naive(self, raw, arrays, count, cfg, mss, min_embeddings,
                                     threshold, adaptation, lp, diags, group, kinds):
    return self._reduced("reduced_naive", arrays, count, mss, min_embeddings, lp, kinds,
                         threshold=threshold, adaptation=adaptation, group=group)

  def _single(self, name, arrays, count, lp, single, **extra):
    rows = [int(arrays[i].rows) for i in range(count)]
    for i, n in enumerate(rows):
      single[i] = i % 2
      for r in range(n):
        lp[i][r] = 1
    self.calls.append(dict(name=name, rows=rows, **extra))
    return 0

  def sc_predict_batch_single_fallback(self, raw, arrays, count, cfg, threshold, lp, diags, group,
                                       single):
    return self._single("single_fallback", arrays, count, lp, single, threshold=threshold,
                        group=group)

  def sc_predict_batch_single_naive(self, raw, arrays, count, cfg, threshold, adaptation, lp,
                                    diags, group, single):
    return self._single("single_naive", arrays, count, lp, single, threshold=threshold,
                        adaptation=adaptation, group=group)


def wire(monkeypatch, c):
  """`c` on a stand-in handle; predict() replaced by a recorder that returns int64 zeros."""
  handle, single = _batch_fake.wire(monkeypatch, c, FakeLib(), marker=0)
  return handle.lib.calls, single


def utts(*rows, d=3):
  return [np.ones((n, d)) for n in rows]


def naive_options(**kw):
  return fb.FallbackOptions(**kw)  # (the default type IS Naive)


def agglomerative_options(**kw):
  return fb.FallbackOptions(fallback_clusterer_type=fb.FallbackClustererType.Agglomerative, **kw)


def test_the_default_fallback_type_is_naive():
  assert fb.FallbackOptions().fallback_clusterer_type == fb.FallbackClustererType.Naive


def test_reduced_predicate_with_the_flag_on_and_off(monkeypatch):
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=4, max_spectral_size=12,
                            fallback_options=naive_options(spectral_min_embeddings=5))
  assert not c._reduced_batch_covers(utts(4, 9, 13), None, None)
  assert c._reduced_batch_covers(utts(4, 9, 13), None, None, naive=True)
  assert c._reduced_batch_covers(utts(9, 13), None, None)  # nobody needs the fallback
  calls, single = wire(monkeypatch, c)
  # off: the loop, as before
  got = c.predict_batch(utts(4, 9, 13))
  assert calls == [] and single == [4, 9, 13] and c.last_batch_routes == [0, 0, 0]
  # on: ONE call, None adaptation travels as the threshold, a one-row fallback member is fine
  del single[:]
  got = c.predict_batch(utts(1, 4, 5, 12, 13), batch_naive_fallback=True)
  assert single == []
  assert calls == [dict(name="reduced_naive", rows=[1, 4, 5, 12, 13], mss=12, min_embeddings=5,
                        threshold=0.5, adaptation=0.5, group=16)]
  assert c.last_batch_reduced == [2, 2, 0, 0, 1]
  assert [g.dtype for g in got] == [np.int64] * 4 + [np.float64]
  assert all(np.all(g == 1) for g in got) and len(c.last_batch_diags) == 5
  # no fallback utterance in the batch: the old call with the old arguments
  c.predict_batch(utts(5, 13), batch_naive_fallback=True, group=8)
  assert calls[-1] == dict(name="reduced", rows=[5, 13], mss=12, min_embeddings=5, threshold=0.5,
                           group=8)


def test_an_adaptation_threshold_travels(monkeypatch):
  c = sca.SpectralClusterer(fallback_options=naive_options(
      spectral_min_embeddings=5, naive_threshold=0.7, naive_adaptation_threshold=0.9))
  calls, single = wire(monkeypatch, c)
  c.predict_batch(utts(4, 9), batch_naive_fallback=True)
  assert calls[-1]["name"] == "reduced_naive"
  assert calls[-1]["threshold"] == 0.7 and calls[-1]["adaptation"] == 0.9 and single == []


@pytest.mark.parametrize("ctor,kwargs", [
    (dict(min_clusters=1), {}),
    (dict(), dict(group=1)),
    (dict(), dict(streams=2)),
    (dict(custom_dist="euclidean"), {}),
    (dict(affinity_function=lambda x: x), {}),
    (dict(post_eigen_cluster_function=lambda **kw: None), {}),
    (dict(max_spectral_size=4), {}),
], ids=["min1", "group1", "streams", "metric", "affinity", "kmeans", "mss<min"])
def test_the_flag_leaves_every_other_clause_of_the_reduced_predicate(monkeypatch, ctor, kwargs):
  c = sca.SpectralClusterer(fallback_options=naive_options(spectral_min_embeddings=5), **ctor)
  calls, single = wire(monkeypatch, c)
  c.predict_batch(utts(4, 9, 13), batch_naive_fallback=True, **kwargs)
  assert calls == [] and single == [4, 9, 13] and c.last_batch_routes == [0, 0, 0]


def single_clusterer(options, **kw):
  options.single_cluster_condition = fb.SingleClusterCondition.FallbackClusterer
  return sca.SpectralClusterer(min_clusters=1, max_clusters=4, fallback_options=options, **kw)


def test_single_predicate_with_the_flags_on_and_off(monkeypatch):
  c = single_clusterer(naive_options(naive_threshold=0.6))
  assert not c._fallback_condition_covers()
  assert c._fallback_condition_covers(naive=True)
  calls, single = wire(monkeypatch, c)
  # either flag alone keeps the loop
  for kwargs in ({}, dict(batch_fallback_condition=True), dict(batch_naive_fallback=True)):
    del single[:]
    c.predict_batch(utts(1, 4, 9), **kwargs)
    assert calls == [] and single == [1, 4, 9], kwargs
    assert c.last_batch_single is None
  del single[:]
  got = c.predict_batch(utts(1, 4, 9), batch_fallback_condition=True, batch_naive_fallback=True)
  assert single == []
  assert calls == [dict(name="single_naive", rows=[1, 4, 9], threshold=0.6, adaptation=0.6,
                        group=16)]
  assert c.last_batch_single == [False, True, False]
  assert np.array_equal(got[1], np.array([0] * 4)) and np.all(got[0] == 1) and np.all(got[2] == 1)


@pytest.mark.parametrize("ctor,kwargs", [
    (dict(max_spectral_size=12), {}),
    (dict(), dict(group=1)),
    (dict(), dict(streams=2)),
    (dict(custom_dist="euclidean"), {}),
    (dict(affinity_function=lambda x: x), {}),
], ids=["mss", "group1", "streams", "metric", "affinity"])
def test_the_flags_leave_every_other_clause_of_the_single_predicate(monkeypatch, ctor, kwargs):
  c = single_clusterer(naive_options(), **ctor)
  calls, single = wire(monkeypatch, c)
  c.predict_batch(utts(4, 9), batch_fallback_condition=True, batch_naive_fallback=True, **kwargs)
  assert calls == [] and single == [4, 9]


def test_the_agglomerative_type_gets_the_old_calls_with_the_old_arguments(monkeypatch):
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=4, max_spectral_size=12,
                            fallback_options=agglomerative_options(spectral_min_embeddings=5,
                                                                   agglomerative_threshold=0.4))
  calls, single = wire(monkeypatch, c)
  c.predict_batch(utts(4, 9, 13), batch_naive_fallback=True)
  assert calls == [dict(name="reduced", rows=[4, 9, 13], mss=12, min_embeddings=5, threshold=0.4,
                        group=16)] and single == []
  with pytest.raises(ValueError, match="Found array with 1 sample"):
    c.predict_batch(utts(1, 9), batch_naive_fallback=True)
  c = single_clusterer(agglomerative_options(agglomerative_threshold=0.3))
  calls, single = wire(monkeypatch, c)
  c.predict_batch(utts(4, 9), batch_fallback_condition=True, batch_naive_fallback=True)
  assert calls == [dict(name="single_fallback", rows=[4, 9], threshold=0.3, group=16)]
  assert single == []
  with pytest.raises(ValueError, match="Found array with 1 sample"):
    c.predict_batch(utts(1, 9), batch_fallback_condition=True, batch_naive_fallback=True)


def test_a_bad_threshold_pair_raises_before_anything_is_launched(monkeypatch):
  bad = dict(naive_threshold=0.7, naive_adaptation_threshold=0.5)
  c = sca.SpectralClusterer(fallback_options=naive_options(spectral_min_embeddings=5, **bad))
  calls, single = wire(monkeypatch, c)
  with pytest.raises(ValueError, match="adaptation_threshold cannot be smaller than threshold"):
    c.predict_batch(utts(4, 9), batch_naive_fallback=True)
  c = single_clusterer(naive_options(**bad))
  calls2, single2 = wire(monkeypatch, c)
  with pytest.raises(ValueError, match="adaptation_threshold cannot be smaller than threshold"):
    c.predict_batch(utts(4, 9), batch_fallback_condition=True, batch_naive_fallback=True)
  assert calls == [] and calls2 == [] and single == [] and single2 == []


def test_the_stream_pool_predicates_are_untouched():
  c = single_clusterer(naive_options())
  assert not c._fallback_condition_covers(min_embeddings_met=True)
  m = sca.MultiStageClusterer(main_clusterer=sca.SpectralClusterer(), fallback_threshold=0.5,
                              L=5, U1=10, U2=20)
  assert (m.main.fallback_options.fallback_clusterer_type ==
          fb.FallbackClustererType.Agglomerative)
