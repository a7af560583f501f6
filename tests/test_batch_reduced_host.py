"""CPU: the size-reducing batch (sc_batch_ahc, sc_set_reduce_wave_bytes,
sc_predict_batch_reduced) is exported and prototyped, and SpectralClusterer.predict_batch routes
to it exactly when its predicate holds -- driven with a stand-in handle, no device."""

import os
import re

import numpy as np
import pytest

import _batch_fake
import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import fallback_clusterer as fb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sc_batch_ahc", "sc_set_reduce_wave_bytes", "sc_predict_batch_reduced")


def test_new_symbols_are_declared_prototyped_and_exported():
  header = open(os.path.join(ROOT, "include", "spectralcluster_amd.h")).read()
  declared = set(re.findall(r"^int\s+(sc_[a-z0-9_]+)\s*\(", header, flags=re.M))
  lib = _lib.load()
  for name in NEW_SYMBOLS:
    assert name in declared, name
    assert name in _lib.PROTOTYPES, name
    assert hasattr(lib, name), name
  assert re.search(r"SC_BATCH_ROUTE_FALLBACK\s*=\s*3\b", header)
  assert _lib.BATCH_ROUTE_FALLBACK == 3
  assert lib.sc_abi_version() == 11  # functions were only added
  # NULL handle: an error code, no crash
  assert lib.sc_set_reduce_wave_bytes(None, 0) == _lib.SC_ERR_INVALID
  assert lib.sc_batch_ahc(None, None, 0, 1, 2, 0.0, None, None) == _lib.SC_ERR_INVALID
  assert lib.sc_predict_batch_reduced(None, None, 0, None, 0, 1, 0.5, None, None, 16,
                                      None) == _lib.SC_ERR_INVALID


class FakeLib:
  """Records the size-reducing call; classifies as the library does and writes label 1."""

  def __init__(self):
    self.calls = []

  def sc_predict_batch_reduced(self, raw, arrays, count, cfg, mss, min_embeddings, threshold,
                               lp, diags, group, kinds):
    rows = [int(arrays[i].rows) for i in range(count)]
    for i, n in enumerate(rows):
      kinds[i] = 2 if n < min_embeddings else (1 if mss > 0 and n > mss else 0)
      for r in range(n):
        lp[i][r] = 1
    self.calls.append(dict(rows=rows, mss=mss, min_embeddings=min_embeddings,
                           threshold=threshold, group=group))
    return 0


def wire(monkeypatch, c):
  """`c` on a stand-in handle; predict() replaced by a recorder that returns int64 zeros."""
  handle, single = _batch_fake.wire(monkeypatch, c, FakeLib(), marker=0)
  return handle.lib.calls, single


def agglomerative(min_embeddings=100, threshold=0.4):
  return fb.FallbackOptions(spectral_min_embeddings=min_embeddings,
                            fallback_clusterer_type=fb.FallbackClustererType.Agglomerative,
                            agglomerative_threshold=threshold)


def utts(*rows, d=3):
  return [np.ones((n, d)) for n in rows]


def test_kind_classification_at_the_boundaries_and_result_dtypes(monkeypatch):
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=4, max_spectral_size=12,
                            fallback_options=agglomerative(min_embeddings=5))
  calls, single = wire(monkeypatch, c)
  got = c.predict_batch(utts(4, 5, 12, 13))
  assert single == []
  assert calls == [dict(rows=[4, 5, 12, 13], mss=12, min_embeddings=5, threshold=0.4, group=16)]
  assert c.last_batch_reduced == [_lib.BATCH_KIND_FALLBACK, _lib.BATCH_KIND_SPECTRAL,
                                  _lib.BATCH_KIND_SPECTRAL, _lib.BATCH_KIND_REDUCED]
  assert [c._batch_kind(n) for n in (4, 5, 12, 13)] == c.last_batch_reduced
  # predict()'s dtypes: chain_labels' float64 for the size-reduced utterance, int64 otherwise
  assert [g.dtype for g in got] == [np.int64, np.int64, np.int64, np.float64]
  assert [g.shape for g in got] == [(4,), (5,), (12,), (13,)]
  assert all(np.all(g == 1) for g in got)
  assert len(c.last_batch_diags) == 4
  # an explicit group travels; an empty batch is no call at all
  c.predict_batch(utts(13, 20), group=8)
  assert calls[-1]["group"] == 8 and len(calls) == 2
  assert c.predict_batch([]) == [] and len(calls) == 2 and c.last_batch_reduced == []


def test_either_option_alone_routes(monkeypatch):
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=4, max_spectral_size=12)
  calls, single = wire(monkeypatch, c)
  c.predict_batch(utts(1, 13))  # (no fallback: a 1-row utterance is a spectral member)
  assert calls[-1]["mss"] == 12 and calls[-1]["min_embeddings"] == 1 and single == []
  assert c.last_batch_reduced == [0, 1]
  c = sca.SpectralClusterer(fallback_options=agglomerative(min_embeddings=5))
  calls, single = wire(monkeypatch, c)
  c.predict_batch(utts(4, 9))
  assert calls[-1]["mss"] == 0 and calls[-1]["min_embeddings"] == 5 and single == []
  # a Naive fallback type is fine as long as no utterance needs the fallback
  c = sca.SpectralClusterer(max_spectral_size=12,
                            fallback_options=fb.FallbackOptions(spectral_min_embeddings=5))
  calls, single = wire(monkeypatch, c)
  c.predict_batch(utts(5, 13))
  assert len(calls) == 1 and single == []


@pytest.mark.parametrize("ctor,kwargs", [
    # the Naive fallback with an utterance that needs it
    (dict(max_spectral_size=12, fallback_options=fb.FallbackOptions(spectral_min_embeddings=5)),
     {}),
    (dict(max_spectral_size=12, min_clusters=1), {}),
    (dict(max_spectral_size=12), dict(group=1)),
    (dict(max_spectral_size=12), dict(streams=2)),
    (dict(max_spectral_size=12), dict(streams=2, group=4)),
    (dict(max_spectral_size=12, custom_dist="euclidean"), {}),
    (dict(max_spectral_size=12, autotune=sca.AutoTune(
        p_percentile_min=0.5, p_percentile_max=0.9, init_search_step=0.1, search_level=1)), {}),
    (dict(max_spectral_size=12, affinity_function=lambda x: x), {}),
    (dict(max_spectral_size=12, post_eigen_cluster_function=lambda **kw: None), {}),
    # the centroids would be fallback members themselves
    (dict(max_spectral_size=4, fallback_options=agglomerative(min_embeddings=5)), {}),
], ids=["naive", "min1", "group1", "streams", "streams+group", "metric", "autotune", "affinity",
        "kmeans", "mss<min"])
def test_everything_outside_the_predicate_keeps_the_loop(monkeypatch, ctor, kwargs):
  c = sca.SpectralClusterer(**ctor)
  calls, single = wire(monkeypatch, c)
  got = c.predict_batch(utts(4, 9, 13), **kwargs)
  assert calls == [] and single == [4, 9, 13]
  assert c.last_batch_routes == [0, 0, 0]
  assert [g.dtype for g in got] == [np.int64] * 3


def test_constraints_keep_the_loop(monkeypatch):
  c = sca.SpectralClusterer(
      max_spectral_size=12,
      constraint_options=sca.ConstraintOptions(
          constraint_name=sca.ConstraintName.AffinityIntegration, apply_before_refinement=False,
          integration_type=sca.IntegrationType.Max))
  calls, single = wire(monkeypatch, c)
  c.predict_batch(utts(4, 9), constraint_matrices=[np.eye(4), np.eye(9)])
  assert calls == [] and single == [4, 9]
  c.predict_batch(utts(4, 13))  # the options alone constrain nothing
  assert len(calls) == 1


def test_a_clusterer_without_either_option_is_untouched(monkeypatch):
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=4)
  assert not c._reduced_batch_covers(utts(5, 7), None, None)
  assert c._library_batch_covers()
  assert not sca.SpectralClusterer(max_spectral_size=12)._library_batch_covers()


def test_errors_before_anything_is_launched(monkeypatch):
  c = sca.SpectralClusterer(max_clusters=7, max_spectral_size=7)
  calls, _ = wire(monkeypatch, c)
  with pytest.raises(ValueError, match="max_spectral_size should be a relatively big number"):
    c.predict_batch(utts(5, 8))
  c.predict_batch(utts(5, 7))  # nobody exceeds the size: nothing to complain about
  assert len(calls) == 1
  c = sca.SpectralClusterer(fallback_options=agglomerative(min_embeddings=5))
  calls, _ = wire(monkeypatch, c)
  with pytest.raises(ValueError, match="Found array with 1 sample"):
    c.predict_batch(utts(1, 9))
  with pytest.raises(ValueError, match="same d"):
    c.predict_batch([np.ones((4, 3)), np.ones((9, 2))])
  with pytest.raises(ValueError, match="same d"):
    c.predict_batch([np.ones((4, 3)), np.ones(9)])
  assert calls == []


def test_batch_ahc_argument_errors_need_no_device():
  x = np.ones((4, 3))
  with pytest.raises(_lib.UnsupportedOnDeviceError):
    sca.utils.cosine_agglomerative_clustering_batch([x], n_clusters=2, linkage="ward")
  with pytest.raises(ValueError, match="Exactly one of n_clusters and distance_threshold"):
    sca.utils.cosine_agglomerative_clustering_batch([x])
  with pytest.raises(ValueError, match="Exactly one of n_clusters and distance_threshold"):
    sca.utils.cosine_agglomerative_clustering_batch([x], n_clusters=2, distance_threshold=0.5)
  with pytest.raises(ValueError, match="2-dimensional"):
    sca.utils.cosine_agglomerative_clustering_batch([np.ones(4)], n_clusters=2)
  assert sca.utils.cosine_agglomerative_clustering_batch([], n_clusters=2) == []
