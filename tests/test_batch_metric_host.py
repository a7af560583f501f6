"""CPU: predict_batch(..., batch_any_metric=True) and the same keyword of predict_affinity_batch.
The new symbols are declared, prototyped, exported and listed; with the flag and a device metric
other than cosine every one-call form makes its ONE library call with the handle's permission
(sc_set_batch_any_metric) set before and cleared after -- also when the call raises --, without
the flag the calls are today's, and cosine makes the same calls flag or no flag.  Driven with a
stand-in handle, no device."""

import os
import re

import numpy as np
import pytest

import _batch_fake
import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import fallback_clusterer as fb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sc_set_batch_any_metric", "sc_stage_kmeans_trace_metric",
               "sc_stage_kmeans_trace_group_metric")


def test_new_symbols_are_declared_prototyped_exported_and_listed():
  header = open(os.path.join(ROOT, "include", "spectralcluster_amd.h")).read()
  declared = set(re.findall(r"^int\s+(sc_[a-z0-9_]+)\s*\(", header, flags=re.M))
  integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
  lib = _lib.load()
  for name in NEW_SYMBOLS:
    assert name in declared, name
    assert name in _lib.PROTOTYPES, name
    assert hasattr(lib, name), name
    assert "`%s`" % name in integration, name
  assert lib.sc_abi_version() == 11  # functions were only added; sc_config is as it was
  assert lib.sc_set_batch_any_metric(None, 1) == _lib.SC_ERR_INVALID  # NULL handle: no crash


class FakeLib:
  """Every sc_* call is recorded by name -- the permission with its value -- and returns 0;
  `fail`: the name of a call that raises instead."""

  def __init__(self):
    self.events = []
    self.fail = None

  def __getattr__(self, name):
    if not name.startswith("sc_") or name == "sc_last_batch_routes":
      raise AttributeError(name)

    def call(*args):
      if name == "sc_set_batch_any_metric":
        self.events.append(("permit", args[1]))
      elif name != "sc_clear_constraint":
        self.events.append(("call", name))
        if name == self.fail:
          raise RuntimeError("the library call failed")
      return 0
    return call


def wire(monkeypatch, c):
  handle, looped = _batch_fake.wire(monkeypatch, c, FakeLib())
  return handle.lib, looped


def options(condition="AllAffinity"):
  return fb.FallbackOptions(
      spectral_min_embeddings=5,
      single_cluster_condition=getattr(fb.SingleClusterCondition, condition),
      single_cluster_affinity_threshold=0.6,
      fallback_clusterer_type=fb.FallbackClustererType.Agglomerative, agglomerative_threshold=0.4)


def band_options():
  return sca.ConstraintOptions(constraint_name=sca.ConstraintName.AffinityIntegration,
                               apply_before_refinement=False,
                               integration_type=sca.IntegrationType.Max)


def utts(*rows, d=3):
  return [np.ones((n, d)) for n in rows]


# form -> (clusterer keywords, predict_batch keywords for the rows, the form's library call)
def form(name, custom_dist, rows):
  single = fb.FallbackOptions(single_cluster_condition=fb.SingleClusterCondition.AllAffinity,
                              single_cluster_affinity_threshold=0.6)
  if name == "plain":
    return dict(min_clusters=2, max_clusters=4), {}, "sc_predict_batch_grouped"
  if name == "band":
    return (dict(min_clusters=2, max_clusters=4, constraint_options=band_options()),
            dict(constraint_matrices=[sca.ConstraintMatrix([0.0] * n, 1) for n in rows]),
            "sc_predict_batch_constrained")
  if name == "single":
    return (dict(min_clusters=1, max_clusters=4, fallback_options=single), {},
            "sc_predict_batch_single")
  if name == "reduced":
    return (dict(min_clusters=2, max_clusters=4, max_spectral_size=12,
                 fallback_options=options()), {}, "sc_predict_batch_reduced")
  if name == "multi_stage":
    return (dict(min_clusters=1, max_clusters=4, max_spectral_size=12,
                 fallback_options=options()), dict(batch_multi_stage=True),
            "sc_predict_batch_multi_stage")
  raise ValueError(name)


FORMS = ("plain", "band", "single", "reduced", "multi_stage")
ROWS = (6, 9, 13, 20)


def run(monkeypatch, name, custom_dist, fail=False, **flag):
  kwargs, call, symbol = form(name, custom_dist, ROWS)
  c = sca.SpectralClusterer(custom_dist=custom_dist, **kwargs)
  lib, looped = wire(monkeypatch, c)
  if fail:
    lib.fail = symbol
    with pytest.raises(RuntimeError, match="the library call failed"):
      c.predict_batch(utts(*ROWS), **call, **flag)
  else:
    got = c.predict_batch(utts(*ROWS), **call, **flag)
    assert [len(g) for g in got] == list(ROWS)
  return c, lib.events, looped, symbol


@pytest.mark.parametrize("metric", ["euclidean", "cityblock", "correlation", "minkowski"])
@pytest.mark.parametrize("name", FORMS)
def test_with_the_flag_each_form_is_one_call_under_the_permission(monkeypatch, name, metric):
  c, events, looped, symbol = run(monkeypatch, name, metric, batch_any_metric=True)
  assert looped == []
  assert events == [("permit", 1), ("call", symbol), ("permit", 0)]
  assert c._batch_any_metric is False


@pytest.mark.parametrize("name", FORMS)
def test_the_permission_is_cleared_when_the_call_raises(monkeypatch, name):
  c, events, looped, symbol = run(monkeypatch, name, "euclidean", fail=True,
                                  batch_any_metric=True)
  assert events == [("permit", 1), ("call", symbol), ("permit", 0)] and looped == []
  assert c._batch_any_metric is False


@pytest.mark.parametrize("flag", [{}, {"batch_any_metric": False}], ids=["default", "false"])
@pytest.mark.parametrize("name", FORMS)
def test_without_the_flag_the_loop_runs(monkeypatch, name, flag):
  c, events, looped, symbol = run(monkeypatch, name, "euclidean", **flag)
  if name == "plain":
    # the plain batch is a library call today as well: the loop runs inside it (routes all 0),
    # because nobody gave the permission
    assert events == [("call", symbol)] and looped == []
  else:
    assert events == [] and looped == list(ROWS)
    assert c.last_batch_routes == [0] * len(ROWS)


@pytest.mark.parametrize("name", FORMS)
def test_cosine_makes_the_same_calls_flag_or_no_flag(monkeypatch, name):
  _, plain, looped_plain, symbol = run(monkeypatch, name, "cosine")
  _, flagged, looped_flagged, _ = run(monkeypatch, name, "cosine", batch_any_metric=True)
  assert plain == flagged == [("call", symbol)]
  assert looped_plain == looped_flagged == []


@pytest.mark.parametrize("call", [dict(group=1), dict(streams=2)], ids=["group1", "streams"])
def test_group1_and_streams_take_no_permission(monkeypatch, call):
  c = sca.SpectralClusterer(custom_dist="euclidean", min_clusters=2, max_clusters=4)
  lib, looped = wire(monkeypatch, c)
  c.predict_batch(utts(*ROWS), batch_any_metric=True, **call)
  assert lib.events == [("call", "sc_predict_batch_streams")] and looped == []


@pytest.mark.parametrize("flag", [False, True])
def test_a_metric_that_is_not_on_the_device_raises_as_today(monkeypatch, flag):
  c = sca.SpectralClusterer(custom_dist="mahalanobis", min_clusters=2, max_clusters=4)
  lib, looped = wire(monkeypatch, c)
  with pytest.raises(_lib.UnsupportedOnDeviceError, match="mahalanobis"):
    c.predict_batch(utts(*ROWS), batch_any_metric=flag)
  assert lib.events == []
  # ... and where today's batch is the loop, predict() is what raises: the loop runs
  kwargs, call, _ = form("reduced", "mahalanobis", ROWS)
  c = sca.SpectralClusterer(custom_dist="mahalanobis", **kwargs)
  lib, looped = wire(monkeypatch, c)
  c.predict_batch(utts(*ROWS), batch_any_metric=flag, **call)
  assert lib.events == [] and looped == list(ROWS)


def test_autotune_batches_ignore_the_flag(monkeypatch):
  tune = sca.AutoTune(p_percentile_min=0.5, p_percentile_max=0.9, init_search_step=0.1,
                      search_level=1)
  seq = [sca.RefinementName.RowWiseThreshold]
  ref = sca.RefinementOptions(refinement_sequence=seq, p_percentile=0.9)
  for flag in (False, True):
    c = sca.SpectralClusterer(custom_dist="euclidean", min_clusters=2, max_clusters=4,
                              autotune=tune, refinement_options=ref)
    lib, looped = wire(monkeypatch, c)
    c.predict_batch(utts(*ROWS), autotune_from_entry_state=True, batch_any_metric=flag)
    assert lib.events == [] and looped == list(ROWS)


def test_the_flag_is_keyword_only_on_both_methods():
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=4)
  with pytest.raises(TypeError):
    c.predict_batch(utts(6, 9), None, None, None, False, False, False, False, True)
  with pytest.raises(TypeError):
    c.predict_affinity_batch([np.eye(6)], None, None, True)


@pytest.mark.parametrize("constrained", [False, True], ids=["plain", "band"])
def test_predict_affinity_batch_takes_the_flag(monkeypatch, constrained):
  kwargs = dict(constraint_options=band_options()) if constrained else {}
  cms = [sca.ConstraintMatrix([0.0] * n, 1) for n in (6, 9)] if constrained else None
  mats = [np.eye(6), np.eye(9)]
  c = sca.SpectralClusterer(custom_dist="euclidean", min_clusters=2, max_clusters=4, **kwargs)
  lib, _ = wire(monkeypatch, c)
  looped = []
  monkeypatch.setattr(c, "predict_affinity",
                      lambda a, cm=None: looped.append(len(a)) or np.zeros(len(a), np.int64))
  c.predict_affinity_batch(mats, cms, batch_any_metric=True)
  assert lib.events == [("permit", 1), ("call", "sc_predict_batch_affinities"), ("permit", 0)]
  assert looped == []
  lib.events.clear()
  c.predict_affinity_batch(mats, cms)
  if constrained:  # today: cosine when constraints travel, else the loop
    assert lib.events == [] and looped == [6, 9]
  else:
    assert lib.events == [("call", "sc_predict_batch_affinities")] and looped == []
