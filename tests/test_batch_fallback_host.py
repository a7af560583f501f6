"""CPU: the batched FallbackClusterer single-cluster test (sc_batch_fallback_check,
sc_predict_batch_single_fallback) is declared, prototyped, exported and documented, and
SpectralClusterer.predict_batch / MultiStageStreamPool route to it exactly when asked to and able
to -- driven with a stand-in handle, no device."""

import os
import re

import numpy as np
import pytest

import _batch_fake
import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import fallback_clusterer as fb
from spectralcluster_amd import multi_stage_clusterer as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sc_batch_fallback_check", "sc_predict_batch_single_fallback")


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
  assert lib.sc_abi_version() == 11  # functions were only added
  assert "no batched form" not in header
  # NULL handle: an error code, no crash
  assert lib.sc_batch_fallback_check(None, None, 0, 0.5, None, None) == _lib.SC_ERR_INVALID
  assert lib.sc_predict_batch_single_fallback(None, None, 0, None, 0.5, None, None, 16,
                                              None) == _lib.SC_ERR_INVALID


def clusterer_with(kind="Agglomerative", condition="FallbackClusterer", **kwargs):
  options = fb.FallbackOptions(
      single_cluster_condition=getattr(fb.SingleClusterCondition, condition),
      fallback_clusterer_type=getattr(fb.FallbackClustererType, kind),
      agglomerative_threshold=0.3125)
  return sca.SpectralClusterer(min_clusters=1, max_clusters=6, fallback_options=options, **kwargs)


class FakeLib:
  """Records the call; says "single" for every utterance of fewer than 10 rows."""

  def __init__(self):
    self.calls = []

  def sc_clear_constraint(self, raw):
    return 0

  def sc_predict_batch_single_fallback(self, raw, arrays, count, cfg, threshold, lp, diags, group,
                                       single):
    rows = [int(arrays[i].rows) for i in range(count)]
    for i, n in enumerate(rows):
      single[i] = 1 if n < 10 else 0
      for r in range(n):
        lp[i][r] = 0 if n < 10 else 1 + r % 2
    self.calls.append(dict(rows=rows, group=group, threshold=threshold,
                           min_clusters=cfg.min_clusters))
    return 0


def with_fake_handle(clusterer):
  # (the loop's marker is 7; build_config stays the clusterer's own)
  return _batch_fake.wire(None, clusterer, FakeLib(), keep_config=True)[0]


BATCH = [np.ones((n, 4)) for n in (5, 12, 9, 200)]


def test_with_the_flag_the_batch_is_one_call():
  clusterer = clusterer_with()
  handle = with_fake_handle(clusterer)
  got = clusterer.predict_batch(BATCH, batch_fallback_condition=True)
  assert handle.lib.calls == [dict(rows=[5, 12, 9, 200], group=16, threshold=0.3125,
                                   min_clusters=1)]
  assert clusterer.last_batch_single == [True, False, True, False]
  for u, labels, one in zip(BATCH, got, clusterer.last_batch_single):
    want = np.array([0] * u.shape[0]) if one else 1 + np.arange(u.shape[0]) % 2
    assert labels.dtype == want.dtype and np.array_equal(labels, want)
  # the described-sources form makes the same call
  arrays = [_lib.ScArray(u.ctypes.data, _lib.SC_DTYPE_F64, _lib.SC_MEM_HOST, u.shape[0], 4, 4, 1)
            for u in BATCH]
  got = clusterer.predict_device_batch(arrays, batch_fallback_condition=True)
  assert len(handle.lib.calls) == 2 and handle.lib.calls[1] == handle.lib.calls[0]
  assert [len(l) for l in got] == [5, 12, 9, 200]
  # an utterance of one row: predict()'s ValueError, before any call
  with pytest.raises(ValueError, match="Found array with 1 sample"):
    clusterer.predict_batch([np.ones((5, 4)), np.ones((1, 4))], batch_fallback_condition=True)
  assert len(handle.lib.calls) == 2


def test_without_the_flag_there_is_no_call():
  clusterer = clusterer_with()
  handle = with_fake_handle(clusterer)
  got = clusterer.predict_batch(BATCH)
  assert handle.lib.calls == []
  assert all((l == 7).all() for l in got)
  assert clusterer.last_batch_routes == [0] * 4 and clusterer.last_batch_single is None
  # the predicates the other batch forms ask are as they were
  assert clusterer._single_check_struct() is None
  assert not clusterer._library_batch_covers()
  assert not clusterer._library_batch_covers(single_check_covered=True)


@pytest.mark.parametrize("how", ["naive", "constraints", "autotune", "reduced", "streams",
                                 "group1", "euclidean", "min_embeddings", "min_clusters_2"])
def test_what_keeps_the_loop_despite_the_flag(how):
  kwargs, call, kind = {}, {}, "Agglomerative"
  if how == "naive":
    kind = "Naive"
  if how == "constraints":
    kwargs["constraint_options"] = sca.ConstraintOptions(
        constraint_name=sca.ConstraintName.AffinityIntegration, apply_before_refinement=False,
        integration_type=sca.IntegrationType.Max)
    call["constraint_matrices"] = [None] * 4
  if how == "autotune":
    kwargs["autotune"] = sca.AutoTune()
  if how == "reduced":
    kwargs["max_spectral_size"] = 50
  if how == "streams":
    call["streams"] = 2
  if how == "group1":
    call["group"] = 1
  if how == "euclidean":
    kwargs["custom_dist"] = "euclidean"
  clusterer = clusterer_with(kind, **kwargs)
  if how == "min_embeddings":
    clusterer.fallback_options.spectral_min_embeddings = 3
  if how == "min_clusters_2":
    clusterer.min_clusters = 2
  handle = with_fake_handle(clusterer)
  if how == "min_clusters_2":
    # (a min_clusters=2 clusterer is the library batch's: keep it off the stand-in handle)
    clusterer._library_batch_covers = lambda *a, **k: False
  got = clusterer.predict_batch(BATCH, batch_fallback_condition=True, **call)
  assert handle.lib.calls == []
  assert all((l == 7).all() for l in got)
  assert clusterer.last_batch_routes == [0] * 4 and clusterer.last_batch_single is None


def test_an_affinity_condition_ignores_the_flag():
  clusterer = clusterer_with(condition="AllAffinity")
  assert not clusterer._fallback_condition_covers()
  assert clusterer._library_batch_covers(single_check_covered=True)


def test_pool_predicate_reads_the_flag_with_a_default():
  main = clusterer_with()
  pool = ms.MultiStageStreamPool.__new__(ms.MultiStageStreamPool)   # (no attribute set)
  pool.main, pool.L, pool.U1 = main, 1, 4
  assert not pool._main_is_batchable()
  pool.pool_fallback_condition = True
  assert pool._main_is_batchable()
  pool.pool_early_stage = True
  assert pool._early_pooled()
  main.fallback_options.fallback_clusterer_type = fb.FallbackClustererType.Naive
  assert not pool._main_is_batchable() and not pool._early_pooled()
  # L rows are vouched for by the pool (spectral_min_embeddings = L <= U1)
  main = clusterer_with()
  main.fallback_options.spectral_min_embeddings = 3
  pool.main, pool.L = main, 3
  assert pool._main_is_batchable()
  assert not main._fallback_condition_covers()
