"""CPU: the multi-stage regime with min_clusters=1 as one call (sc_predict_batch_multi_stage,
sc_multi_stage_layout) is declared, prototyped, exported and listed, its struct mirror has the
header's layout, and SpectralClusterer.predict_batch(..., batch_multi_stage=True) routes to it
exactly when its predicate holds -- driven with a stand-in handle, no device."""

import ctypes
import os
import re

import numpy as np
import pytest

import _batch_fake
import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import fallback_clusterer as fb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sc_predict_batch_multi_stage", "sc_multi_stage_layout")
CONDITIONS = ("AffinityGmmBic", "AllAffinity", "NeighborAffinity", "AffinityStd",
              "FallbackClusterer")
FALLBACK_TYPES = ("Agglomerative", "Naive")
FIELDS = ["max_spectral_size", "spectral_min_embeddings", "fallback_type",
          "agglomerative_threshold", "naive_threshold", "naive_adaptation_threshold",
          "single_condition", "single_threshold", "diagonal_offset"]


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
  assert lib.sc_abi_version() == 11  # functions and a struct were only added
  assert re.search(r"SC_SINGLE_BY_FALLBACK\s*=\s*5\b", header)
  assert _lib.SC_SINGLE_BY_FALLBACK == fb.SingleClusterCondition.FallbackClusterer.value == 5
  # NULL handle: an error code, no crash
  assert lib.sc_predict_batch_multi_stage(None, None, 0, None, None, None, None, 16, None,
                                          None) == _lib.SC_ERR_INVALID


def test_multi_stage_mirror_has_the_headers_layout():
  lib = _lib.load()
  size, offsets = ctypes.c_int(0), (ctypes.c_int * len(FIELDS))()
  assert lib.sc_multi_stage_layout(ctypes.byref(size), offsets) == 0
  assert size.value == ctypes.sizeof(_lib.ScMultiStage)
  assert [name for name, _ in _lib.ScMultiStage._fields_] == FIELDS
  assert list(offsets) == [getattr(_lib.ScMultiStage, f).offset for f in FIELDS]
  # the header declares the fields in that order
  header = open(os.path.join(ROOT, "include", "spectralcluster_amd.h")).read()
  body = re.search(r"typedef struct sc_multi_stage \{(.*?)\} sc_multi_stage;", header, re.S)
  assert re.findall(r"^\s*(?:int32_t|double)\s+(\w+);", body.group(1), flags=re.M) == FIELDS
  # the enum values the struct carries are the reference's
  assert fb.FallbackClustererType.Agglomerative.value == 1
  assert fb.FallbackClustererType.Naive.value == 2
  # either out pointer may be NULL
  assert lib.sc_multi_stage_layout(None, None) == 0


class FakeLib:
  """Records the call; classifies as the library does, says "single" for every tested member of
  an odd number of rows, writes label 1 elsewhere."""

  def __init__(self):
    self.calls = []

  def sc_predict_batch_multi_stage(self, raw, arrays, count, cfg, stage, lp, diags, group, kinds,
                                   single):
    stage = ctypes.cast(stage, ctypes.POINTER(_lib.ScMultiStage)).contents
    rows = [int(arrays[i].rows) for i in range(count)]
    mss, low = stage.max_spectral_size, stage.spectral_min_embeddings
    for i, n in enumerate(rows):
      kinds[i] = 2 if n < low else (1 if mss > 0 and n > mss else 0)
      single[i] = -1 if kinds[i] == 2 else n % 2
      for r in range(n):
        lp[i][r] = 0 if single[i] == 1 else 1
    self.calls.append(dict(rows=rows, group=group,
                           stage={f: getattr(stage, f) for f in FIELDS}))
    return 0


def wire(monkeypatch, c):
  """`c` on a stand-in handle; predict() replaced by a recorder that returns int64 sevens."""
  handle, looped = _batch_fake.wire(monkeypatch, c, FakeLib())
  return handle.lib.calls, looped


def options(condition="AffinityGmmBic", fallback_type="Agglomerative", min_embeddings=5,
            **kwargs):
  return fb.FallbackOptions(
      spectral_min_embeddings=min_embeddings,
      single_cluster_condition=getattr(fb.SingleClusterCondition, condition),
      single_cluster_affinity_threshold=0.6, single_cluster_affinity_diagonal_offset=2,
      fallback_clusterer_type=getattr(fb.FallbackClustererType, fallback_type),
      agglomerative_threshold=0.4, naive_threshold=0.3, **kwargs)


def clusterer(condition="AffinityGmmBic", fallback_type="Agglomerative", min_embeddings=5,
              max_spectral_size=12, **kwargs):
  return sca.SpectralClusterer(min_clusters=1, max_clusters=4,
                               max_spectral_size=max_spectral_size,
                               fallback_options=options(condition, fallback_type, min_embeddings),
                               **kwargs)


def utts(*rows, d=3):
  return [np.ones((n, d)) for n in rows]


@pytest.mark.parametrize("fallback_type", FALLBACK_TYPES)
@pytest.mark.parametrize("condition", CONDITIONS)
def test_one_call_with_the_struct_filled_from_the_options(monkeypatch, condition, fallback_type):
  c = clusterer(condition, fallback_type)
  calls, looped = wire(monkeypatch, c)
  batch = utts(4, 5, 8, 12, 13, 20)
  got = c.predict_batch(batch, batch_multi_stage=True)
  assert looped == [] and len(calls) == 1
  naive = fallback_type == "Naive"
  assert calls[0] == dict(rows=[4, 5, 8, 12, 13, 20], group=16, stage=dict(
      max_spectral_size=12, spectral_min_embeddings=5,
      fallback_type=2 if naive else 1, agglomerative_threshold=0.4,
      # (a None adaptation threshold arrives as the threshold; neither is read otherwise)
      naive_threshold=0.3 if naive else 0.0, naive_adaptation_threshold=0.3 if naive else 0.0,
      single_condition=getattr(fb.SingleClusterCondition, condition).value,
      single_threshold=0.6, diagonal_offset=2))
  assert c.last_batch_reduced == [2, 0, 0, 0, 1, 1]
  assert [c._batch_kind(n) for n in (4, 5, 8, 12, 13, 20)] == c.last_batch_reduced
  assert c.last_batch_single == [None, True, False, False, True, False]
  assert len(c.last_batch_diags) == 6
  # predict()'s dtypes: chain_labels' float64 for a size-reduced utterance (zeros when its
  # centroids are single), np.array([0] * n) for a single one, int64 otherwise
  want = [np.ones(4, dtype=np.int64), np.array([0] * 5), np.ones(8, dtype=np.int64),
          np.ones(12, dtype=np.int64), np.zeros(13), np.ones(20)]
  for g, w in zip(got, want):
    assert g.dtype == w.dtype and np.array_equal(g, w)


def test_without_the_flag_the_loop_runs(monkeypatch):
  c = clusterer()
  calls, looped = wire(monkeypatch, c)
  got = c.predict_batch(utts(4, 9, 13))
  assert calls == [] and looped == [4, 9, 13]
  assert c.last_batch_routes == [0, 0, 0] and c.last_batch_single is None
  assert all((g == 7).all() for g in got)
  got = c.predict_batch(utts(4, 9, 13), batch_multi_stage=False)
  assert calls == [] and looped == [4, 9, 13] * 2
  # the flag is keyword only
  with pytest.raises(TypeError):
    c.predict_batch(utts(4, 9), None, None, None, False, False, False, True)


def test_either_size_option_alone_a_batch_of_one_an_explicit_group_an_empty_batch(monkeypatch):
  c = clusterer(max_spectral_size=None)
  calls, looped = wire(monkeypatch, c)
  c.predict_batch(utts(4, 9), batch_multi_stage=True)
  assert calls[-1]["stage"]["max_spectral_size"] == 0 and looped == []
  c = clusterer(min_embeddings=1)
  calls, looped = wire(monkeypatch, c)
  got = c.predict_batch(utts(13), batch_multi_stage=True, group=8)
  assert calls[-1]["stage"]["spectral_min_embeddings"] == 1 and calls[-1]["group"] == 8
  assert calls[-1]["rows"] == [13] and looped == []
  assert len(got) == 1 and got[0].dtype == np.float64
  assert c.predict_batch([], batch_multi_stage=True) == [] and len(calls) == 1
  assert c.last_batch_reduced == [] and c.last_batch_single == []


@pytest.mark.parametrize("how", ["constraints", "autotune", "group1", "streams", "euclidean",
                                 "mss<min", "neither", "affinity", "kmeans"])
@pytest.mark.parametrize("flag", [False, True])
def test_what_keeps_the_loop(monkeypatch, how, flag):
  kwargs, call = {}, {}
  if how == "constraints":
    kwargs["constraint_options"] = sca.ConstraintOptions(
        constraint_name=sca.ConstraintName.AffinityIntegration, apply_before_refinement=False,
        integration_type=sca.IntegrationType.Max)
    call["constraint_matrices"] = [None, None, None]
  if how == "autotune":
    kwargs["autotune"] = sca.AutoTune(p_percentile_min=0.5, p_percentile_max=0.9,
                                      init_search_step=0.1, search_level=1)
  if how == "group1":
    call["group"] = 1
  if how == "streams":
    call["streams"] = 2
  if how == "euclidean":
    kwargs["custom_dist"] = "euclidean"
  if how == "mss<min":
    kwargs["max_spectral_size"] = 4   # the centroids would be fallback members themselves
  if how == "affinity":
    kwargs["affinity_function"] = lambda x: x
  if how == "kmeans":
    kwargs["post_eigen_cluster_function"] = lambda **kw: None
  c = clusterer(**kwargs)
  if how == "neither":
    c.max_spectral_size = None
    c.fallback_options.spectral_min_embeddings = 1
    c.fallback_options.single_cluster_condition = fb.SingleClusterCondition.FallbackClusterer
  calls, looped = wire(monkeypatch, c)
  got = c.predict_batch(utts(4, 9, 13), batch_multi_stage=flag, **call)
  assert calls == [] and looped == [4, 9, 13]
  assert c.last_batch_routes == [0, 0, 0] and c.last_batch_single is None
  assert all((g == 7).all() for g in got)


def test_other_clusterers_answer_as_they_did(monkeypatch):
  assert clusterer()._multi_stage_batch_covers()
  c = clusterer()
  c.min_clusters = 2   # sc_predict_batch_reduced's batch, flag or no flag
  assert not c._multi_stage_batch_covers() and c._reduced_batch_covers(utts(4, 13), None, None)
  assert not sca.SpectralClusterer(min_clusters=1)._multi_stage_batch_covers()
  # the flag changes no predicate of the sibling calls
  c = clusterer()
  assert not c._library_batch_covers(single_check_covered=True)
  assert not c._reduced_batch_covers(utts(4, 13), None, None)
  assert not clusterer("FallbackClusterer")._fallback_condition_covers()


def test_errors_carry_the_index_and_come_before_any_call(monkeypatch):
  # max_spectral_size not above max_clusters: the size-reduced utterance is named
  c = clusterer("AffinityStd", max_spectral_size=4, min_embeddings=2)
  calls, _ = wire(monkeypatch, c)
  with pytest.raises(ValueError, match=r"max_spectral_size should be a relatively big number "
                                       r"\(utterance 2\)"):
    c.predict_batch(utts(3, 4, 5), batch_multi_stage=True)
  c.predict_batch(utts(3, 4), batch_multi_stage=True)   # nobody exceeds the size
  assert len(calls) == 1
  # an agglomerative fallback utterance of one row; the Naive type takes it
  c = clusterer()
  calls, _ = wire(monkeypatch, c)
  with pytest.raises(ValueError, match=r"Found array with 1 sample.*\(utterance 1\)"):
    c.predict_batch(utts(9, 1), batch_multi_stage=True)
  assert calls == []
  c = clusterer(fallback_type="Naive")
  calls, _ = wire(monkeypatch, c)
  c.predict_batch(utts(9, 1), batch_multi_stage=True)
  assert len(calls) == 1
  # AffinityGmmBic, offset 2: a spectral utterance of 3 rows; for a size-reduced utterance the
  # tested rows are the max_spectral_size centroids
  c = clusterer(min_embeddings=2)
  calls, _ = wire(monkeypatch, c)
  with pytest.raises(ValueError, match=r"diagonal_offset must be significantly smaller.*"
                                       r"\(utterance 1\)"):
    c.predict_batch(utts(9, 3, 1), batch_multi_stage=True)
  c = clusterer(min_embeddings=2, max_spectral_size=3)
  c.max_clusters = 2
  calls, _ = wire(monkeypatch, c)
  with pytest.raises(ValueError, match=r"diagonal_offset must be significantly smaller.*"
                                       r"\(utterance 0\)"):
    c.predict_batch(utts(50), batch_multi_stage=True)
  # ... a fallback utterance is not tested, and the other conditions do not read the offset
  c = clusterer(min_embeddings=4)
  calls, _ = wire(monkeypatch, c)
  c.predict_batch(utts(9, 3), batch_multi_stage=True)
  c = clusterer("AffinityStd", min_embeddings=2)
  calls2, _ = wire(monkeypatch, c)
  c.predict_batch(utts(9, 3), batch_multi_stage=True)
  assert len(calls) == 1 and len(calls2) == 1
  # the FallbackClusterer condition with the agglomerative type tests a spectral utterance of
  # one row: AgglomerativeClustering's error
  c = clusterer("FallbackClusterer", min_embeddings=1)
  calls, _ = wire(monkeypatch, c)
  with pytest.raises(ValueError, match=r"Found array with 1 sample.*\(utterance 2\)"):
    c.predict_batch(utts(9, 3, 1), batch_multi_stage=True)
  assert calls == []
  # NaiveClusterer's threshold pair
  c = clusterer(fallback_type="Naive")
  c.fallback_options.naive_adaptation_threshold = 0.1
  calls, _ = wire(monkeypatch, c)
  with pytest.raises(ValueError, match="adaptation_threshold cannot be smaller than threshold"):
    c.predict_batch(utts(9, 3), batch_multi_stage=True)
  with pytest.raises(ValueError, match="same d"):
    c.predict_batch([np.ones((4, 3)), np.ones((9, 2))], batch_multi_stage=True)
  assert calls == []
