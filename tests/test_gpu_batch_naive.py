"""GPU: predict_batch(batch_naive_fallback=True) -- the Naive fallback type, what a default
FallbackOptions selects, inside the two batch calls (`sc_predict_batch_reduced_naive`,
`sc_predict_batch_single_naive`) -- against per-utterance predict(), and
NaiveClusterer.predict_batch against a fresh NaiveClusterer per utterance."""

import ctypes

import numpy as np
import pytest
# (at module level on purpose: PyTorch has to be in the process before the library is loaded,
#  so that both use one HIP runtime -- INTEGRATION.md section 6)
import torch  # noqa: F401
import spectral_oracle as so

import _naive_ref
import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import fallback_clusterer as fb
from spectralcluster_amd.naive_clusterer import NaiveClusterer

pytestmark = pytest.mark.gpu


def refinement():
  return sca.RefinementOptions(gaussian_blur_sigma=1, p_percentile=0.95,
                               refinement_sequence=sca.ICASSP2018_REFINEMENT_SEQUENCE)


class CountingLib:
  """The handle's library with every sc_ call counted by name."""

  def __init__(self, lib):
    self._lib = lib
    self.names = []

  def __getattr__(self, name):
    fn = getattr(self._lib, name)
    if not name.startswith("sc_"):
      return fn

    def counted(*args):
      self.names.append(name)
      return fn(*args)

    return counted


def batch_without_predict(monkeypatch, c, utterances, **kwargs):
  """predict_batch with predict() forbidden; returns (labels, the batch / predict calls made)."""
  handle = c._handle()
  lib = CountingLib(handle.lib)
  with monkeypatch.context() as m:
    m.setattr(handle, "_lib", lib)  # (what the `lib` property returns)
    m.setattr(c, "predict", lambda *a, **k: pytest.fail("predict() inside the batch"))
    got = c.predict_batch(utterances, **kwargs)
  return got, [n for n in lib.names if n.startswith(("sc_predict", "sc_batch", "sc_naive"))]


# --- the reduced form -------------------------------------------------------------------------
REDUCED_ROWS = (1, 40, 99, 100, 128, 129, 300)


def reduced_clusterer(**options):
  return sca.SpectralClusterer(
      min_clusters=2, max_clusters=7, max_spectral_size=128, refinement_options=refinement(),
      fallback_options=fb.FallbackOptions(spectral_min_embeddings=100, **options))


def test_reduced_batch_with_naive_fallback_members(monkeypatch):
  c = reduced_clusterer()
  assert c.fallback_options.fallback_clusterer_type == fb.FallbackClustererType.Naive
  utts = [so.blobs(n, 16, 3, 500 + n, noise=0.6) for n in REDUCED_ROWS]
  kinds = [c._batch_kind(n) for n in REDUCED_ROWS]
  assert kinds == [2, 2, 2, 0, 0, 1, 1]
  # the fallback members' walks are decisive, and not all of one centroid
  walks = [_naive_ref.naive_walk(u, 0.5) for u, k in zip(utts, kinds) if k == 2]
  assert min(w[3] for w in walks) > 1e-9 and max(len(w[1]) for w in walks) > 1
  got, calls = batch_without_predict(monkeypatch, c, utts, batch_naive_fallback=True)
  assert calls == ["sc_predict_batch_reduced_naive"]
  assert c.last_batch_reduced == kinds
  routes = c.last_batch_routes
  assert [r == _lib.BATCH_ROUTE_FALLBACK for r in routes] == [k == 2 for k in kinds]
  assert all(r != 0 for r in routes)
  assert [d.n for d in c.last_batch_diags] == [0, 0, 0, 100, 128, 128, 128]
  for u, lab, kind, walk in zip(utts, got, kinds, walks + [None] * 4):
    want = c.predict(u)
    assert lab.dtype == want.dtype and np.array_equal(lab, want), u.shape
    if kind == 2:
      assert np.array_equal(lab, walk[0])
  # without the flag: the loop, as today
  got = c.predict_batch(utts)
  assert c.last_batch_routes == [0] * len(utts)


def test_the_agglomerative_type_ignores_the_flag():
  c = reduced_clusterer(fallback_clusterer_type=fb.FallbackClustererType.Agglomerative,
                        agglomerative_threshold=0.4)
  utts = [so.blobs(n, 16, 3, 500 + n, noise=0.6) for n in REDUCED_ROWS[1:]]
  plain = c.predict_batch(utts)
  plain_routes, plain_kinds = c.last_batch_routes, c.last_batch_reduced
  flagged = c.predict_batch(utts, batch_naive_fallback=True)
  assert c.last_batch_routes == plain_routes and c.last_batch_reduced == plain_kinds
  assert plain_routes[0] == _lib.BATCH_ROUTE_FALLBACK
  for a, b in zip(plain, flagged):
    assert a.dtype == b.dtype and np.array_equal(a, b)


# --- the single form --------------------------------------------------------------------------
SINGLE_ROWS = (1, 30, 128, 129, 400)


def single_clusterer(**options):
  return sca.SpectralClusterer(
      min_clusters=1, max_clusters=6, refinement_options=refinement(),
      fallback_options=fb.FallbackOptions(
          single_cluster_condition=fb.SingleClusterCondition.FallbackClusterer, **options))


def single_batch():
  """Per size one single-speaker blob (tight: every row joins centroid 0) and one of three
  speakers."""
  utts = []
  for n in SINGLE_ROWS:
    utts.append(so.blobs(n, 16, 1, 600 + n, noise=0.1))
    utts.append(so.blobs(n, 16, 3, 700 + n, noise=0.1))
  return utts


def test_single_batch_with_the_naive_condition(monkeypatch):
  c = single_clusterer()
  utts = single_batch()
  walks = [_naive_ref.naive_walk(u, 0.5) for u in utts]
  assert min(w[3] for w in walks) > 1e-9
  want_single = [_naive_ref.verdict(w[0])[0] for w in walks]
  # one row is single; the single-speaker blobs are; the three-speaker ones of several rows not
  assert want_single == [True, True] + [True, False] * 4
  got, calls = batch_without_predict(monkeypatch, c, utts, batch_fallback_condition=True,
                                     batch_naive_fallback=True)
  assert calls == ["sc_predict_batch_single_naive"]
  assert c.last_batch_single == want_single
  for u, lab, one, route, diag in zip(utts, got, want_single, c.last_batch_routes,
                                      c.last_batch_diags):
    want = c.predict(u)
    assert lab.dtype == want.dtype and np.array_equal(lab, want), u.shape
    assert (route == _lib.BATCH_ROUTE_FALLBACK) == one
    assert (bytes(diag) == b"\0" * ctypes.sizeof(_lib.ScDiag)) == one
  # a small wave budget (the rows do not all stay on the device): the same results
  handle = c._handle()
  handle.check(handle.lib.sc_set_reduce_wave_bytes(handle.raw, 64 << 10))
  try:
    again = c.predict_batch(utts, batch_fallback_condition=True, batch_naive_fallback=True)
  finally:
    handle.check(handle.lib.sc_set_reduce_wave_bytes(handle.raw, 0))
  assert c.last_batch_single == want_single
  assert all(np.array_equal(a, b) for a, b in zip(got, again))


def test_one_flag_alone_keeps_the_loop():
  c = single_clusterer()
  utts = single_batch()[2:6]
  for kwargs in (dict(batch_fallback_condition=True), dict(batch_naive_fallback=True)):
    got = c.predict_batch(utts, **kwargs)
    assert c.last_batch_routes == [0] * 4 and c.last_batch_single is None
    for u, lab in zip(utts, got):
      assert np.array_equal(lab, c.predict(u))


def test_a_zero_row_names_its_utterance_and_leaves_the_handle_usable():
  c = single_clusterer()
  utts = single_batch()[2:8]
  bad = utts[2].copy()  # (a single-speaker utterance: the verdict does not excuse the row)
  bad[17] = 0.0
  flags = dict(batch_fallback_condition=True, batch_naive_fallback=True)
  with pytest.raises(ValueError, match="utterance 2"):
    c.predict_batch(utts[:2] + [bad] + utts[3:], **flags)
  nan = utts[1].copy()
  nan[3, 3] = np.nan
  with pytest.raises(ValueError, match="utterance 1"):
    c.predict_batch([utts[0], nan, bad], **flags)
  got = c.predict_batch(utts, **flags)
  for u, lab in zip(utts, got):
    assert np.array_equal(lab, c.predict(u))


def test_a_bad_threshold_pair_raises_before_any_launch(monkeypatch):
  bad = dict(naive_threshold=0.7, naive_adaptation_threshold=0.5)
  for c, kwargs in ((reduced_clusterer(**bad), dict(batch_naive_fallback=True)),
                    (single_clusterer(**bad), dict(batch_fallback_condition=True,
                                                   batch_naive_fallback=True))):
    handle = c._handle()
    lib = CountingLib(handle.lib)
    with monkeypatch.context() as m:
      m.setattr(handle, "_lib", lib)  # (what the `lib` property returns)
      with pytest.raises(ValueError, match="adaptation_threshold cannot be smaller"):
        c.predict_batch([so.blobs(40, 16, 2, 1), so.blobs(150, 16, 2, 2)], **kwargs)
    assert lib.names == []


# --- NaiveClusterer.predict_batch ---------------------------------------------------------------
def test_naive_clusterer_predict_batch_is_a_fresh_predict_per_utterance():
  utts = [so.blobs(n, 24, 3, 800 + n, noise=0.6) for n in (1, 2, 50, 130, 300)]
  utts.append(utts[3].astype(np.float32))
  utts.append(torch.from_numpy(utts[4]).cuda())
  c = NaiveClusterer(0.5, 0.8)
  c.predict(utts[2])  # some online state
  state = [(s.embedding.copy(), s.count) for s in c.centroids]
  assert len(state) > 1
  got, centroids, counts = c.predict_batch(utts, return_state=True)
  assert all(g.dtype == np.int64 for g in got)
  assert all(np.array_equal(a, b) for a, b in zip(c.predict_batch(utts), got))
  for u, lab, cent, cnt in zip(utts, got, centroids, counts):
    x = u.cpu().numpy() if isinstance(u, torch.Tensor) else u.astype(np.float64)
    fresh = NaiveClusterer(0.5, 0.8)
    assert np.array_equal(lab, fresh.predict(x))
    assert np.array_equal(cnt, fresh._counts)
    assert np.array_equal(cent.view(np.uint64), fresh._centroids.view(np.uint64))
  after = [(s.embedding, s.count) for s in c.centroids]
  assert len(after) == len(state)
  assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(state, after))
  assert c.predict_batch([]) == []
