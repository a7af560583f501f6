"""GPU: MultiStageStreamPool -- many multi-stage streaming sessions advanced per call, caches
resident on the device -- against what each session's own MultiStageClusterer returns (every
comparison is an equality, values and dtype), against outputs of the real reference
(tests/golden/fallback.npz) and, for the pooled pre-clusterer alone, against sklearn's labels
(tests/golden/stream_pool_ahc.npz, tools/make_stream_pool_golden.py)."""

import ctypes

import numpy as np
import pytest
# (at module level on purpose: PyTorch has to be in the process before the library is loaded,
#  so that both use one HIP runtime -- INTEGRATION.md section 6)
import torch

import spectral_oracle as so
from conftest import golden

import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import multi_stage_clusterer as ms
from spectralcluster_amd import utils

pytestmark = pytest.mark.gpu


def make_main(**kwargs):
  options = sca.RefinementOptions(gaussian_blur_sigma=0, p_percentile=0.2,
                                  refinement_sequence=sca.ICASSP2018_REFINEMENT_SEQUENCE)
  return sca.SpectralClusterer(refinement_options=options, stop_eigenvalue=0.01, **kwargs)


def conversation(seed, count, d=16, speakers=4, noise=0.02, run=5):
  """`count` rows: speakers are orthonormal directions (no common shift), turns in runs of
  `run` rows, noise * N(0, I) on every row."""
  rng = np.random.default_rng(seed)
  centres = np.linalg.qr(rng.standard_normal((d, speakers)))[0].T
  who = np.repeat(rng.integers(0, speakers, (count + run - 1) // run), run)[:count]
  return centres[who] + noise * rng.standard_normal((count, d))


def same(got, want):
  return got.dtype == want.dtype and np.array_equal(got, want)


# --- 1. outputs of the real reference ----------------------------------------------------
@pytest.mark.parametrize("tag,deflicker", [("none", ms.Deflicker.NoDeflicker),
                                           ("hungarian", ms.Deflicker.Hungarian)])
def test_pool_stream_vs_reference_golden(tag, deflicker):
  """The 360-row stream of the existing single-stream golden test through two sessions of one
  pool, the second 37 steps behind: each crosses L = 20, U1 = 60 and U2 = 120 while the other
  is in another stage.  The existing test's bars at every recorded step of both."""
  g = golden("fallback.npz")
  stream = g["stream"]
  pool = ms.MultiStageStreamPool(make_main(), fallback_threshold=0.5, L=20, U1=60, U2=120,
                                 deflicker=deflicker, capacity=2)
  sessions = [pool.open(), pool.open()]
  lag, checked = 37, 0
  for t in range(len(stream) + lag):
    active = [(s, t - k * lag) for k, s in enumerate(sessions) if 0 <= t - k * lag < len(stream)]
    outs = pool.streaming_predict([s for s, _ in active],
                                  np.stack([stream[i] for _, i in active]))
    for (_, i), labels in zip(active, outs):
      key = "ms_%s_%d" % (tag, i + 1)
      if key in g:
        want = g[key]
        checked += 1
        if deflicker == ms.Deflicker.Hungarian and i + 1 > 60:
          np.testing.assert_array_equal(labels, want)     # the matching pins the numbering
          assert labels.dtype == want.dtype
        else:
          assert so.adjusted_rand_index(np.asarray(labels).astype(int), want.astype(int)) == 1.0
  assert checked == 16     # steps 10, 30, 61, 119, 120, 121, 200, 360 of two sessions


# --- 2. the pool equals independent sessions ---------------------------------------------
OFFSETS = (0, 3, 11, 29, 64)


@pytest.mark.parametrize("L,U1,U2", [(8, 24, 40), (20, 70, 130)])
def test_pool_equals_independent_sessions(L, U1, U2):
  """Five sessions that start 0 / 3 / 11 / 29 / 64 steps apart, 150 steps each, one of them
  reset at its step 90: at every step every session's labels are those of its own
  MultiStageClusterer.  (8, 24, 40): the cache crosses U1 = 24 and is compressed every 16
  steps; (20, 70, 130): cache sizes cross one and two waves (64, 128)."""
  steps, reset_at, reset_session = 150, 90, 2
  rows = [conversation(seed, steps) for seed in range(5)]
  rows[reset_session][reset_at:] = conversation(50, steps - reset_at)
  pool = ms.MultiStageStreamPool(make_main(), L=L, U1=U1, U2=U2, capacity=5)
  ref_main = make_main()
  refs = [ms.MultiStageClusterer(ref_main, L=L, U1=U1, U2=U2) for _ in range(5)]
  ids = [pool.open() for _ in range(5)]
  seen_routes = set()
  for t in range(steps + OFFSETS[-1]):
    active = [k for k in range(5) if 0 <= t - OFFSETS[k] < steps]
    for k in active:
      if k == reset_session and t - OFFSETS[k] == reset_at:
        pool.reset(ids[k])
        refs[k] = ms.MultiStageClusterer(ref_main, L=L, U1=U1, U2=U2)
    outs = pool.streaming_predict([ids[k] for k in active],
                                  np.stack([rows[k][t - OFFSETS[k]] for k in active]))
    seen_routes.update(pool.last_routes)
    for k, got in zip(active, outs):
      want = refs[k].streaming_predict(rows[k][t - OFFSETS[k]])
      assert same(got, want), (k, t - OFFSETS[k], got, want)
  assert seen_routes == {0, 1}
  assert len(np.unique(outs[-1])) == 4     # (the streams end with their four speakers)


def test_pool_main_clusterer_above_128_centroids():
  """U1 = 160: the main clusterer sees 160 centroids per session, more than the short route
  takes, so the grouped call runs them as a lockstep group.  Sessions resumed with load()."""
  L, U1, U2, loaded, steps = 20, 160, 200, 195, 12
  rows = [conversation(20 + k, loaded + steps) for k in range(3)]
  pool = ms.MultiStageStreamPool(make_main(), L=L, U1=U1, U2=U2, capacity=3)
  ref_main = make_main()
  refs, ids = [], []
  for k in range(3):
    ids.append(pool.open())
    pool.load(ids[k], rows[k][:loaded])
    ref = ms.MultiStageClusterer(ref_main, L=L, U1=U1, U2=U2)
    ref.cache, ref.num_embeddings = rows[k][:loaded].copy(), loaded   # the same resumed state
    refs.append(ref)
  for t in range(loaded, loaded + steps):
    outs = pool.streaming_predict(ids, np.stack([rows[k][t] for k in range(3)]))
    assert pool.last_routes == [1, 1, 1]
    assert len(pool.main.last_batch_routes) == 3
    for k, got in enumerate(outs):
      assert same(got, refs[k].streaming_predict(rows[k][t])), (k, t)


# --- 3. the pooled pre-clusterer at the sizes where it can go wrong -----------------------
SIZES = (25, 63, 64, 65, 129, 1025)   # one merge | around one wave | ... | workgroup + 1


def precluster(pool, ids):
  """One sc_pool_precluster call for the listed sessions -> (labels, centroids) per session."""
  handle, count = pool._pool_handle, len(ids)
  labels = [np.empty(handle.lib.sc_pool_rows(pool._pool, s), dtype=np.int64) for s in ids]
  handle.check(handle.lib.sc_pool_precluster(
      pool._pool, (ctypes.c_int32 * count)(*ids), count,
      (ctypes.POINTER(ctypes.c_int64) * count)(*[_lib.as_int64_p(l) for l in labels])))
  centroids = []
  for s in ids:
    centroids.append(np.empty((pool.U1, pool.d), dtype=np.float64))
    handle.check(handle.lib.sc_pool_get(pool._pool, s, _lib.SC_POOL_CENTROIDS,
                                        _lib.as_double_p(centroids[-1])))
  return labels, centroids


@pytest.fixture(scope="module")
def ahc_reference():
  """rows, sc_ahc's labels and centroids per case, computed once: d = 16 at every size (the
  golden's rows), d = 256 at the three smallest."""
  g = golden("stream_pool_ahc.npz")
  cases = {}
  for d, sizes in ((16, SIZES), (256, SIZES[:3])):
    for n in sizes:
      x = (g["rows_%d" % n] if d == 16
           else np.random.default_rng(9000 + n).standard_normal((n, d)))
      labels = utils.cosine_agglomerative_clustering(x, n_clusters=24)
      cases[d, n] = (x, labels, utils.get_cluster_centroids(x, labels))
  return g, cases


@pytest.mark.parametrize("d,sizes", [(16, SIZES), (256, SIZES[:3])])
def test_pool_precluster_sizes(ahc_reference, d, sizes):
  g, cases = ahc_reference
  pool = ms.MultiStageStreamPool(make_main(), L=8, U1=24, U2=1100, capacity=len(sizes))
  ids = []
  for n in sizes:
    ids.append(pool.open())
    pool.load(ids[-1], cases[d, n][0])
    got = np.empty((n, d))
    pool._pool_handle.check(pool._pool_handle.lib.sc_pool_get(
        pool._pool, ids[-1], _lib.SC_POOL_CACHE, _lib.as_double_p(got)))
    assert np.array_equal(got, cases[d, n][0])
  for order in (list(range(len(sizes))), list(range(len(sizes)))[::-1]):
    labels, centroids = precluster(pool, [ids[i] for i in order])
    for i, lab, cen in zip(order, labels, centroids):
      x, want_labels, want_centroids = cases[d, sizes[i]]
      assert np.array_equal(lab, want_labels), (d, sizes[i])
      assert np.array_equal(cen.view(np.int64), want_centroids.view(np.int64)), (d, sizes[i])
      if d == 16:
        assert np.array_equal(lab, g["labels_%d" % sizes[i]]), sizes[i]   # sklearn itself


# --- 4. inputs ---------------------------------------------------------------------------
def test_pool_inputs_host_and_device_dtypes():
  """A float32 stream fed as widened float64 NumPy rows, as float32 NumPy rows and as float32
  device tensors: the same labels, those of the float64 rows."""
  L, U1, U2, steps = 8, 24, 40, 60
  x32 = conversation(31, steps).astype(np.float32)
  pool = ms.MultiStageStreamPool(make_main(), L=L, U1=U1, U2=U2, capacity=3)
  ref = ms.MultiStageClusterer(make_main(), L=L, U1=U1, U2=U2)
  a, b, c = pool.open(), pool.open(), pool.open()
  on_device = torch.from_numpy(x32).to("cuda")
  for t in range(steps):
    want = ref.streaming_predict(x32[t].astype(np.float64))
    got = [pool.streaming_predict([a], x32[t:t + 1].astype(np.float64))[0],
           pool.streaming_predict([b], x32[t:t + 1])[0],
           pool.streaming_predict([c], on_device[t:t + 1])[0]]
    for labels in got:
      assert same(labels, want), t


# --- 5. errors and limits ------------------------------------------------------------------
def test_pool_errors_and_limits():
  pool = ms.MultiStageStreamPool(make_main(), L=8, U1=24, U2=40, capacity=2)
  a, b = pool.open(), pool.open()
  with pytest.raises(RuntimeError):
    pool.open()
  assert pool.streaming_predict([], np.zeros((0, 16))) == []
  row = conversation(1, 2)
  pool.streaming_predict([a, b], row)
  for sessions, rows in (([a, b], np.zeros((2, 17))),     # another width
                         ([a, a], row),                   # a duplicate
                         ([a, 7], row),                   # never opened
                         ([a], row)):                     # one id, two rows
    with pytest.raises(ValueError):
      pool.streaming_predict(sessions, rows)
  pool.close(b)
  with pytest.raises(ValueError):
    pool.streaming_predict([a, b], row)                   # a closed id
  with pytest.raises(ValueError):
    pool.load(a, conversation(2, 40))                     # 1 + 40 rows > U2
  # nothing above was appended: the next step of `a` is its second
  assert pool.streaming_predict([a], row[:1])[0].shape == (2,)
  assert pool.open() == b
  with pytest.raises(ValueError):
    ms.MultiStageStreamPool(sca.SpectralClusterer(max_spectral_size=50))
  with pytest.raises(MemoryError):                        # 60000 distance matrices of 9.7 MB
    ms.MultiStageStreamPool(make_main(), L=8, U1=24, U2=1100, capacity=60000)


def test_pool_min_clusters_1_takes_per_session_main_calls():
  """min_clusters = 1 (the single-cluster test) is not in the library batch: pooled
  pre-cluster, then main.predict per session (route 2) -- with the labels of independent
  sessions."""
  L, U1, U2, steps = 8, 24, 40, 50
  rows = [conversation(40 + k, steps) for k in range(2)]
  pool = ms.MultiStageStreamPool(make_main(min_clusters=1), L=L, U1=U1, U2=U2, capacity=2)
  ref_main = make_main(min_clusters=1)
  refs = [ms.MultiStageClusterer(ref_main, L=L, U1=U1, U2=U2) for _ in range(2)]
  ids = [pool.open(), pool.open()]
  for t in range(steps):
    outs = pool.streaming_predict(ids, np.stack([rows[k][t] for k in range(2)]))
    assert pool.last_routes == ([0, 0] if t < U1 else [2, 2])
    for k, got in enumerate(outs):
      assert same(got, refs[k].streaming_predict(rows[k][t])), (k, t)
