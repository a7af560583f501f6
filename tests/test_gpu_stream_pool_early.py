"""GPU: the stage of a MultiStageStreamPool at or below U1 rows, pooled (`pool_early_stage=True`):
sc_pool_fallback against sc_ahc and against sklearn's labels (tests/golden/
stream_pool_fallback.npz, tools/make_stream_pool_fallback_golden.py), sc_pool_cache, and the
pool against what each session's own MultiStageClusterer returns (every comparison is an
equality, values and dtype) and against outputs of the real reference (tests/golden/
fallback.npz)."""

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
  """The generator of tests/test_gpu_stream_pool.py."""
  rng = np.random.default_rng(seed)
  centres = np.linalg.qr(rng.standard_normal((d, speakers)))[0].T
  who = np.repeat(rng.integers(0, speakers, (count + run - 1) // run), run)[:count]
  return centres[who] + noise * rng.standard_normal((count, d))


def same(got, want):
  return got.dtype == want.dtype and np.array_equal(got, want)


def table_route(rows, L, U1):
  """The route of a session that holds `rows` rows after the append."""
  if rows == 1:
    return ms.ROUTE_MAIN_ONLY
  if rows < L:
    return ms.ROUTE_EARLY_FALLBACK
  return ms.ROUTE_EARLY_MAIN if rows <= U1 else ms.ROUTE_POOLED_GROUPED


# --- 1. sc_pool_fallback at the sizes where it can go wrong --------------------------------
# a single merge | the first chain restarts | one element per lane going to two | the LDS bound
# | the first session on the global-memory kernels
SIZES = (2, 3, 5, 33, 63, 64, 65, 96, 127, 128, 129)
WIDE_SIZES = (2, 64, 128)
THRESHOLDS = (("t05", 0.5), ("t19", 1.9))


def fallback(pool, ids, threshold, slots=None, labels_p=None):
  """One sc_pool_fallback call for the listed sessions -> labels per session."""
  handle, count = pool._pool_handle, len(ids)
  labels = [np.empty(max(handle.lib.sc_pool_rows(pool._pool, s), 1), dtype=np.int64)
            for s in ids]
  if slots is None:
    slots = (ctypes.c_int32 * count)(*ids)
  if labels_p is None:
    labels_p = (ctypes.POINTER(ctypes.c_int64) * count)(*[_lib.as_int64_p(l) for l in labels])
  handle.check(handle.lib.sc_pool_fallback(pool._pool, slots, count, float(threshold), labels_p))
  return labels


@pytest.fixture(scope="module")
def fallback_reference():
  """rows and sc_ahc's labels at both thresholds per case, computed once: d = 16 at every size
  (the golden's rows), d = 256 at three."""
  g = golden("stream_pool_fallback.npz")
  cases = {}
  for d, sizes in ((16, SIZES), (256, WIDE_SIZES)):
    for n in sizes:
      x = g["rows_%d" % n] if d == 16 else conversation(9000 + n, n, d=256, noise=0.05)
      cases[d, n] = (x, {tag: utils.cosine_agglomerative_clustering(
          x, linkage="average", distance_threshold=t) for tag, t in THRESHOLDS})
  return g, cases


def test_fallback_golden_is_well_conditioned():
  """The chain breaks ties on exact values and the cut compares heights with the threshold: the
  recorded inputs are a yardstick only while these are far above the 1e-15 that a reordered
  K = 16 sum moves."""
  g = golden("stream_pool_fallback.npz")
  for n in SIZES:
    for name in ("min_gap_%d", "height_gap_%d", "margin_%d"):
      assert float(g[name % n]) >= 1e-9, (name % n, float(g[name % n]))


@pytest.mark.parametrize("d,sizes", [(16, SIZES), (256, WIDE_SIZES)])
def test_pool_fallback_sizes(fallback_reference, d, sizes):
  g, cases = fallback_reference
  pool = ms.MultiStageStreamPool(make_main(), L=8, U1=24, U2=200, capacity=len(sizes) + 2,
                                 pool_early_stage=True)
  ids = []
  for n in sizes:
    ids.append(pool.open())
    pool.load(ids[-1], cases[d, n][0])
    assert pool._sessions[ids[-1]].mirror is None      # no host copy with the flag set
  for order in (list(range(len(sizes))), list(range(len(sizes)))[::-1]):
    for tag, t in THRESHOLDS:
      labels = fallback(pool, [ids[i] for i in order], t)
      for i, lab in zip(order, labels):
        assert np.array_equal(lab, cases[d, sizes[i]][1][tag]), (d, sizes[i], tag)
        if d == 16:
          assert np.array_equal(lab, g["labels_%d_%s" % (sizes[i], tag)]), (sizes[i], tag)
        if tag == "t19":
          assert not lab.any()                          # 1.9 merges everything
  # a slot with one row is label 0, alone and among others
  one = pool.open()
  pool.load(one, cases[d, sizes[-1]][0][:1])
  assert np.array_equal(fallback(pool, [one], 0.5)[0], [0])
  mixed = fallback(pool, [ids[0], one, ids[-1]], 0.5)
  assert np.array_equal(mixed[1], [0])
  assert np.array_equal(mixed[0], cases[d, sizes[0]][1]["t05"])
  assert np.array_equal(mixed[2], cases[d, sizes[-1]][1]["t05"])


def test_pool_fallback_errors(fallback_reference):
  _, cases = fallback_reference
  pool = ms.MultiStageStreamPool(make_main(), L=8, U1=24, U2=200, capacity=3, d=16,
                                 pool_early_stage=True)
  a, b, empty = pool.open(), pool.open(), pool.open()
  pool.load(a, cases[16, 33][0])
  pool.load(b, cases[16, 5][0])
  lib, raw = pool._pool_handle.lib, pool._pool
  with pytest.raises(ValueError):
    fallback(pool, [a, empty], 0.5)                     # a slot with no rows
  with pytest.raises(ValueError):
    fallback(pool, [a, b, a], 0.5)                      # a slot listed twice
  with pytest.raises(ValueError):
    fallback(pool, [a, 3], 0.5)                         # outside the pool
  slots = (ctypes.c_int32 * 2)(a, b)
  assert lib.sc_pool_fallback(raw, None, 2, 0.5,
                              (ctypes.POINTER(ctypes.c_int64) * 2)()) == _lib.SC_ERR_INVALID
  assert lib.sc_pool_fallback(raw, slots, 2, 0.5, None) == _lib.SC_ERR_INVALID
  with pytest.raises(ValueError):                       # a NULL entry of labels_out
    fallback(pool, [a, b], 0.5, labels_p=(ctypes.POINTER(ctypes.c_int64) * 2)())
  with pytest.raises(ValueError):
    pool._pool_handle.check(lib.sc_pool_cache(raw, empty, ctypes.byref(_lib.ScArray())))
  assert lib.sc_pool_cache(raw, a, None) == _lib.SC_ERR_INVALID
  # nothing above ran or moved anything: the next call is right
  labels = fallback(pool, [a, b], 0.5)
  assert np.array_equal(labels[0], cases[16, 33][1]["t05"])
  assert np.array_equal(labels[1], cases[16, 5][1]["t05"])


# --- 2. sc_pool_cache ------------------------------------------------------------------------
def test_pool_cache_descriptor():
  """d = 20: the slab rows are 32 doubles apart, so the descriptor is a strided view."""
  n, d = 40, 20
  rows = conversation(77, n, d=d)
  pool = ms.MultiStageStreamPool(make_main(), L=8, U1=60, U2=120, capacity=2,
                                 pool_early_stage=True)
  a = pool.open()
  pool.load(a, rows)
  handle = pool._pool_handle
  array = _lib.ScArray()
  handle.check(handle.lib.sc_pool_cache(pool._pool, a, ctypes.byref(array)))
  assert (array.rows, array.cols, array.row_stride, array.col_stride) == (n, d, 32, 1)
  assert (array.dtype, array.location) == (_lib.SC_DTYPE_F64, _lib.SC_MEM_DEVICE)
  got = np.empty((n, d))
  handle.check(handle.lib.sc_pool_get(pool._pool, a, _lib.SC_POOL_CACHE, _lib.as_double_p(got)))
  assert np.array_equal(got, rows)
  assert same(pool.main.predict_device_batch([array])[0], pool.main.predict(rows))


# --- 3. the pool equals independent sessions -------------------------------------------------
OFFSETS = (0, 3, 11, 29, 64)


@pytest.mark.parametrize("L,U1,U2", [(8, 24, 40), (20, 70, 130)])
def test_early_pool_equals_independent_sessions(L, U1, U2):
  """test_pool_equals_independent_sessions with the flag set: five sessions that start 0 / 3 /
  11 / 29 / 64 steps apart, 150 steps each, one of them reset at its step 90.  At every step
  every session's labels are those of its own MultiStageClusterer and its route is the one its
  row count asks for.  A session's first row (route 0) comes alone by construction; the offsets
  and the reset put sessions of the three routes that launch something -- 3, 4 and 1 -- into
  one step."""
  steps, reset_at, reset_session = 150, 90, 2
  rows = [conversation(seed, steps) for seed in range(5)]
  rows[reset_session][reset_at:] = conversation(50, steps - reset_at)
  pool = ms.MultiStageStreamPool(make_main(), L=L, U1=U1, U2=U2, capacity=5,
                                 pool_early_stage=True)
  ref_main = make_main()
  refs = [ms.MultiStageClusterer(ref_main, L=L, U1=U1, U2=U2) for _ in range(5)]
  ids = [pool.open() for _ in range(5)]
  seen_routes, mixed_steps = set(), 0
  for t in range(steps + OFFSETS[-1]):
    active = [k for k in range(5) if 0 <= t - OFFSETS[k] < steps]
    for k in active:
      if k == reset_session and t - OFFSETS[k] == reset_at:
        pool.reset(ids[k])
        refs[k] = ms.MultiStageClusterer(ref_main, L=L, U1=U1, U2=U2)
    outs = pool.streaming_predict([ids[k] for k in active],
                                  np.stack([rows[k][t - OFFSETS[k]] for k in active]))
    seen_routes.update(pool.last_routes)
    mixed_steps += {1, 3, 4} <= set(pool.last_routes)
    for k, got, route in zip(active, outs, pool.last_routes):
      want = refs[k].streaming_predict(rows[k][t - OFFSETS[k]])
      assert same(got, want), (k, t - OFFSETS[k], got, want)
      assert route == table_route(refs[k].num_embeddings, L, U1), (k, t - OFFSETS[k])
      assert pool._sessions[ids[k]].mirror is None
  assert seen_routes == {0, 1, 3, 4}
  assert mixed_steps > 0
  assert len(np.unique(outs[-1])) == 4     # (the streams end with their four speakers)


# --- 4. outputs of the real reference ---------------------------------------------------------
@pytest.mark.parametrize("tag,deflicker", [("none", ms.Deflicker.NoDeflicker),
                                           ("hungarian", ms.Deflicker.Hungarian)])
def test_early_pool_stream_vs_reference_golden(tag, deflicker):
  """test_pool_stream_vs_reference_golden with the flag set, that test's bars at all 16
  recorded steps; steps 10 and 30 are the pooled fallback and the cache in the grouped call."""
  g = golden("fallback.npz")
  stream = g["stream"]
  pool = ms.MultiStageStreamPool(make_main(), fallback_threshold=0.5, L=20, U1=60, U2=120,
                                 deflicker=deflicker, capacity=2, pool_early_stage=True)
  sessions = [pool.open(), pool.open()]
  lag, checked = 37, 0
  for t in range(len(stream) + lag):
    active = [(s, t - k * lag) for k, s in enumerate(sessions) if 0 <= t - k * lag < len(stream)]
    outs = pool.streaming_predict([s for s, _ in active],
                                  np.stack([stream[i] for _, i in active]))
    for (_, i), labels, route in zip(active, outs, pool.last_routes):
      assert route == table_route(i + 1, 20, 60), i + 1
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
  assert table_route(10, 20, 60) == 3 and table_route(30, 20, 60) == 4


# --- 5. U1 above the short route ----------------------------------------------------------------
def test_early_pool_main_clusterer_across_128_rows():
  """U1 = 160: caches of 121 .. 136 rows in the grouped main call cross the bound of its short
  route at 128 rows.  Sessions resumed with load()."""
  L, U1, U2, loaded, steps = 20, 160, 200, 120, 16
  rows = [conversation(20 + k, loaded + steps) for k in range(3)]
  pool = ms.MultiStageStreamPool(make_main(), L=L, U1=U1, U2=U2, capacity=3,
                                 pool_early_stage=True)
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
    assert pool.last_routes == [4, 4, 4]
    assert pool.main.last_batch_routes == [2 if t + 1 <= 128 else 1] * 3, t + 1
    for k, got in enumerate(outs):
      assert same(got, refs[k].streaming_predict(rows[k][t])), (k, t)


# --- 6. inputs --------------------------------------------------------------------------------
def test_early_pool_inputs_host_and_device_dtypes():
  """A float32 stream fed as widened float64 NumPy rows, as float32 NumPy rows and as float32
  device tensors with the flag set: the same labels, those of the float64 rows."""
  L, U1, U2, steps = 8, 24, 40, 60
  x32 = conversation(31, steps).astype(np.float32)
  pool = ms.MultiStageStreamPool(make_main(), L=L, U1=U1, U2=U2, capacity=3,
                                 pool_early_stage=True)
  ref = ms.MultiStageClusterer(make_main(), L=L, U1=U1, U2=U2)
  a, b, c = pool.open(), pool.open(), pool.open()
  on_device = torch.from_numpy(x32).to("cuda")
  for t in range(steps):
    want = ref.streaming_predict(x32[t].astype(np.float64))
    got = [pool.streaming_predict([a], x32[t:t + 1].astype(np.float64))[0],
           pool.streaming_predict([b], x32[t:t + 1])[0],
           pool.streaming_predict([c], on_device[t:t + 1])[0]]
    assert pool.last_routes == [table_route(t + 1, L, U1)]
    for labels in got:
      assert same(labels, want), t


# --- 7. a main clusterer the batch does not cover ------------------------------------------------
def test_early_flag_changes_nothing_for_min_clusters_1():
  """min_clusters = 1 is not in the library batch: with the flag set the early stage stays
  main.predict on the host mirror (route 0), then route 2 -- the labels of independent
  sessions."""
  L, U1, U2, steps = 8, 24, 40, 50
  rows = [conversation(40 + k, steps) for k in range(2)]
  pool = ms.MultiStageStreamPool(make_main(min_clusters=1), L=L, U1=U1, U2=U2, capacity=2,
                                 pool_early_stage=True)
  ref_main = make_main(min_clusters=1)
  refs = [ms.MultiStageClusterer(ref_main, L=L, U1=U1, U2=U2) for _ in range(2)]
  ids = [pool.open(), pool.open()]
  for t in range(steps):
    outs = pool.streaming_predict(ids, np.stack([rows[k][t] for k in range(2)]))
    assert pool.last_routes == ([0, 0] if t < U1 else [2, 2])
    for k, got in enumerate(outs):
      assert same(got, refs[k].streaming_predict(rows[k][t])), (k, t)


def test_missing_mirror_is_fetched_from_the_device():
  """A session loaded and stepped without a host mirror whose main clusterer then leaves the
  library batch: route 0 fetches the cache from the device."""
  L, U1, U2, loaded = 8, 24, 40, 5
  rows = conversation(60, 14)
  pool = ms.MultiStageStreamPool(make_main(), L=L, U1=U1, U2=U2, capacity=1,
                                 pool_early_stage=True)
  ref_main = make_main()
  ref = ms.MultiStageClusterer(ref_main, L=L, U1=U1, U2=U2)
  ref.cache, ref.num_embeddings = rows[:loaded].copy(), loaded
  a = pool.open()
  pool.load(a, rows[:loaded])
  for t in range(loaded, len(rows)):
    if t == 10:
      pool.main.min_clusters = ref_main.min_clusters = 1
    got = pool.streaming_predict([a], rows[t:t + 1])[0]
    assert pool.last_routes == [table_route(t + 1, L, U1) if t < 10 else 0]
    assert same(got, ref.streaming_predict(rows[t])), t
    if t >= 10:
      assert np.array_equal(pool._sessions[a].mirror, rows[:t + 1])
