"""GPU: k_naive_cluster_batch (naive_batch.hip) through `sc_batch_naive_cluster` and
`sc_batch_naive_check`: the NumPy reference's labels on a grid where every decision has a margin,
and `sc_naive_cluster`'s labels, counts and centroids BIT FOR BIT per member.

Grid (tests/_naive_ref.py): d = 3, 64, 255 (idle threads of the 256-thread stride), 256 (exactly
full), 257 (a second term in one thread only), 600 (ragged), plus d = 1; n = 1, 2, 65, 300;
(threshold, adaptation) = (0.5, None), (0.7, 0.9) on four blobs, (0.2, 0.2) on one.  A call takes
one threshold pair and arrays of one width, so the grid is one call per (pair, d): the four sizes
of a width share it."""

import ctypes

import numpy as np
import pytest
# (at module level on purpose: PyTorch has to be in the process before the library is loaded,
#  so that both use one HIP runtime -- INTEGRATION.md section 6)
import torch
import spectral_oracle as so
from conftest import golden

import _naive_ref
from spectralcluster_amd import _dlpack
from spectralcluster_amd import _lib
from spectralcluster_amd.naive_clusterer import NaiveClusterer

pytestmark = pytest.mark.gpu

SENTINEL = -7


def raw_cluster(members, threshold, adaptation, want_state=True):
  """sc_batch_naive_cluster into sentinel-filled outputs: (rc, message, labels, found, centroids,
  counts)."""
  handle = _lib.default_handle()
  sources = [_dlpack.describe(x, lambda: handle) for x in members]
  try:
    count = len(sources)
    rows = [s.shape[0] for s in sources]
    d = sources[0].shape[1]
    labels = [np.full(n, SENTINEL, dtype=np.int64) for n in rows]
    found = np.full(count, SENTINEL, dtype=np.int32)
    centroids = [np.full((n, d), float(SENTINEL)) for n in rows]
    counts = [np.full(n, SENTINEL, dtype=np.int32) for n in rows]
    lp = (ctypes.POINTER(ctypes.c_int64) * count)(*[_lib.as_int64_p(l) for l in labels])
    cp = (ctypes.POINTER(ctypes.c_double) * count)(*[_lib.as_double_p(c) for c in centroids])
    kp = (ctypes.POINTER(ctypes.c_int32) * count)(
        *[c.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) for c in counts])
    rc = handle.lib.sc_batch_naive_cluster(
        handle.raw, (_lib.ScArray * count)(*[s.array for s in sources]), count, float(threshold),
        float(threshold if adaptation is None else adaptation), lp,
        found.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), cp if want_state else None,
        kp if want_state else None)
  finally:
    for s in sources:
      s.release()
  return rc, handle.last_error(), labels, found, centroids, counts


def single_call(x64, threshold, adaptation):
  """sc_naive_cluster from the empty state: (labels, counts, centroids)."""
  c = NaiveClusterer(threshold, adaptation)
  labels = c.predict(x64)
  return labels, c._counts, c._centroids


def assert_same_bits(got, want, what):
  got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
  assert got.shape == want.shape, what
  assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), what


def check_member_is_the_single_call(x64, threshold, adaptation, labels, found, centroids, counts,
                                    what):
  want_labels, want_counts, want_centroids = single_call(x64, threshold, adaptation)
  k = len(want_counts)
  assert found == k, what
  assert np.array_equal(labels, want_labels), what
  assert np.array_equal(counts[:k], want_counts), what
  assert_same_bits(centroids[:k], want_centroids, what)
  # nothing past the first k rows / entries is written
  assert (counts[k:] == SENTINEL).all() and (centroids[k:] == SENTINEL).all(), what


GRID = _naive_ref.grid()
# the reference, once per case: (labels, counts, centroids, margin)
GRID_REF = [_naive_ref.naive_walk(x, t, a) for x, t, a in GRID]


def by_pair(j):
  """The grid cases of threshold pair j (a call takes ONE pair) regrouped by d."""
  pairs = {}
  for (x, t, a), ref in zip(GRID, GRID_REF):
    if (t, a) == _naive_ref.GRID_PAIRS[j][:2]:
      pairs.setdefault(x.shape[1], []).append((x, ref))
  return pairs


@pytest.mark.parametrize("j", range(len(_naive_ref.GRID_PAIRS)))
def test_grid_against_the_reference_and_bit_for_bit_against_the_single_call(j):
  threshold, adaptation, _ = _naive_ref.GRID_PAIRS[j]
  for d, cases in by_pair(j).items():
    members = [x for x, _ in cases]
    assert all(ref[3] > 1e-9 for _, ref in cases)  # every decision of every case has a margin
    rc, message, labels, found, centroids, counts = raw_cluster(members, threshold, adaptation)
    assert rc == _lib.SC_OK, message
    for i, (x, ref) in enumerate(cases):
      what = "d=%d n=%d pair=%d" % (d, x.shape[0], j)
      print(what, "centroids", found[i], "margin %.3g" % ref[3])
      assert np.array_equal(labels[i], ref[0]), what
      assert found[i] == len(ref[1]), what
      check_member_is_the_single_call(x, threshold, adaptation, labels[i], found[i], centroids[i],
                                      counts[i], what)
    # the verdict form on the same members
    single, stopped = NaiveClusterer(threshold, adaptation).check_single_batch(members)
    for i, (x, ref) in enumerate(cases):
      want_single, want_stop = _naive_ref.verdict(ref[0])
      assert bool(single[i]) == want_single and stopped[i] == want_stop, (d, x.shape[0], j)
      assert bool(single[i]) == (found[i] == 1)


def test_a_single_column():
  rng = np.random.default_rng(11)
  members = [rng.standard_normal((n, 1)) for n in (1, 2, 65, 300)]
  rc, message, labels, found, centroids, counts = raw_cluster(members, 0.5, None)
  assert rc == _lib.SC_OK, message
  for i, x in enumerate(members):
    check_member_is_the_single_call(x, 0.5, None, labels[i], found[i], centroids[i], counts[i],
                                    "d=1 n=%d" % x.shape[0])
  assert max(found) == 2  # (a cosine of d = 1 is +-1: two centroids at most)


def test_dtypes_strides_and_device_tensors():
  base = so.blobs(130, 48, 3, 4242, noise=0.6)
  wide = np.zeros((130, 100))
  wide[:, ::2][:, :48] = base
  members = [
      base.astype(np.float32),
      base.astype(np.float16),
      torch.from_numpy(base).to(torch.bfloat16),
      wide[:, ::2][:, :48],                               # a column stride
      base[::3],                                          # a row stride
      torch.from_numpy(base).to(torch.float32).cuda(),    # device memory
      torch.from_numpy(base).cuda()[::2],                 # ... strided
      torch.from_numpy(base).to(torch.bfloat16).cuda(),
  ]
  def widened(x):
    if isinstance(x, torch.Tensor):
      return x.to(torch.float64).cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float64)
  rc, message, labels, found, centroids, counts = raw_cluster(members, 0.7, 0.9)
  assert rc == _lib.SC_OK, message
  for i, x in enumerate(members):
    check_member_is_the_single_call(widened(x), 0.7, 0.9, labels[i], found[i], centroids[i],
                                    counts[i], "member %d" % i)
  assert max(found) > 1


def test_golden_reference_output():
  g = golden("fallback.npz")
  x = so.blobs(300, 16, 4, 101, noise=0.6)
  for key, threshold, adaptation in (("t5", 0.5, None), ("t7a9", 0.7, 0.9)):
    labels, centroids, counts = NaiveClusterer(threshold, adaptation).predict_batch(
        [x], return_state=True)
    assert np.array_equal(labels[0], g["naive_" + key]) and labels[0].dtype == np.int64
    assert np.array_equal(counts[0], g["naive_counts_" + key])
    np.testing.assert_allclose(centroids[0], g["naive_cent_" + key], rtol=1e-13, atol=0)


def test_every_row_opens_a_centroid():
  """threshold 0.999 on N(0, I): k = n, the capacity edge of centroids and counts."""
  x = np.random.default_rng(5).standard_normal((65, 64))
  ref_labels, ref_counts, _, margin = _naive_ref.naive_walk(x, 0.999)
  assert margin > 1e-9 and np.array_equal(ref_labels, np.arange(65))
  rc, message, labels, found, centroids, counts = raw_cluster([x], 0.999, None)
  assert rc == _lib.SC_OK, message
  assert found[0] == 65 and np.array_equal(labels[0], np.arange(65))
  assert (counts[0] == 1).all()
  assert_same_bits(centroids[0], x, "the centroids are the rows")
  single, stopped = NaiveClusterer(0.999).check_single_batch([x])
  assert not single[0] and stopped[0] == 1


def test_the_knife_edge():
  """Centroid (1, 0), row (3, 4): the cosine is exactly 0.6.  At threshold 0.6 the row joins
  (not < threshold) without a merge (not > adaptation); at the next double it opens a centroid."""
  x = np.array([[1.0, 0.0], [3.0, 4.0]])
  rc, message, labels, found, centroids, counts = raw_cluster([x], 0.6, None)
  assert rc == _lib.SC_OK, message
  assert found[0] == 1 and labels[0].tolist() == [0, 0] and counts[0][0] == 1
  assert_same_bits(centroids[0][:1], x[:1], "no merge")
  above = np.nextafter(0.6, 1)
  rc, message, labels, found, centroids, counts = raw_cluster([x], above, None)
  assert rc == _lib.SC_OK, message
  assert found[0] == 2 and labels[0].tolist() == [0, 1] and counts[0][:2].tolist() == [1, 1]
  for threshold, want in ((0.6, (True, 2)), (above, (False, 1))):
    single, stopped = NaiveClusterer(threshold).check_single_batch([x])
    assert (bool(single[0]), int(stopped[0])) == want
    check_member_is_the_single_call(x, threshold, None, *[v[0] for v in raw_cluster(
        [x], threshold, None)[2:]], "knife edge %r" % threshold)


def test_zero_and_nan_rows_are_the_single_calls():
  zero = so.blobs(40, 24, 2, 77, noise=0.6)
  zero[0] = 0.0
  zero[13] = 0.0
  nan = so.blobs(40, 24, 2, 78, noise=0.6)
  nan[7, 3] = np.nan
  nan[20] = np.inf
  rc, message, labels, found, centroids, counts = raw_cluster([zero, nan], 0.5, None)
  assert rc == _lib.SC_OK, message
  for i, x in enumerate((zero, nan)):
    want_labels, want_counts, want_centroids = single_call(x, 0.5, None)
    assert found[i] == len(want_counts) and np.array_equal(labels[i], want_labels)
    assert np.array_equal(counts[i][:found[i]], want_counts)
    assert_same_bits(centroids[i][:found[i]], want_centroids, "member %d" % i)  # (NaN bits too)
    single, stopped = NaiveClusterer(0.5).check_single_batch([x])
    assert (bool(single[0]), int(stopped[0])) == _naive_ref.verdict(want_labels)


def test_a_member_does_not_depend_on_the_call_or_the_waves():
  probe = so.blobs(150, 64, 4, 900, noise=0.6)
  others = [so.blobs(20 + 7 * i, 64, 3, 901 + i, noise=0.6) for i in range(39)]
  crowd = others[:20] + [probe] + others[20:]
  alone = raw_cluster([probe], 0.5, None)
  among = raw_cluster(crowd, 0.5, None)
  handle = _lib.default_handle()
  # the longest member (286 rows) needs about 2 * 286 * 64 * 8 = 0.3 MB: 512 KB a wave makes
  # >= 3 waves of the 40 members (3.1 MB of rows alone)
  assert sum(x.shape[0] for x in crowd) * 64 * 8 > 3 * (512 << 10)
  handle.check(handle.lib.sc_set_reduce_wave_bytes(handle.raw, 512 << 10))
  try:
    waves = raw_cluster(crowd, 0.5, None)
    single_w, stopped_w = NaiveClusterer(0.5).check_single_batch(crowd)
  finally:
    handle.check(handle.lib.sc_set_reduce_wave_bytes(handle.raw, 0))
  single_1, stopped_1 = NaiveClusterer(0.5).check_single_batch(crowd)
  assert np.array_equal(single_w, single_1) and np.array_equal(stopped_w, stopped_1)
  for run in (alone, among, waves):
    assert run[0] == _lib.SC_OK, run[1]
  assert alone[3][0] > 1
  for run, at in ((among, 20), (waves, 20)):
    assert np.array_equal(run[2][at], alone[2][0]) and run[3][at] == alone[3][0]
    assert np.array_equal(run[5][at], alone[5][0])
    assert_same_bits(run[4][at], alone[4][0], "centroids, sentinel rows included")
  for i in range(len(crowd)):  # the small waves change nobody
    assert np.array_equal(waves[2][i], among[2][i]) and np.array_equal(waves[5][i], among[5][i])
    assert_same_bits(waves[4][i], among[4][i], "member %d" % i)
  # without the state outputs: the same labels
  plain = raw_cluster(crowd, 0.5, None, want_state=False)
  assert plain[0] == _lib.SC_OK
  assert all(np.array_equal(a, b) for a, b in zip(plain[2], among[2]))
  assert all((c == SENTINEL).all() for c in plain[4])


def test_a_call_that_fails_validation_writes_nothing():
  good = so.blobs(30, 16, 2, 1, noise=0.6)
  for members, threshold, adaptation, needle in (
      ([good, so.blobs(30, 17, 2, 2)], 0.5, None, "same d"),
      ([good, good], 0.7, 0.5, "adaptation_threshold cannot be smaller"),
  ):
    rc, message, labels, found, centroids, counts = raw_cluster(members, threshold, adaptation)
    assert rc == _lib.SC_ERR_INVALID and needle in message, message
    assert (found == SENTINEL).all()
    assert all((l == SENTINEL).all() for l in labels)
    assert all((c == SENTINEL).all() for c in centroids + counts)
  handle = _lib.default_handle()
  src = _dlpack.describe(good, lambda: handle)
  assert handle.lib.sc_batch_naive_cluster(handle.raw, (_lib.ScArray * 1)(src.array), 1, 0.5, 0.5,
                                           None, None, None, None) == _lib.SC_ERR_INVALID
  assert handle.lib.sc_batch_naive_check(handle.raw, (_lib.ScArray * 1)(src.array), 1, 0.5, 0.5,
                                         None, None) == _lib.SC_ERR_INVALID
  src.release()
  # the handle is usable afterwards
  assert NaiveClusterer(0.5).predict_batch([good])[0].shape == (30,)
