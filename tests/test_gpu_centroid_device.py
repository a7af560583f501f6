"""GPU: centroids and labels where the caller wants them.  `utils.get_cluster_centroids` /
`get_cluster_centroids_batch` on described arrays (csrc/centroids.hip) against `_centroid_ref` on
the widened float64 input, bit for bit, in every output dtype, into views inside sentinel-filled
tensors; every error of the entry, with the outputs untouched; `out=` of the predict entries
(`sc_labels_egress`, csrc/egress.hip); INTEGRATION.md's example."""

import ctypes
import os
import re

import numpy as np
import pytest
# (at module level on purpose: PyTorch has to be in the process before the library is loaded,
#  so that both use one HIP runtime -- INTEGRATION.md section 6)
import torch

import _centroid_ref as cr
import _narrow_ref as nr
import test_gpu_egress as eg

import spectralcluster_amd as sca
from spectralcluster_amd import _dlpack
from spectralcluster_amd import _lib
from spectralcluster_amd import utils

pytestmark = pytest.mark.gpu

FLOAT, INT = eg.FLOAT, eg.INT
NS = [1, 2, 63, 64, 65, 255, 256, 257, 1000]
DS = [1, 3, 16, 17, 255, 256, 257, 600]
# the cross of the extremes and a diagonal
SHAPES = sorted(set([(1, 1), (1, 600), (1000, 1), (1000, 600)] + list(zip(NS, DS + [600]))))
PATTERNS = ("blocks", "modulo", "permutation", "one_of_several", "unused", "negative")


def labels_of(pattern, n, k, rng):
  base = np.arange(n) % k
  if pattern == "blocks":
    return np.sort(base)
  if pattern == "modulo":
    return base
  if pattern == "permutation":
    return rng.permutation(base)
  if pattern == "one_of_several":  # every row in the last of k clusters: k - 1 rows of NaN
    return np.full(n, k - 1)
  lab = rng.permutation(base)
  if pattern == "unused":  # label 0 of range(k) is carried by no row; k - 1 stays the largest
    lab[lab == 0] = k - 1
    return lab
  lab[int(rng.integers(0, n))] = -1 - int(rng.integers(0, 5))  # "negative"
  return lab


def embeddings(n, d, dtype, seed):
  """Three decades of dynamic range per column, in `dtype` (a torch CPU tensor)."""
  rng = np.random.default_rng(seed)
  return torch.from_numpy(cr.wide_range_input(rng, n, d)).to(FLOAT[dtype])


def bits_of(t, dtype):
  return t.detach().cpu().contiguous().view(INT[dtype][0]).numpy().view(nr.BITS[dtype])


def check(x, labels, dtype_out="float64", what=""):
  """One call with a new device output of exactly k rows; returns k."""
  lab_host = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
  wide = x.detach().cpu().double().numpy() if isinstance(x, torch.Tensor) else np.asarray(
      x, dtype=np.float64)
  want = cr.centroid_bits(wide, lab_host, dtype_out)
  k, d = want.shape
  out = torch.full((max(k, 1), d), 7.0, dtype=FLOAT[dtype_out], device="cuda")[:k]
  got = utils.get_cluster_centroids(x, labels, out=out)
  assert tuple(got.shape) == (k, d), what
  nr.assert_same_bits(bits_of(out, dtype_out), want, dtype_out, what)
  return k


@pytest.mark.parametrize("n,d", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_every_label_pattern_and_cluster_count(handle, n, d):
  rng = np.random.default_rng(1000 * n + d)
  x = embeddings(n, d, "float64", n + d).cuda()
  done = set()
  for k in (1, 2, 7, 64, n):
    k = min(k, n)
    for pattern in PATTERNS:
      if (pattern in ("one_of_several", "unused") and k < 2) or (k, pattern) in done:
        continue
      done.add((k, pattern))
      lab = labels_of(pattern, n, k, rng)
      check(x, torch.from_numpy(lab).cuda(), what="%dx%d k=%d %s" % (n, d, k, pattern))


SOURCE_VIEWS = {
    "contiguous": lambda n, d: ((n, d), lambda b: b),
    "pitched": lambda n, d: ((n + 2, d + 24), lambda b: b[1:1 + n, 8:8 + d]),
    "pitched_offset_1": lambda n, d: ((n + 2, d + 24), lambda b: b[1:1 + n, 9:9 + d]),
    "transposed": lambda n, d: ((d, n), lambda b: b.T),
    "step_2": lambda n, d: ((2 * n, 2 * d), lambda b: b[::2, 1::2]),
}


@pytest.mark.parametrize("device", ["cuda", "cpu"])
@pytest.mark.parametrize("dtype", nr.DTYPES)
def test_sources_of_every_dtype_layout_and_location(handle, dtype, device):
  for n, d, k in ((257, 17, 7), (65, 255, 2)):
    values = embeddings(n, d, dtype, 17 * n)
    lab = torch.from_numpy(np.random.default_rng(n).integers(0, k, size=n)).cuda()
    for name, make in SOURCE_VIEWS.items():
      shape, view = make(n, d)
      big = torch.zeros(shape, dtype=FLOAT[dtype], device=device)
      src = view(big)
      src.copy_(values)
      for out_dtype in ("float64", "float32") if name != "contiguous" else nr.DTYPES:
        check(src, lab, out_dtype, "%s %s %s %dx%d -> %s" % (dtype, device, name, n, d, out_dtype))
    if device == "cpu" and dtype != "bfloat16":  # ... and as a NumPy view
      big = np.zeros((n + 2, 2 * d + 3), dtype=dtype)
      src = big[1:1 + n, 3::2]
      src[...] = values.numpy()
      check(src, lab, "float64", "numpy view " + dtype)


@pytest.mark.parametrize("device", ["cuda", "cpu"])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.float64, torch.float32])
def test_labels_of_every_dtype_layout_and_location(handle, dtype, device):
  n, d, k = 257, 17, 7
  x = embeddings(n, d, "float32", 5).cuda()
  lab = np.random.default_rng(11).integers(0, k, size=n)
  lab[5] = -2
  contiguous = torch.from_numpy(lab).to(dtype).to(device)
  stepped = torch.full((2 * n + 1,), 3, dtype=dtype, device=device)[1::2]
  stepped.copy_(contiguous)
  for labels in (contiguous, stepped):
    assert check(x, labels, "float64", str(dtype)) == k
  if device == "cpu":
    assert check(x, contiguous.numpy()[::1], "float32") == k
    assert check(x, stepped.numpy(), "float32") == k
    assert check(x.cpu().numpy(), lab.astype(np.int16), "float32") == k  # promoted on the host
  # a broadcast label array: every row in cluster 2
  assert check(x, torch.full((1,), 2, dtype=dtype, device=device).expand(n), "float64") == 3


@pytest.mark.parametrize("dtype", nr.DTYPES)
def test_destinations_of_every_layout_and_only_the_first_k_rows_are_written(handle, dtype):
  n, d, k, room = 200, 33, 5, 7  # two rows more than clusters
  x = embeddings(n, d, "float64", 9)
  lab = np.random.default_rng(2).integers(0, k, size=n)
  lab[lab == 3] = 1  # (a NaN row among them)
  want = cr.centroid_bits(x.numpy(), lab, dtype)
  itype, sentinel = INT[dtype]
  xd, ld = x.cuda(), torch.from_numpy(lab).cuda()
  for name, (shape, view) in eg.destinations(room, d).items():
    for device in ("cuda", "cpu"):
      big = torch.full(shape, sentinel, dtype=itype, device=device)
      dest = view(big.view(FLOAT[dtype]))
      assert tuple(dest.shape) == (room, d)
      got = utils.get_cluster_centroids(xd, ld, out=dest)
      what = "%s %s -> %s" % (dtype, device, name)
      assert tuple(got.shape) == (k, d) and got.data_ptr() == dest.data_ptr(), what
      after = big.cpu().numpy().view(nr.BITS[dtype])
      inside = view(after)
      nr.assert_same_bits(np.ascontiguousarray(inside[:k]), want, dtype, what)
      inside[:k] = 0
      untouched = np.full(shape, sentinel, dtype=nr.BITS[dtype])
      view(untouched)[:k] = 0
      assert np.array_equal(after, untouched), what + ": memory outside the first k rows was written"
  # NumPy destinations
  for ndtype in ("float64", "float32", "float16"):
    big = np.full((room + 2, 2 * d + 8), -7.0, dtype=ndtype)
    dest = big[1:1 + room, 3:3 + 2 * d:2]
    got = utils.get_cluster_centroids(xd, ld, out=dest)
    assert got.shape == (k, d) and got.base is big
    nr.assert_same_bits(np.ascontiguousarray(got).view(nr.BITS[ndtype]),
                        cr.centroid_bits(x.numpy(), lab, ndtype), ndtype, "numpy " + ndtype)
    dest[:k] = -7.0
    assert (big == -7.0).all()


def test_without_out_the_result_is_a_new_host_float64_array(handle):
  x = embeddings(130, 20, "float16", 4)
  lab = np.arange(130) % 6
  want = cr.centroids(x.double().numpy(), lab)
  for e, l in ((x.cuda(), torch.from_numpy(lab).cuda()), (x.cuda(), lab), (x.numpy(), torch.from_numpy(lab)),
               (x, torch.from_numpy(lab).int().cuda())):
    got = utils.get_cluster_centroids(e, l)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
  # ... and today's path on the same values gives the same bits
  today = utils.get_cluster_centroids(x.double().numpy(), lab)
  assert np.array_equal(today.view(np.uint64), want.view(np.uint64))
  # every label negative: no cluster
  got = utils.get_cluster_centroids(x.cuda(), torch.full((130,), -1, device="cuda"))
  assert got.shape == (0, 20)


def sentinel_outputs(count, rows, d):
  return [torch.full((rows, d), 7.0, dtype=torch.float32, device="cuda") for _ in range(count)]


def test_every_error_names_the_member_and_writes_nothing(handle):
  n, d = 50, 6
  x = embeddings(n, d, "float32", 1).cuda()
  good = torch.arange(n, device="cuda") % 3

  def refused(match, xs, labels, outs):
    with pytest.raises(ValueError, match=match):
      utils.get_cluster_centroids_batch(xs, labels, outs)
    torch.cuda.synchronize()
    for o in outs:
      assert (o == 7.0).all(), match

  outs = sentinel_outputs(2, 3, d)
  refused("labels of member 1 must hold 50 entries, not 49", [x, x], [good, good[:49]], outs)
  fraction = good.double()
  fraction[7] = 0.5
  refused("labels of member 1.*integral", [x, x], [good, fraction], outs)
  for value in (float("nan"), float("inf"), -float("inf")):
    bad = good.float()
    bad[n - 1] = value
    refused("labels of member 1.*finite", [x, x], [good, bad], outs)
  big = good.clone()
  big[3] = 2**31
  refused("labels of member 0.*2\\^31", [x, x], [big, good], outs)
  big[3] = 2**31 - 1
  refused("labels of member 0.*2\\^31", [x, x], [big, good], outs)
  refused("labels of member 1", [x, x], [good, (good.double() + 2.0**40)], outs)
  refused("out of member 1 must be .*6", [x, x], [good, good],
          [outs[0], torch.full((3, 7), 7.0, device="cuda")[:, :5]])
  four = good.clone()
  four[n - 1] = 3
  refused("out of member 1 has 3 rows, the labels make 4 clusters", [x, x], [good, four], outs)
  # a device out that overlaps a device source of the call, another member's included
  pool = torch.full((n + 3, d), 7.0, dtype=torch.float32, device="cuda")
  pool_x = pool[3:]
  with pytest.raises(ValueError, match="out of member 0 overlaps"):
    utils.get_cluster_centroids_batch([x, pool_x], [good, good], [pool[1:4], outs[1]])
  lab_pool = torch.zeros(n + 8, dtype=torch.int64, device="cuda")
  with pytest.raises(ValueError, match="out of member 1 overlaps"):
    utils.get_cluster_centroids_batch(
        [x, x.double()], [lab_pool[8:], good],
        [outs[0], lab_pool.view(torch.float64)[:3 * d].view(3, d)])  # entries 0 .. 17
  torch.cuda.synchronize()
  assert (pool == 7.0).all() and (outs[0] == 7.0).all() and (outs[1] == 7.0).all()
  # ... the rows just before the source are fine
  got = utils.get_cluster_centroids(pool_x, good, out=pool[:3])
  assert tuple(got.shape) == (3, d)


def test_the_library_makes_every_check_itself(handle):
  """The entry on descriptors of one's own: what the Python side refuses first is refused here."""
  n, d = 20, 4
  x = torch.ones(n, d, dtype=torch.float64, device="cuda")
  lab = (torch.arange(n, device="cuda") % 3)
  out = torch.full((3, d), 7.0, dtype=torch.float64, device="cuda")
  lib = handle.lib

  def call(outs=True, **changes):
    xa = _lib.ScArray(x.data_ptr(), _lib.SC_DTYPE_F64, _lib.SC_MEM_DEVICE, n, d, d, 1)
    la = _lib.ScArray(lab.data_ptr(), _lib.SC_DTYPE_I64, _lib.SC_MEM_DEVICE, 1, n, 0, 1)
    oa = _lib.ScArray(out.data_ptr(), _lib.SC_DTYPE_F64, _lib.SC_MEM_DEVICE, 3, d, d, 1)
    arrays = {"x": xa, "l": la, "o": oa}
    for key, value in changes.items():
      setattr(arrays[key[0]], key[2:], value)
    ks = (ctypes.c_int32 * 1)(-5)
    rc = lib.sc_cluster_centroids_arrays(handle.raw, ctypes.byref(xa), ctypes.byref(la), 1,
                                         ctypes.byref(oa) if outs else None, ks)
    return rc, ks[0]

  assert call(outs=False) == (_lib.SC_OK, 3)
  assert (out.cpu() == 7.0).all()
  assert call() == (_lib.SC_OK, 3)
  assert (out.cpu() == 1.0).all()
  out.fill_(7.0)
  torch.cuda.synchronize()
  for bad in (dict(l_cols=n - 1), dict(l_rows=2), dict(l_dtype=_lib.SC_DTYPE_F16), dict(l_dtype=9),
              dict(l_col_stride=-1), dict(l_data=None), dict(l_location=3),
              dict(l_data=np.zeros(n, dtype=np.int64).ctypes.data),  # host memory called device
              dict(o_cols=d - 1), dict(o_rows=2), dict(o_dtype=_lib.SC_DTYPE_I64),
              dict(o_row_stride=d - 1), dict(o_col_stride=-1), dict(o_data=x.data_ptr() + 8),
              dict(o_data=lab.data_ptr()), dict(x_dtype=_lib.SC_DTYPE_I32), dict(x_rows=0)):
    rc, _ = call(**bad)
    assert rc == _lib.SC_ERR_INVALID, bad
    assert "member 0" in handle.last_error(), (bad, handle.last_error())
  assert (out.cpu() == 7.0).all()
  # the label dtypes are answered as any unknown dtype by the entries that take no labels
  xa = _lib.ScArray(x.data_ptr(), _lib.SC_DTYPE_I64, _lib.SC_MEM_DEVICE, n, d, d, 1)
  sq = _lib.ScArray(x.data_ptr(), _lib.SC_DTYPE_I32, _lib.SC_MEM_DEVICE, 4, 4, 4, 1)
  fa = _lib.ScArray(out.data_ptr(), _lib.SC_DTYPE_F64, _lib.SC_MEM_DEVICE, 4, 4, 4, 1)
  host = np.zeros((n, n))
  for rc in (lib.sc_set_embeddings_array(handle.raw, ctypes.byref(xa)),
             lib.sc_set_affinity_array(handle.raw, ctypes.byref(sq)),
             lib.sc_stage_ingest(handle.raw, ctypes.byref(xa), _lib.as_double_p(host)),
             lib.sc_stage_ingest_columns(handle.raw, ctypes.byref(xa), _lib.as_double_p(host)),
             lib.sc_stage_affinity_array(handle.raw, ctypes.byref(xa), ctypes.byref(fa)),
             lib.sc_stage_laplacian_array(handle.raw, 2, ctypes.byref(sq), ctypes.byref(fa)),
             lib.sc_stage_egress(handle.raw, _lib.as_double_p(host), 4, 4, 0, ctypes.byref(sq)),
             lib.sc_set_constraint_array(handle.raw, ctypes.byref(sq))):
    assert rc == _lib.SC_ERR_INVALID
    assert "unknown dtype" in handle.last_error()


# ------------------------------------------------------------------------------- batch
def members(count, seed):
  """Mixed n in [1, 300], dtype, location and k; d = 24."""
  rng = np.random.default_rng(seed)
  xs, ls = [], []
  for i in range(count):
    n = int(rng.integers(1, 301)) if i else 300
    k = int(rng.integers(1, min(n, 9) + 1))
    dtype = nr.DTYPES[i % 4]
    x = embeddings(n, 24, dtype, seed + i)
    lab = rng.permutation(np.arange(n) % k)
    if i % 5 == 4 and n > 2:
      lab[0] = -1
    where = i % 3
    xs.append(x.cuda() if where != 1 else (x if dtype == "bfloat16" or i % 2 else x.numpy()))
    lt = torch.from_numpy(lab).to(torch.int32 if i % 2 else torch.int64)
    ls.append(lt.cuda() if where == 0 else (lt if where == 1 else lt.numpy()))
  return xs, ls


@pytest.mark.parametrize("count", [1, 2, 65, 200])
def test_a_batch_equals_its_members_one_by_one(handle, count):
  xs, ls = members(count, 100 + count)
  out_dtypes = [nr.DTYPES[(i // 2) % 4] for i in range(count)]
  rooms = [12 for _ in range(count)]
  outs = [torch.full((rooms[i], 24), 7.0, dtype=FLOAT[out_dtypes[i]],
                     device="cuda" if i % 2 else "cpu") for i in range(count)]
  got = utils.get_cluster_centroids_batch(xs, ls, outs)
  assert len(got) == count
  for i in range(count):
    one = torch.full((rooms[i], 24), 7.0, dtype=FLOAT[out_dtypes[i]], device="cuda")
    single = utils.get_cluster_centroids(xs[i], ls[i], out=one)
    k = single.shape[0]
    assert tuple(got[i].shape) == (k, 24) and got[i].data_ptr() == outs[i].data_ptr(), i
    nr.assert_same_bits(bits_of(outs[i], out_dtypes[i]), bits_of(one, out_dtypes[i]),
                        out_dtypes[i], "member %d" % i)
    assert (outs[i][k:] == 7.0).all() and (one[k:] == 7.0).all()
  # ... and without out: new host float64 arrays of exactly k rows
  plain = utils.get_cluster_centroids_batch(xs[:3], ls[:3])
  for i, p in enumerate(plain):
    wide = xs[i].double().cpu().numpy() if isinstance(xs[i], torch.Tensor) else xs[i].astype(np.float64)
    lab = ls[i].cpu().numpy() if isinstance(ls[i], torch.Tensor) else ls[i]
    assert np.array_equal(p.view(np.uint64), cr.centroids(wide, lab).view(np.uint64))


def test_one_member_with_every_row_its_own_cluster_among_many_small_ones(handle):
  """130 members bound the launch at 64 workgroups a member: the 24000 outputs of the member with
  k = n = 1000 go round them, before, between and after members of a few clusters."""
  xs, ls = members(130, 31)
  for at in (0, 64, 129):
    xs[at] = embeddings(1000, 24, "float32", 900 + at).cuda()
    ls[at] = torch.randperm(1000, generator=torch.Generator().manual_seed(at)).cuda()
  outs = [torch.full((1000 if i in (0, 64, 129) else 9, 24), 7.0, dtype=torch.float64,
                     device="cuda") for i in range(130)]
  got = utils.get_cluster_centroids_batch(xs, ls, outs)
  for i in (0, 1, 63, 64, 65, 128, 129):
    wide = xs[i].double().cpu().numpy() if isinstance(xs[i], torch.Tensor) else xs[i].astype(np.float64)
    lab = ls[i].cpu().numpy() if isinstance(ls[i], torch.Tensor) else ls[i]
    want = cr.centroid_bits(wide, lab, "float64")
    assert tuple(got[i].shape) == want.shape, i
    nr.assert_same_bits(bits_of(got[i], "float64"), want, "float64", "member %d" % i)
    assert (outs[i][want.shape[0]:] == 7.0).all()


def test_an_overlapping_out_and_source_pair_of_a_batch_raises(handle):
  xs, ls = members(4, 7)
  flat = torch.full((4 * 12 * 24 + 300 * 24,), 7.0, dtype=torch.float64, device="cuda")
  source = flat[4 * 12 * 24 - 8:4 * 12 * 24 - 8 + 300 * 24].view(300, 24)  # eight elements early
  source.copy_(xs[0].double())
  outs = [flat[i * 12 * 24:(i + 1) * 12 * 24].view(12, 24) for i in range(4)]
  before = flat.clone()
  with pytest.raises(ValueError, match="out of member 3 overlaps"):
    utils.get_cluster_centroids_batch([source] + xs[1:], ls, outs)
  assert torch.equal(flat, before)


# -------------------------------------------------------------------------- labels out
def blobs(n, d, speakers, seed):
  rng = np.random.default_rng(seed)
  centres = rng.standard_normal((speakers, d)) * 4.0
  return (centres[np.arange(n) % speakers] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)


def label_destinations(n):
  """name -> (dtype, device, length of the buffer, the view of n entries)."""
  dests = {}
  for dtype in (torch.int64, torch.int32):
    for device in ("cuda", "cpu"):
      dests["%s %s contiguous" % (dtype, device)] = (dtype, device, n + 9, lambda b, n=n: b[5:5 + n])
      dests["%s %s step 2" % (dtype, device)] = (dtype, device, 2 * n + 9,
                                                 lambda b, n=n: b[3:3 + 2 * n:2])
  return dests


SENTINEL = -77


def check_labels_out(call, n, want):
  want = np.asarray(want)
  assert np.array_equal(want, want.astype(np.int64))
  for name, (dtype, device, length, view) in label_destinations(n).items():
    big = torch.full((length,), SENTINEL, dtype=dtype, device=device)
    out = view(big)
    got = call(out)
    assert got is out, name
    after = big.cpu().numpy()
    assert np.array_equal(view(after), want.astype(after.dtype)), name
    view(after)[...] = SENTINEL
    assert (after == SENTINEL).all(), name + ": written outside the view"
  # NumPy destinations
  for ndtype in (np.int64, np.int32):
    big = np.full(2 * n + 2, SENTINEL, dtype=ndtype)
    for out in (big[1:1 + n], big[1:1 + 2 * n:2]):
      big[...] = SENTINEL
      assert call(out) is out
      assert np.array_equal(out, want.astype(ndtype))
      out[...] = SENTINEL
      assert (big == SENTINEL).all()


def grouped_clusterer():
  """A refinement sequence the grouped front covers: in a batch, up to 128 rows take the short
  route (2) and more than 128 the lockstep route (1)."""
  options = sca.RefinementOptions(gaussian_blur_sigma=0, p_percentile=0.2,
                                  refinement_sequence=sca.ICASSP2018_REFINEMENT_SEQUENCE)
  return sca.SpectralClusterer(refinement_options=options, stop_eigenvalue=0.01, min_clusters=2,
                               max_clusters=6)


@pytest.mark.parametrize("n,route", [(40, 2), (200, 1)], ids=["40-short", "200-lockstep"])
def test_predict_writes_its_labels_into_out(handle, n, route):
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=6)
  x = torch.from_numpy(blobs(n, 16, 3, n)).cuda()
  want = c.predict(x)
  assert want.dtype == np.int64 and len(set(want.tolist())) == 3
  check_labels_out(lambda out: c.predict(x, out=out), n, want)
  # ... and through the batch call, on the route of this size, into every destination
  g = grouped_clusterer()
  want = g.predict_batch([x])[0]
  assert g.last_batch_routes == [route]

  def batch(out):
    got = g.predict_batch([x], out=[out])[0]
    assert g.last_batch_routes == [route]
    return got
  check_labels_out(batch, n, want)


def test_the_float64_labels_of_a_size_reduced_utterance_are_converted_exactly(handle):
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=6, max_spectral_size=32)
  x = torch.from_numpy(blobs(120, 16, 3, 5)).cuda()
  want = c.predict(x)
  assert want.dtype == np.float64 and len(set(want.tolist())) == 3
  check_labels_out(lambda out: c.predict(x, out=out), 120, want)


def test_predict_batch_writes_views_of_one_flat_tensor(handle):
  c = grouped_clusterer()  # (200 and 129 rows take the lockstep route)
  sizes = [40, 200, 129, 17, 64]
  xs = [torch.from_numpy(blobs(n, 16, 2 + i % 3, 50 + i)) for i, n in enumerate(sizes)]
  xs = [x.cuda() if i % 2 == 0 else x.numpy() for i, x in enumerate(xs)]
  want = c.predict_batch(xs)
  assert set(c.last_batch_routes) == {1, 2}
  for dtype in (torch.int64, torch.int32):
    flat = torch.full((sum(sizes) + 2 * len(sizes) + 1,), SENTINEL, dtype=dtype, device="cuda")
    at, outs = 1, []
    for n in sizes:
      outs.append(flat[at:at + n])
      at += n + 2
    got = c.predict_batch(xs, out=outs)
    assert len(got) == len(outs) and all(g is o for g, o in zip(got, outs))
    after = flat.cpu().numpy()
    at = 1
    for n, w in zip(sizes, want):
      assert np.array_equal(after[at:at + n], w)
      after[at:at + n] = SENTINEL
      at += n + 2
    assert (after == SENTINEL).all()
  # a mixed list: device and host destinations, both widths, a step
  host = np.full(2 * sizes[1], SENTINEL, dtype=np.int32)
  outs = [torch.empty(sizes[0], dtype=torch.int32, device="cuda"), host[::2],
          torch.empty(sizes[2], dtype=torch.int64), torch.empty(2 * sizes[3], dtype=torch.int64,
                                                               device="cuda")[::2],
          np.empty(sizes[4], dtype=np.int64)]
  got = c.predict_batch(xs, out=outs)
  for g, o, w in zip(got, outs, want):
    assert g is o
    assert np.array_equal(o.cpu().numpy() if isinstance(o, torch.Tensor) else o, w)
  assert (host[1::2] == SENTINEL).all()
  # a bad entry anywhere: nothing runs, nothing is written
  outs[3] = torch.empty(sizes[3], dtype=torch.float32, device="cuda")
  outs[0].fill_(SENTINEL)
  with pytest.raises(TypeError, match="out 3 must be int64 or int32"):
    c.predict_batch(xs, out=outs)
  assert (outs[0].cpu() == SENTINEL).all()


def test_predict_affinity_writes_its_labels_into_out(handle):
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=6)
  x = blobs(40, 16, 3, 8)
  a = utils.compute_affinity_matrix(x, out=torch.empty(40, 40, dtype=torch.float32, device="cuda"))
  want = c.predict_affinity(a)
  assert len(set(want.tolist())) == 3
  check_labels_out(lambda out: c.predict_affinity(a, out=out), 40, want)
  out = torch.empty(40, dtype=torch.int32, device="cuda")
  got = c.predict_affinity_batch([a, a.cpu().numpy()], out=[out, np.empty(40, dtype=np.int64)])
  assert got[0] is out and np.array_equal(out.cpu().numpy(), want) and np.array_equal(got[1], want)


def test_a_user_kmeans_function_and_autotune_leave_through_the_same_egress(handle):
  x = torch.from_numpy(blobs(90, 16, 3, 21)).cuda()

  def tail(spectral_embeddings, n_clusters, custom_dist, max_iter):
    return sca.custom_distance_kmeans.run_kmeans(spectral_embeddings, n_clusters, custom_dist,
                                                 max_iter)
  def user():
    return sca.SpectralClusterer(min_clusters=2, max_clusters=6, post_eigen_cluster_function=tail)

  def tuned():
    refinement_options = sca.RefinementOptions(
        thresholding_type=sca.ThresholdType.Percentile,
        refinement_sequence=[sca.RefinementName.RowWiseThreshold, sca.RefinementName.Symmetrize])
    return sca.SpectralClusterer(
        min_clusters=2, max_clusters=6, refinement_options=refinement_options,
        autotune=sca.AutoTune(p_percentile_min=0.6, p_percentile_max=0.95, init_search_step=0.05,
                              search_level=1))
  # (a new clusterer per call: an AutoTune search leaves its object narrowed for the next one)
  for make in (user, tuned):
    want = make().predict(x)
    out = torch.full((90,), SENTINEL, dtype=torch.int32, device="cuda")
    assert make().predict(x, out=out) is out
    assert np.array_equal(out.cpu().numpy(), want)
    want = make().predict_batch([x, x])
    outs = [torch.full((90,), SENTINEL, dtype=torch.int64, device="cuda"), np.empty(90, dtype=np.int32)]
    got = make().predict_batch([x, x], out=outs)
    assert got[0] is outs[0] and np.array_equal(outs[0].cpu().numpy(), want[0])
    assert got[1] is outs[1] and np.array_equal(outs[1], want[1])


# ----------------------------------------------------------------------- documentation
def test_the_example_of_the_integration_guide(handle):
  """INTEGRATION.md section 8, as written, against the host path."""
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = open(os.path.join(root, "INTEGRATION.md")).read()
  section = text[text.index("## 8. Labels and centroids on device tensors"):]
  code = re.search(r"```python\n(.*?)```", section, flags=re.S).group(1)
  assert ".cpu()" not in code
  scope = {}
  exec(compile(code, "INTEGRATION.md section 8", "exec"), scope)
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=6)
  x = torch.from_numpy(blobs(150, 24, 4, 3)).to(torch.float16).cuda()
  labels, means = scope["speakers"](c, x, 6)
  assert labels.is_cuda and means.is_cuda and means.dtype == torch.float16
  want_labels = c.predict(x.cpu().numpy())
  assert np.array_equal(labels.cpu().numpy(), want_labels)
  k = int(want_labels.max()) + 1
  assert k == 4 and tuple(means.shape) == (k, 24)
  want = utils.get_cluster_centroids(x.cpu().double().numpy(), want_labels)
  nr.assert_same_bits(bits_of(means, "float16"), nr.narrow_bits(want, "float16"), "float16",
                      "speaker means")
