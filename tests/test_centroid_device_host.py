"""Labels and centroids where the caller wants them, the part that needs no GPU: the reference of
the GPU tests (`_centroid_ref`) pinned against the oracle and `np.mean`, on an input where another
order of the adds changes bits; label arrays and every `out` described as they lie or refused
before any library call; the routing rule of `get_cluster_centroids`; one library call per batch."""

import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import _centroid_ref as cr

from spectralcluster_amd import _batch
from spectralcluster_amd import _dlpack
from spectralcluster_amd import _lib
from spectralcluster_amd import utils
import spectralcluster_amd as sca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import spectral_oracle  # noqa: E402


# ------------------------------------------------------------------------- the reference
def cases():
  rng = np.random.default_rng(20261021)
  out = []
  for n, d, k in ((1, 1, 1), (40, 3, 4), (257, 17, 7), (300, 2, 300), (500, 16, 2)):
    x = rng.standard_normal((n, d))
    out.append(("normal %dx%d k=%d" % (n, d, k), x, rng.permutation(n) % k))
  x = cr.wide_range_input(rng, 600, 8)
  out.append(("wide range", x, rng.integers(0, 3, size=600)))
  return out


CASES = cases()


@pytest.mark.parametrize("name,x,labels", CASES, ids=[c[0] for c in CASES])
def test_the_reference_is_the_oracle_and_numpy_mean_bit_for_bit(name, x, labels):
  got = cr.centroids(x, labels)
  want = spectral_oracle.get_cluster_centroids(x, labels)
  assert got.dtype == want.dtype == np.float64 and got.shape == want.shape
  assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
  for c in range(int(labels.max()) + 1):
    row = np.mean(x[labels == c], axis=0)
    assert np.array_equal(got[c].view(np.uint64), row.view(np.uint64)), c


def test_another_order_of_the_adds_changes_bits_on_the_wide_range_input():
  _, x, labels = CASES[-1]
  want = cr.centroids(x, labels)
  # reversed: the same rows, added from the last to the first
  rev = cr.centroids(x[::-1], labels[::-1])
  assert not np.array_equal(rev.view(np.uint64), want.view(np.uint64))
  # pairwise: halves summed separately
  pair = np.empty_like(want)
  for c in range(want.shape[0]):
    rows = x[labels == c]
    half = rows.shape[0] // 2
    lo, hi = np.zeros(x.shape[1]), np.zeros(x.shape[1])
    for r in rows[:half]:
      lo = lo + r
    for r in rows[half:]:
      hi = hi + r
    pair[c] = (lo + hi) / rows.shape[0]
  assert not np.array_equal(pair.view(np.uint64), want.view(np.uint64))
  np.testing.assert_allclose(pair, want, rtol=1e-10)
  np.testing.assert_allclose(rev, want, rtol=1e-10)


def test_the_label_patterns_of_the_gpu_tests_are_what_they_say():
  import test_gpu_centroid_device as gpu_tests
  rng = np.random.default_rng(3)
  for n, k in ((64, 7), (257, 64), (10, 10), (2, 2)):
    lab = gpu_tests.labels_of("unused", n, k, rng)
    assert lab.max() == k - 1 and 0 not in lab and lab.min() >= 0
    assert (gpu_tests.labels_of("negative", n, k, rng) < 0).sum() == 1
    assert set(gpu_tests.labels_of("one_of_several", n, k, rng).tolist()) == {k - 1}
    assert np.array_equal(np.bincount(gpu_tests.labels_of("permutation", n, k, rng)),
                          np.bincount(gpu_tests.labels_of("blocks", n, k, rng)))


def test_negative_labels_are_ignored_and_an_unused_label_is_a_nan_row():
  x = np.arange(12.0).reshape(6, 2)
  got = cr.centroids(x, np.array([0, -1, 3, 0, -7, 3]))
  assert got.shape == (4, 2)
  assert np.array_equal(got[0], (x[0] + x[3]) / 2) and np.array_equal(got[3], (x[2] + x[5]) / 2)
  assert np.isnan(got[1]).all() and np.isnan(got[2]).all()
  assert cr.centroids(x, np.full(6, -1)).shape == (0, 2)
  bits = cr.centroid_bits(x, np.array([0, 0, 0, 1, 1, 1]), "bfloat16")
  assert bits.dtype == np.uint16 and bits.shape == (2, 2)


# ------------------------------------------------------------------- the ABI additions
def test_header_binding_and_library_agree_on_the_additions():
  header = open(os.path.join(ROOT, "include", "spectralcluster_amd.h")).read()
  integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
  lib = _lib.load()
  for name in ("sc_cluster_centroids_arrays", "sc_labels_egress"):
    assert re.search(r"^int\s+%s\s*\(" % name, header, flags=re.M), name
    assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert "`%s`" % name in integration, name
    args = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, header, flags=re.M | re.S).group(1)
    assert len(args.split(",")) == len(_lib.PROTOTYPES[name][1]), name
  assert re.search(r"SC_DTYPE_I64\s*=\s*4,\s*SC_DTYPE_I32\s*=\s*5", header)
  assert (_lib.SC_DTYPE_I64, _lib.SC_DTYPE_I32) == (4, 5)
  assert lib.sc_abi_version() == _lib.SC_ABI_VERSION == 11  # functions were only added
  assert lib.sc_cluster_centroids_arrays(None, None, None, 1, None, None) == _lib.SC_ERR_INVALID
  assert lib.sc_labels_egress(None, None, 1, None) == _lib.SC_ERR_INVALID


def test_the_python_surface():
  assert list(inspect.signature(utils.get_cluster_centroids).parameters) == [
      "embeddings", "labels", "out"]
  assert list(inspect.signature(utils.get_cluster_centroids_batch).parameters) == [
      "embeddings_list", "labels_list", "out"]
  for f in (sca.SpectralClusterer.predict, sca.SpectralClusterer.predict_affinity,
            sca.SpectralClusterer.predict_batch, sca.SpectralClusterer.predict_affinity_batch):
    p = inspect.signature(f).parameters["out"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, f.__qualname__
    assert "`out`" in f.__doc__, f.__qualname__


# ------------------------------------------------------------------------ label arrays
def no_handle():
  raise AssertionError("a host array must not ask for the handle")


def described(src):
  a = src.array
  return (a.data, a.dtype, a.location, a.rows, a.cols, a.row_stride, a.col_stride)


def test_label_inputs_are_described_as_they_lie():
  host = _lib.SC_MEM_HOST
  a = np.arange(10, dtype=np.int64)
  src = _dlpack.describe_labels(a, no_handle, 10)
  assert described(src) == (a.ctypes.data, _lib.SC_DTYPE_I64, host, 1, 10, 0, 1)
  src = _dlpack.describe_labels(a[1::2], no_handle, 5)
  assert described(src) == (a.ctypes.data + 8, _lib.SC_DTYPE_I64, host, 1, 5, 0, 2)
  b = np.arange(6, dtype=np.int32)
  assert described(_dlpack.describe_labels(b, no_handle, 6))[:2] == (b.ctypes.data, _lib.SC_DTYPE_I32)
  f = np.array([0.0, 2.0, -1.0, 2.0])
  assert described(_dlpack.describe_labels(f, no_handle, 4))[:2] == (f.ctypes.data, _lib.SC_DTYPE_F64)
  g = f.astype(np.float32)
  assert described(_dlpack.describe_labels(g, no_handle, 4))[1] == _lib.SC_DTYPE_F32
  # a broadcast (stride 0) label array is an input like any other
  z = np.broadcast_to(np.zeros(1, dtype=np.int64), (7,))
  assert described(_dlpack.describe_labels(z, no_handle, 7))[-1] == 0
  # other integer types, bools and lists are converted on the host
  for other in (np.arange(5, dtype=np.int16), np.arange(5, dtype=np.uint8),
                np.arange(5, dtype=">i8"), np.array([True, False, True, True, False]),
                [0, 1, 2, 1, 0]):
    src = _dlpack.describe_labels(other, no_handle, 5)
    assert described(src)[1:5] == (_lib.SC_DTYPE_I64, host, 1, 5)
    assert np.array_equal(src.numpy, np.asarray(other).astype(np.int64))
  # host DLPack objects
  t = torch.arange(12, dtype=torch.int32)
  src = _dlpack.describe_labels(t[2::3], no_handle, 4)
  assert described(src) == (t.data_ptr() + 8, _lib.SC_DTYPE_I32, host, 1, 4, 0, 3)
  src.release()
  src = _dlpack.describe_labels(torch.zeros(3, dtype=torch.float64), no_handle, 3)
  assert described(src)[1] == _lib.SC_DTYPE_F64
  src.release()


@pytest.mark.parametrize("name,labels,n,exc,match", [
    ("length", np.zeros(5, dtype=np.int64), 6, ValueError, "labels must hold 6 entries, not 5"),
    ("torch length", torch.zeros(5, dtype=torch.int64), 6, ValueError, "must hold 6 entries, not 5"),
    ("two dimensions", np.zeros((3, 2), dtype=np.int64), 3, ValueError, "1-dimensional"),
    ("torch two dimensions", torch.zeros(3, 2, dtype=torch.int64), 3, ValueError, "1-dimensional"),
    ("a fraction", np.array([0.0, 0.5]), 2, ValueError, "finite integral"),
    ("a NaN", np.array([0.0, np.nan]), 2, ValueError, "finite integral"),
    ("an infinity", np.array([0.0, np.inf], dtype=np.float32), 2, ValueError, "finite integral"),
    ("above int32", np.array([0, 2**31], dtype=np.int64), 2, ValueError, "above 2147483646"),
    ("float above int32", np.array([0.0, 2.0**40]), 2, ValueError, "above 2147483646"),
    ("uint64 above int32", np.array([0, 2**63], dtype=np.uint64), 2, ValueError, "above"),
    ("complex", np.zeros(3, dtype=np.complex128), 3, TypeError, "int64 or int32"),
    ("float16", np.zeros(3, dtype=np.float16), 3, TypeError, "int64 or int32"),
    ("torch int16", torch.zeros(3, dtype=torch.int16), 3, TypeError, "int64 or int32"),
    ("negative stride", np.arange(4)[::-1], 4, ValueError, "negative strides"),
    ("torch meta", torch.zeros(3, dtype=torch.int64, device="meta"), 3, (TypeError, ValueError,
                                                                       RuntimeError), None),
])
def test_label_inputs_that_are_refused(name, labels, n, exc, match):
  with pytest.raises(exc, match=match):
    _dlpack.describe_labels(labels, no_handle, n)


def test_label_outputs_are_described_as_they_lie():
  host = _lib.SC_MEM_HOST
  a = np.zeros(10, dtype=np.int32)
  src = _dlpack.describe_labels_out(a[2:8:2], no_handle, 3)
  assert described(src) == (a.ctypes.data + 8, _lib.SC_DTYPE_I32, host, 1, 3, 0, 2)
  assert src.numpy.base is a
  t = torch.zeros(9, dtype=torch.int64)
  src = _dlpack.describe_labels_out(t[1:], no_handle, 8)
  assert described(src) == (t.data_ptr() + 8, _lib.SC_DTYPE_I64, host, 1, 8, 0, 1)
  src.release()
  one = np.broadcast_to(np.zeros(1, dtype=np.int64), (1,)).copy()
  assert described(_dlpack.describe_labels_out(one, no_handle, 1))[4] == 1


def read_only():
  a = np.zeros(4, dtype=np.int64)
  a.flags.writeable = False
  return a


@pytest.mark.parametrize("name,make,n,exc,match", [
    ("a list", lambda: [0, 0, 0, 0], 4, TypeError, "numpy array or an object with __dlpack__"),
    ("float64", lambda: np.zeros(4), 4, TypeError, "out must be int64 or int32"),
    ("int16", lambda: np.zeros(4, dtype=np.int16), 4, TypeError, "int64 or int32"),
    ("torch float32", lambda: torch.zeros(4), 4, TypeError, "int64 or int32"),
    ("too short", lambda: np.zeros(3, dtype=np.int64), 4, ValueError, r"shape \(4,\), not \(3,\)"),
    ("torch too long", lambda: torch.zeros(5, dtype=torch.int32), 4, ValueError, r"shape \(4,\)"),
    ("two dimensions", lambda: np.zeros((4, 1), dtype=np.int64), 4, ValueError, "shape"),
    ("torch two dimensions", lambda: torch.zeros(4, 1, dtype=torch.int64), 4, ValueError,
     "1-dimensional"),
    ("read only", read_only, 4, ValueError, "not writeable"),
    ("negative stride", lambda: np.zeros(4, dtype=np.int64)[::-1], 4, ValueError, "negative"),
    ("zero stride", lambda: np.lib.stride_tricks.as_strided(
        np.zeros(1, dtype=np.int64), (4,), (0,), writeable=True), 4, ValueError, "one address"),
    ("torch zero stride", lambda: torch.zeros(1, dtype=torch.int64).expand(4), 4, ValueError,
     "one address|export"),
])
def test_label_outputs_that_are_refused(name, make, n, exc, match):
  with pytest.raises(exc, match=match):
    _dlpack.describe_labels_out(make(), no_handle, n)


# ---------------------------------------------------------------------- a fake library
class Recorder:
  """Stands for a `_lib.Handle`: every library call is recorded and answers SC_OK."""

  raw = "raw"
  device = 0

  def __init__(self):
    self.calls = []
    self.lib = self

  def __getattr__(self, name):
    if not name.startswith("sc_"):
      raise AttributeError(name)

    def call(*args):
      self.calls.append((name,) + args)
      return _lib.SC_OK
    return call

  def check(self, rc, invalid_exc=ValueError):
    assert rc == _lib.SC_OK

  def stream(self):
    raise AssertionError("a host input must not ask for the stream")


@pytest.fixture
def recorder(monkeypatch):
  rec = Recorder()
  monkeypatch.setattr(_lib, "default_handle", lambda device=None: rec)
  return rec


def test_numpy_in_and_no_out_takes_todays_call_and_nothing_else(recorder):
  x = np.arange(12.0).reshape(6, 2)
  for e, l in ((x, np.array([0, 1, 0, 1, 2, 2])), (x.astype(np.float32), np.array([0, 1, 0, 1, 2, 2],
                                                                                dtype=np.int32)),
               (x.tolist(), [0, 1, 0, 1, 2, 2]), (x[:, ::-1], np.array([2.0, 1, 0, 1, 2, 2]))):
    del recorder.calls[:]
    got = utils.get_cluster_centroids(e, l)
    (call,) = recorder.calls
    assert call[0] == "sc_cluster_centroids" and call[3:5] == (6, 2) and call[6] == 3
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (3, 2)
  with pytest.raises(ValueError, match="labels \\(n_samples,\\)"):
    utils.get_cluster_centroids(x, np.zeros(5, dtype=np.int64))


def test_an_out_or_a_dlpack_argument_takes_the_array_entry(recorder):
  x = np.zeros((6, 4), dtype=np.float32)
  lab = np.array([0, 1, 0, 1, 2, 2])
  big = np.zeros((8, 8), dtype=np.float16)
  o = big[1:6, 2:6]  # five rows for three clusters
  got = utils.get_cluster_centroids(x, lab, out=o)
  (name, raw, xs, ls, count, outs, ks), = recorder.calls
  assert name == "sc_cluster_centroids_arrays" and count == 1
  assert (xs[0].rows, xs[0].cols, xs[0].dtype, xs[0].data) == (6, 4, _lib.SC_DTYPE_F32, x.ctypes.data)
  assert (ls[0].rows, ls[0].cols, ls[0].dtype, ls[0].col_stride) == (1, 6, _lib.SC_DTYPE_I64, 1)
  assert (outs[0].data, outs[0].rows, outs[0].cols, outs[0].row_stride, outs[0].dtype) == (
      o.ctypes.data, 5, 4, 8, _lib.SC_DTYPE_F16)
  assert got.shape == (0, 4) and got.base is big  # (the fake library reports k = 0)

  for e, l in ((torch.zeros(6, 4, dtype=torch.bfloat16), lab), (x, torch.zeros(6, dtype=torch.int32)),
               (torch.zeros(6, 4), torch.zeros(6, dtype=torch.float64))):
    del recorder.calls[:]
    got = utils.get_cluster_centroids(e, l)
    names = [c[0] for c in recorder.calls]
    # labels the host holds give k here; labels in a DLPack object are the library's to read
    assert names == ["sc_cluster_centroids_arrays"] * (1 if isinstance(l, np.ndarray) else 2)
    if len(names) == 2:
      assert recorder.calls[0][5] is None  # the extent call: no outputs
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape[1] == 4


@pytest.mark.parametrize("count", [1, 2, 70])
def test_a_batch_is_one_call_of_the_new_entry(recorder, count):
  rng = np.random.default_rng(count)
  xs, ls = [], []
  for i in range(count):
    n = int(rng.integers(1, 30))
    x = rng.standard_normal((n, 5))
    xs.append(x if i % 3 else torch.from_numpy(x.astype(np.float32)))
    ls.append(rng.integers(0, 3, size=n).astype(np.int32 if i % 2 else np.int64))
  got = utils.get_cluster_centroids_batch(xs, ls)
  (call,) = recorder.calls
  assert call[0] == "sc_cluster_centroids_arrays" and call[4] == count
  assert [int(call[2][i].rows) for i in range(count)] == [x.shape[0] for x in xs]
  assert [int(call[5][i].rows) for i in range(count)] == [int(l.max()) + 1 for l in ls]
  assert len(got) == count
  del recorder.calls[:]
  outs = [np.zeros((3, 5), dtype=np.float32) for _ in range(count)]
  got = utils.get_cluster_centroids_batch(xs, ls, out=outs)
  assert [c[0] for c in recorder.calls] == ["sc_cluster_centroids_arrays"]
  assert all(g.base is o for g, o in zip(got, outs))
  assert utils.get_cluster_centroids_batch([], []) == [] and len(recorder.calls) == 1


class FakeDevice:
  """A DLPack object that says it lives on the GPU: `n` elements of `dtype` at address `at`."""

  def __init__(self, at, shape, dtype):
    self.host = np.zeros(shape, dtype=dtype)
    self.at, self.shape = at, shape

  def __dlpack_device__(self):
    return (_dlpack.KDL_ROCM, 0)

  def __getitem__(self, rows):
    return self

  def __dlpack__(self, stream=None):
    # the capsule of the host twin, its data pointer replaced
    capsule = torch.from_numpy(self.host).__dlpack__()
    address = _dlpack._get_pointer(capsule, _dlpack._NAME)
    managed = ctypes.cast(address, ctypes.POINTER(_dlpack.DLManagedTensor))
    managed.contents.dl_tensor.data = self.at
    managed.contents.dl_tensor.device.device_type = _dlpack.KDL_ROCM
    return capsule


def test_every_error_is_raised_before_any_library_call(recorder, monkeypatch):
  monkeypatch.setattr(Recorder, "stream", lambda self: 0)
  x = np.zeros((6, 4))
  lab = np.array([0, 1, 0, 1, 2, 2])
  good = np.zeros((3, 4))
  for args, exc, match in (
      (([x, x], [lab, lab[:5]], [good, good]), ValueError, "labels of member 1 must hold 6 entries"),
      (([x, x], [lab, lab + 0.5], [good, good]), ValueError, "labels of member 1.*integral"),
      (([x, x], [lab, np.where(lab == 2, np.inf, 0.0)], None), ValueError, "labels of member 1"),
      (([x, x], [lab * 2**31, lab], None), ValueError, "labels of member 0.*above"),
      (([x, x], [lab, lab], [good, np.zeros((3, 5))]), ValueError,
       r"out of member 1 must be \(rows >= k, 4\), not \(3, 5\)"),
      (([x, x], [lab, lab], [good, np.zeros((2, 4))]), ValueError,
       "out of member 1 has 2 rows, the labels make 3 clusters"),
      (([x, x], [lab, lab], [good, np.zeros(4)]), ValueError, "out of member 1"),
      (([x, x], [lab, lab], [good, np.zeros((3, 4), dtype=np.int64)]), TypeError, "out of member 1"),
      (([x, x], [lab, lab], [good, np.zeros((3, 8))[:, ::-2]]), ValueError, "out of member 1"),
      (([x, np.zeros((6, 5))], [lab, lab], None), ValueError, "member 1.*same d"),
      (([x, x], [lab], None), ValueError, "as long as"),
      (([x, x], [lab, lab], [good]), ValueError, "as long as"),
  ):
    with pytest.raises(exc, match=match):
      utils.get_cluster_centroids_batch(args[0], args[1], args[2])
  # an out in device memory that overlaps a device source of the call, of any member
  src = FakeDevice(0x10000, (6, 4), np.float64)          # bytes 0x10000 .. 0x100c0
  lab_d = FakeDevice(0x20000, (6,), np.int64)            # bytes 0x20000 .. 0x20030
  for at, clash in ((0x10000 + 8 * 23, True), (0x10000 + 8 * 24, False), (0x20000 - 96 + 8, True),
                    (0x20000 - 96, False), (0x20028, True), (0x20030, False)):
    out_d = FakeDevice(at, (3, 4), np.float64)
    call = lambda: utils.get_cluster_centroids_batch([x, src], [lab_d, lab],
                                                     [out_d, np.zeros((3, 4))])
    if clash:
      with pytest.raises(ValueError, match="out of member 0 overlaps"):
        call()
    else:
      del recorder.calls[:]
      call()
      assert [c[0] for c in recorder.calls] == ["sc_cluster_centroids_arrays"]
      del recorder.calls[:]
  assert recorder.calls == []


# -------------------------------------------------------------- labels out of predict
def test_every_out_of_a_predict_call_is_validated_before_anything_runs(monkeypatch):
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=4)
  ran = []
  monkeypatch.setattr(c, "_handle", no_handle)
  x = np.zeros((6, 3))
  a = np.zeros((6, 6))
  monkeypatch.setattr(_batch, "_EXECUTORS", {f: (lambda *args: ran.append(1)) for f in _batch.Family})
  bad = [(np.zeros(6), TypeError, "int64 or int32"), (np.zeros(5, dtype=np.int64), ValueError, "shape"),
         (read_only(), ValueError, "writeable|shape"), ([0] * 6, TypeError, "numpy array or"),
         (np.zeros(12, dtype=np.int32)[::-2], ValueError, "negative")]
  for out, exc, match in bad:
    with pytest.raises(exc, match=match):
      c.predict(x, out=out)
    with pytest.raises(exc, match=match):
      c.predict_affinity(a, out=out)
    with pytest.raises(exc, match="out 1|" + match):
      c.predict_batch([x, x], out=[np.zeros(6, dtype=np.int64), out])
    with pytest.raises(exc, match="out 1|" + match):
      c.predict_affinity_batch([a, a], out=[np.zeros(6, dtype=np.int32), out])
  with pytest.raises(ValueError, match="as long as the batch"):
    c.predict_batch([x, x], out=[np.zeros(6, dtype=np.int64)])
  assert ran == []


class OnlyDLPack:
  """A producer without a `shape` attribute."""

  def __init__(self, tensor):
    self._tensor = tensor

  def __dlpack__(self, stream=None):
    return self._tensor.__dlpack__()

  def __dlpack_device__(self):
    return self._tensor.__dlpack_device__()


def test_the_rows_of_an_input_come_from_its_shape_or_its_description():
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=4)
  c._handle = no_handle
  assert _batch.rows_of(c, np.zeros((7, 3))) == 7
  assert _batch.rows_of(c, torch.zeros(5, 3)) == 5
  assert _batch.rows_of(c, OnlyDLPack(torch.zeros(9, 3, dtype=torch.float16))) == 9
  for bad in ([[0.0, 1.0]], 3.0, np.float64(1.0)):
    with pytest.raises(TypeError, match="embeddings must be a numpy array"):
      _batch.rows_of(c, bad)


def test_labels_of_every_dtype_a_call_returns_are_converted_exactly():
  assert _batch.exact_int64(np.array([0.0, 2.0, 1.0])).dtype == np.int64
  assert np.array_equal(_batch.exact_int64(np.array([0.0, 2.0, 1.0])), [0, 2, 1])
  assert np.array_equal(_batch.exact_int64(np.array([0] * 3)), [0, 0, 0])
  with pytest.raises(ValueError, match="not integral"):
    _batch.exact_int64(np.array([0.5]))
