"""GPU: the k-means entries (`run_kmeans`, `CustomKMeans.predict`) take their input where it is --
device tensors and host arrays of float64 / float32 / float16 / bfloat16, contiguous or strided.
Widening to float64 is exact, so every check here is an equality: the column-major ingest
against PyTorch's own CPU widening bit for bit, labels / centroids / pass counts against the
same call on the widened C-contiguous NumPy float64 array (which the goldens of
tests/test_gpu_kmeans_dim.py and tests/test_gpu_stages.py pin to the reference)."""

import ctypes
import functools

import numpy as np
import pytest
# (at module level on purpose: PyTorch has to be in the process before the library is loaded,
#  so that both use one HIP runtime -- INTEGRATION.md section 6)
import torch

import spectral_oracle as so

import spectralcluster_amd as sca
from spectralcluster_amd import _dlpack
from spectralcluster_amd import _lib
from spectralcluster_amd import custom_distance_kmeans as ckm

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32, torch.float16, torch.bfloat16]
dtype_id = lambda t: str(t).split(".")[-1]
# where a 64-row tile, a 16-byte item (2 / 4 / 8 elements) or the round_up(n, 16) pitch changes
NS = [1, 15, 16, 17, 63, 64, 65, 129]
DIMS = [1, 3, 16, 17, 64, 65]

# 16-bit patterns beyond the random values: +-0, the smallest and the largest subnormal, the
# smallest normal, the largest finite value, +-inf, and quiet NaNs with payloads.  (Signalling
# NaNs are left out of a bit-for-bit comparison: the CPU conversion that serves as the reference
# sets their quiet bit.)
SPECIAL_BITS = {
    torch.float16: [0x0000, 0x8000, 0x0001, 0x8001, 0x03ff, 0x0400, 0x7bff, 0xfbff, 0x7c00, 0xfc00,
                    0x7e00, 0x7e01, 0xfe55, 0x7fff],
    torch.bfloat16: [0x0000, 0x8000, 0x0001, 0x8001, 0x007f, 0x0080, 0x7f7f, 0xff7f, 0x7f80,
                     0xff80, 0x7fc0, 0x7fc1, 0xffd5, 0x7fff],
}


def widened(t: torch.Tensor) -> np.ndarray:
  return t.cpu().double().numpy()


def values(n, dim, dtype, seed):
  """(n, dim) random values of `dtype` with the special values spread over them."""
  g = torch.Generator().manual_seed(seed)
  v = (torch.randn(n, dim, generator=g, dtype=torch.float64) * 3).to(dtype)
  flat = v.reshape(-1)
  if dtype in SPECIAL_BITS:
    bits = torch.tensor(SPECIAL_BITS[dtype], dtype=torch.int32).to(torch.int16).view(dtype)
  else:
    bits = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan")]).to(dtype)
  where = (torch.arange(len(bits)) * 7) % flat.numel()
  flat[where] = bits[:len(where)]
  return v


def layouts(v):
  """The (n, dim) values `v` in the six layouts: name -> (base tensor on the CPU, function that
  takes the (n, dim) view of a base -- applied to the base's device copy too, values expected)."""
  n, dim = v.shape
  stepped_rows = torch.zeros(2 * n, dim, dtype=v.dtype)
  stepped_rows[::2] = v
  stepped_cols = torch.zeros(n, 3 * dim, dtype=v.dtype)
  stepped_cols[:, ::3] = v
  shifted = torch.zeros(n, dim + 1, dtype=v.dtype)
  shifted[:, 1:] = v
  return {
      "contiguous": (v.clone(), lambda b: b, v),
      "row_step_2": (stepped_rows, lambda b: b[::2], v),
      "col_step_3": (stepped_cols, lambda b: b[:, ::3], v),
      # base off a 16-byte boundary, row pitch dim + 1
      "col_shift_1": (shifted, lambda b: b[:, 1:], v),
      "transposed": (v.t().contiguous(), lambda b: b.t(), v),
      # a zero row stride: every row is row 0
      "expanded": (v[:1].clone(), lambda b: b.expand(n, dim), v[:1].expand(n, dim)),
  }


def ingest_columns(handle, obj) -> np.ndarray:
  """sc_stage_ingest_columns: the (cols, round_up(rows, 16)) array whose row j is column j of
  what the k-means kernels are handed for `obj`."""
  src = _dlpack.describe(obj, lambda: handle, strided=True)
  try:
    n, dim = src.shape
    out = np.empty((dim, (n + 15) // 16 * 16), dtype=np.float64)
    handle.check(handle.lib.sc_stage_ingest_columns(handle.raw, ctypes.byref(src.array),
                                                    _lib.as_double_p(out)))
    return out
  finally:
    src.release()


def assert_columns(got: np.ndarray, want: np.ndarray, what):
  n = want.shape[0]
  assert got[:, :n].tobytes() == np.asfortranarray(want).T.tobytes(), what
  # the rest of every column: written as +0 (the entry fills the workspace with NaNs first)
  assert not got[:, n:].view(np.int64).any(), what


# --- 1. the kernel alone --------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_column_ingest_is_exact_for_every_layout_from_device_and_host(handle, dtype, n):
  # a larger call first: the workspace of the calls below is a used one
  ingest_columns(handle, torch.full((200, 70), 1.5, dtype=dtype, device="cuda"))
  for dim in DIMS:
    v = values(n, dim, dtype, seed=1000 * n + dim)
    for name, (base, view, expect) in layouts(v).items():
      t = view(base)
      assert tuple(t.shape) == (n, dim)
      want = widened(expect)
      dev = view(base.cuda())  # the same strides and offset in device memory
      assert dev.stride() == t.stride() and dev.storage_offset() == t.storage_offset()
      assert_columns(ingest_columns(handle, dev), want, (dim, name, "device"))
      assert_columns(ingest_columns(handle, t), want, (dim, name, "host"))
      if dtype != torch.bfloat16:  # the NumPy view, strides as they are
        assert_columns(ingest_columns(handle, t.numpy()), want, (dim, name, "numpy"))


def test_column_ingest_refuses_a_bad_descriptor_before_anything_runs(handle):
  lib = handle.lib
  x = so.blobs(50, 8, 2, seed=3)
  out = np.full((8, 64), -7.0)
  good = dict(data=x.ctypes.data, dtype=_lib.SC_DTYPE_F64, location=_lib.SC_MEM_HOST, rows=50,
              cols=8, row_stride=8, col_stride=1)
  labels = np.full(50, -1, dtype=np.int64)
  iters = ctypes.c_int(-1)
  for bad in (dict(data=None), dict(rows=0), dict(cols=-1), dict(dtype=4), dict(dtype=-1),
              dict(location=2), dict(row_stride=-8), dict(col_stride=-1),
              dict(location=_lib.SC_MEM_DEVICE),  # a host pointer called device memory
              dict(rows=1 << 16, cols=1 << 15)):  # 2^31 elements
    arr = _lib.ScArray(**dict(good, **bad))
    assert lib.sc_stage_ingest_columns(handle.raw, ctypes.byref(arr), _lib.as_double_p(out)) == \
        _lib.SC_ERR_INVALID, bad
    assert handle.last_error()
    assert lib.sc_stage_kmeans_general_array(
        handle.raw, ctypes.byref(arr), 2, 10, _lib.KMEANS_METRICS["cosine"], 0.001, None,
        _lib.as_int64_p(labels), None, ctypes.byref(iters)) == _lib.SC_ERR_INVALID, bad
    assert lib.sc_stage_kmeans_metric_array(
        handle.raw, ctypes.byref(arr), 10, _lib.KMEANS_METRICS["cosine"], _lib.as_int64_p(labels),
        None, ctypes.byref(iters)) == _lib.SC_ERR_INVALID, bad
  assert np.all(out == -7.0) and np.all(labels == -1) and iters.value == -1
  # the handle still works, and HIP carries no sticky error
  ok = _lib.ScArray(**good)
  handle.check(lib.sc_stage_ingest_columns(handle.raw, ctypes.byref(ok), _lib.as_double_p(out)))
  assert np.array_equal(out[:, :50], x.T) and not out[:, 50:].any()
  handle.check(lib.sc_synchronize(handle.raw))
  torch.cuda.synchronize()


# --- 2. both k-means forms ------------------------------------------------------------------
SIZES = [(65, 4, 4), (130, 6, 4), (300, 17, 5)]
KM_LAYOUTS = {
    "contiguous": lambda v: (v.clone(), lambda b: b),
    "col_step_2": lambda v: (_spread(v), lambda b: b[:, ::2]),
    "transposed": lambda v: (v.t().contiguous(), lambda b: b.t()),
}


def _spread(v):
  base = torch.zeros(v.shape[0], 2 * v.shape[1], dtype=v.dtype)
  base[:, ::2] = v
  return base


@functools.lru_cache(maxsize=None)
def km_values(n, dim, k, dtype):
  return torch.from_numpy(so.blobs(n, dim, k, seed=n + dim)).to(dtype)


def other_k(dim, k):
  """The cluster count of the `run_kmeans` call whose input is NOT (n, n_clusters)."""
  return k if k != dim else k + 1


def general_passes(obj, k, metric, init):
  """(labels, centroids, distance passes) of `_kmeans_general` on `obj` as the public entries
  hand it over."""
  source = ckm._describe(obj)
  try:
    return ckm._kmeans_general(ckm._input(source, obj), k, 10, _lib.kmeans_metric_code(metric),
                               0.001, init)
  finally:
    if source is not None:
      source.release()


@functools.lru_cache(maxsize=None)
def km_reference(n, dim, k, dtype, metric):
  """Every result of the three forms on the C-contiguous float64 array of the same values."""
  x = widened(km_values(n, dim, k, dtype))
  assert x.flags["C_CONTIGUOUS"] and x.dtype == np.float64
  init = x[np.linspace(0, n - 1, k).astype(int)].copy()
  km = ckm.CustomKMeans(k, centroids=init.copy(), custom_dist=metric)
  ck_labels = km.predict(x)
  ref = dict(square=ckm.run_kmeans(x, dim, metric, 300),
             general=ckm.run_kmeans(x, other_k(dim, k), metric, 300),
             ck_labels=ck_labels, ck_centroids=km.centroids, init=init,
             passes=general_passes(x, k, metric, init)[2])
  for a in ref.values():
    if isinstance(a, np.ndarray):
      a.setflags(write=False)
  return ref


def check_kmeans_forms(obj, n, dim, k, dtype, metric, what):
  ref = km_reference(n, dim, k, dtype, metric)
  assert np.array_equal(ckm.run_kmeans(obj, dim, metric, 300), ref["square"]), what
  assert np.array_equal(ckm.run_kmeans(obj, other_k(dim, k), metric, 300), ref["general"]), what
  km = ckm.CustomKMeans(k, centroids=ref["init"].copy(), custom_dist=metric)
  cent = km.centroids
  assert np.array_equal(km.predict(obj), ref["ck_labels"]), what
  assert km.centroids is cent and cent.dtype == np.float64  # updated in place, on the host
  assert cent.tobytes() == ref["ck_centroids"].tobytes(), what
  labels, cent2, passes = general_passes(obj, k, metric, ref["init"])
  assert passes == ref["passes"] and np.array_equal(labels, ref["ck_labels"]), what
  assert cent2.tobytes() == ref["ck_centroids"].tobytes(), what


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d_k%d" % s)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_kmeans_forms_match_the_float64_array_bit_for_bit(dtype, size):
  n, dim, k = size
  v = km_values(n, dim, k, dtype)
  for metric in ("cosine", "euclidean"):
    for name, make in KM_LAYOUTS.items():
      base, view = make(v)
      assert torch.equal(view(base), v)
      check_kmeans_forms(view(base.cuda()), n, dim, k, dtype, metric, (metric, name, "device"))
      check_kmeans_forms(view(base), n, dim, k, dtype, metric, (metric, name, "host"))
      if dtype != torch.bfloat16:
        check_kmeans_forms(view(base).numpy(), n, dim, k, dtype, metric, (metric, name, "numpy"))


def test_kmeans_forms_correlation_reads_the_row_means():
  n, dim, k = SIZES[2]
  v = km_values(n, dim, k, torch.float16)
  dev = v.t().contiguous().cuda().t()
  check_kmeans_forms(dev, n, dim, k, torch.float16, "correlation", "device transposed")
  check_kmeans_forms(v.clone(), n, dim, k, torch.float16, "correlation", "host contiguous")


def test_drawn_centroids_of_a_device_tensor_are_its_chosen_rows_on_the_host():
  n, dim, k = SIZES[1]
  v = km_values(n, dim, k, torch.float32)
  x = widened(v)
  np.random.seed(11)
  idx = np.random.choice(np.arange(n), size=k, replace=False)
  km = ckm.CustomKMeans(k)
  np.random.seed(11)
  dev = v.cuda()
  source = ckm._describe(dev)
  try:
    km._init_centroids(dev, source)
  finally:
    source.release()
  assert isinstance(km.centroids, np.ndarray) and km.centroids.dtype == np.float64
  assert km.centroids.tobytes() == x[idx].tobytes()
  # the whole call: what the float64 array gives (labels, or the reference's UnboundLocalError)
  def outcome(obj):
    np.random.seed(5)
    try:
      return ckm.CustomKMeans(k).predict(obj)
    except UnboundLocalError as exc:
      return str(exc)
  assert np.array_equal(outcome(dev), outcome(x))


# --- 3. stream ordering ---------------------------------------------------------------------
def test_a_pending_write_on_another_stream_is_ordered_before_the_kmeans_ingest():
  n, dim, k = 400, 16, 4
  x = torch.from_numpy(so.blobs(n, dim, k, seed=77).astype(np.float32))
  want = ckm.run_kmeans(x.numpy(), k, "cosine", 300)
  init = widened(x)[:k].copy()
  want_ck = ckm.CustomKMeans(k, centroids=init.copy()).predict(x.numpy())
  staged = x.cuda()
  t = torch.zeros_like(staged)
  big = torch.empty(1 << 30, dtype=torch.float32, device="cuda")  # 4 GiB: a fill takes a while
  torch.cuda.synchronize()
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    big.fill_(1.0)
    big.fill_(2.0)
    t.copy_(staged)                           # queued behind the fills, not yet done ...
    got = ckm.run_kmeans(t, k, "cosine", 300)  # ... when this is called, with no synchronisation
    t.zero_()
    big.fill_(3.0)
    t.copy_(staged)
    got_ck = ckm.CustomKMeans(k, centroids=init.copy()).predict(t)
    kept = t.clone()
  torch.cuda.synchronize()
  assert np.array_equal(got, want) and np.array_equal(got_ck, want_ck)
  assert torch.equal(kept.cpu(), x)  # the source was only read


# --- 4. the source is not modified and may be reused after return ----------------------------
@pytest.mark.parametrize("where", ["device", "host"])
def test_the_source_may_be_overwritten_after_return(where):
  n, dim, k = 130, 6, 4
  a = torch.from_numpy(so.blobs(n, dim, k, seed=1)).to(torch.float16)
  b = torch.from_numpy(so.blobs(n, dim, k, seed=2)[::-1].copy()).to(torch.float16)
  want_a = ckm.run_kmeans(widened(a), k + 1, "euclidean", 300)
  want_b = ckm.run_kmeans(widened(b), k + 1, "euclidean", 300)
  assert not np.array_equal(want_a, want_b)
  t = a.cuda() if where == "device" else a.clone()
  before = t.clone()
  assert np.array_equal(ckm.run_kmeans(t, k + 1, "euclidean", 300), want_a)
  assert torch.equal(t, before)
  t.copy_(b)  # the library holds nothing of the source any more
  assert np.array_equal(ckm.run_kmeans(t, k + 1, "euclidean", 300), want_b)


# --- 5. errors, each raised before anything moves ---------------------------------------------
def test_what_cannot_be_taken_is_refused_before_any_library_call(monkeypatch):
  good = torch.from_numpy(so.blobs(20, 3, 2, seed=9)).cuda()
  cent = widened(good)[:2].copy()
  handle = _lib.default_handle()

  class NoCalls:
    """The handle with a library that refuses every call."""
    device, raw = handle.device, handle.raw
    stream, check = handle.stream, handle.check

    class lib:
      def __getattr__(self, name):
        raise AssertionError("library call %s" % name)
    lib = lib()

  monkeypatch.setattr(_lib, "default_handle", lambda device=None: NoCalls)
  predict = lambda x, **kw: ckm.CustomKMeans(2, centroids=cent.copy(), **kw).predict(x)
  for x in (torch.zeros(20, 3, dtype=torch.int32, device="cuda"),
            torch.zeros(20, 3, dtype=torch.int32)):
    with pytest.raises(TypeError, match="float64, float32, float16 or bfloat16"):
      ckm.run_kmeans(x, 2, "cosine", 10)
    with pytest.raises(TypeError, match="float64, float32, float16 or bfloat16"):
      predict(x)
  with pytest.raises(BufferError):  # PyTorch's own refusal, passed on as it is
    ckm.run_kmeans(torch.zeros(20, 3, requires_grad=True), 2, "cosine", 10)
  with pytest.raises(BufferError):
    predict(torch.zeros(20, 3, requires_grad=True))
  for x in (torch.zeros(20, device="cuda"), torch.zeros(5, 2, 2, device="cuda")):
    with pytest.raises(ValueError, match="2-dimensional"):
      ckm.run_kmeans(x, 2, "cosine", 10)
    with pytest.raises(ValueError):  # the shape unpacking, as in the reference
      predict(x)
  with pytest.raises(ValueError, match=r"^n_samples=20 should be >= n_clusters=21$"):
    ckm.CustomKMeans(21, centroids=np.zeros((21, 3))).predict(good)
  with pytest.raises(sca.UnsupportedOnDeviceError, match="float64"):
    ckm.CustomKMeans(2, centroids=cent.astype(np.float32)).predict(good)
  with pytest.raises(sca.UnsupportedOnDeviceError):
    predict(good, custom_dist="mahalanobis")
  with pytest.raises(sca.UnsupportedOnDeviceError):
    ckm.run_kmeans(good, 2, "mahalanobis", 10)
  monkeypatch.undo()
  # n < k of run_kmeans is the library's check (the reference's message), before any copy
  with pytest.raises(ValueError, match="n_samples should be >= n_clusters"):
    ckm.run_kmeans(good, 21, "cosine", 10)
  with pytest.raises(ValueError, match="Number of iterations should be a positive number"):
    ckm.run_kmeans(good, 3, "cosine", 0)
  assert np.array_equal(predict(good), predict(widened(good)))  # the handle still works
