"""GPU: embeddings taken where they are -- device tensors and host arrays of float64 / float32 /
float16 / bfloat16, contiguous or strided.  Widening to float64 is exact, so every check here is
an equality: the ingest against PyTorch's own CPU widening bit for bit, labels / eigenvalues /
routes against the same call on the widened NumPy float64 array."""

import copy
import ctypes

import numpy as np
import pytest
# (at module level on purpose: PyTorch has to be in the process before the library is loaded,
#  so that both use one HIP runtime -- INTEGRATION.md section 6)
import torch

import spectral_oracle as so
from conftest import golden

import spectralcluster_amd as sca
from spectralcluster_amd import _dlpack
from spectralcluster_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32, torch.float16, torch.bfloat16]
# (1,1): one element; (5,3) / (7,17): rows shorter / a little longer than one 16-byte load and
# than the 16-column padding; (33,257): a ragged tail after whole loads; (64,256): no tail at all;
# (130,250): more rows than a workgroup has lanes per row, tail and padding together
# (the last three: one row -- its pitch addresses nothing; 65 rows cross the 64-wide tile edge with
#  17 columns, where the 16-byte item straddles the row end for every element width; one column)
SHAPES = [(1, 1), (5, 3), (7, 17), (33, 257), (64, 256), (130, 250), (1, 17), (65, 17), (65, 1)]
LAP = {0: None, 4: sca.LaplacianType.GraphCut}


def widened(t: torch.Tensor) -> np.ndarray:
  return t.cpu().double().numpy()


def layouts(n, d, dtype, seed):
  """One (n, d) matrix of values in four layouts: name -> (base tensor on the CPU, function
  that takes the (n, d) view of a base -- applied to the base's device copy too)."""
  g = torch.Generator().manual_seed(seed)
  v = (torch.randn(n, d, generator=g, dtype=torch.float64) * 3).to(dtype)
  sliced = torch.zeros(n, d + 5, dtype=dtype)
  sliced[:, 3:3 + d] = v
  stepped = torch.zeros(2 * n, d, dtype=dtype)
  stepped[::2] = v
  return v, {
      "contiguous": (v.clone(), lambda b: b),
      # starts at an odd element: misaligned base, row stride > d
      "column_slice": (sliced, lambda b: b[:, 3:3 + d]),
      "row_step_2": (stepped, lambda b: b[::2]),
      "transposed": (v.t().contiguous(), lambda b: b.t()),
  }


def stage_ingest(handle, obj) -> np.ndarray:
  """sc_stage_ingest: the (rows, cols) float64 values the pipeline sees for `obj`."""
  src = _dlpack.describe(obj, lambda: handle)
  try:
    out = np.empty(src.shape, dtype=np.float64)
    handle.check(handle.lib.sc_stage_ingest(handle.raw, ctypes.byref(src.array),
                                            _lib.as_double_p(out)))
    return out
  finally:
    src.release()


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
  return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64),
                                               np.ascontiguousarray(b).view(np.int64))


def icassp_options():
  return sca.RefinementOptions(
      gaussian_blur_sigma=1, p_percentile=0.95, thresholding_soft_multiplier=0.01,
      thresholding_type=sca.ThresholdType.RowMax,
      refinement_sequence=sca.ICASSP2018_REFINEMENT_SEQUENCE)


# --- the ingest alone ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda t: str(t).split(".")[-1])
def test_ingest_is_exact_for_every_layout_from_device_and_host(handle, dtype, shape):
  n, d = shape
  v, views = layouts(n, d, dtype, seed=n * 1000 + d)
  want = widened(v)
  for name, (base, view) in views.items():
    t = view(base)
    assert tuple(t.shape) == (n, d) and torch.equal(t, v)
    dev = view(base.cuda())  # the same strides and offset in device memory
    assert dev.stride() == t.stride() and dev.storage_offset() == t.storage_offset()
    assert same_bits(stage_ingest(handle, dev), want), (name, "device")
    # host memory, strides as they are
    assert same_bits(stage_ingest(handle, t), want), (name, "host")
    if dtype != torch.bfloat16:  # ... and as the NumPy array of the same dtype
      assert same_bits(stage_ingest(handle, t.numpy()), want), (name, "numpy")
  # rows that overlap (row stride 1 < d): from the host they are gathered before the upload
  flat = v.flatten()[:n + d - 1].contiguous()
  for base in (flat, flat.cuda()):
    rows = base.as_strided((n, d), (1, 1))
    assert same_bits(stage_ingest(handle, rows), widened(rows.contiguous())), ("overlapping", base.device)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16],
                         ids=lambda t: str(t).split(".")[-1])
def test_every_bit_pattern_of_the_16_bit_formats(handle, dtype):
  bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).reshape(256, 256)
  t = bits.view(dtype)
  want = widened(t)
  got = stage_ingest(handle, t.cuda())
  nan = np.isnan(want)
  assert nan.sum() == (2046 if dtype == torch.float16 else 254)
  assert np.array_equal(np.isnan(got), nan)
  # every finite value, +-0 and +-inf: the same 64 bits
  assert np.array_equal(got.view(np.int64)[~nan], want.view(np.int64)[~nan])
  # the aligned host form runs the wide loads on the staging buffer
  assert same_bits(stage_ingest(handle, t)[~nan], want[~nan])


# --- predict() ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["e2e_f32_n200_lap4_max7.npz", "e2e_f32_n1000_lap4_max20.npz"])
def test_predict_on_a_device_float32_tensor_vs_golden_and_vs_numpy(name):
  g = golden(name)
  n, d, k, seed, lap, max_clusters = [int(v) for v in g["params"]]
  x = so.blobs(n, d, k, seed).astype(np.float32)
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=max_clusters,
                            refinement_options=icassp_options(), laplacian_type=LAP[lap])
  want = c.predict(x.astype(np.float64))
  w_want = c.last_diag.eigenvalue_array()
  labels = c.predict(torch.from_numpy(x).cuda())
  assert labels.dtype == np.int64 and isinstance(labels, np.ndarray)
  assert so.adjusted_rand_index(labels, g["labels"]) == 1.0
  assert c.last_diag.n_clusters_raw == int(g["n_clusters_raw"])
  assert np.array_equal(labels, want)
  assert np.array_equal(c.last_diag.eigenvalue_array(), w_want)
  # host float32, now uploaded at its own width
  assert np.array_equal(c.predict(x), want)
  assert np.array_equal(c.last_diag.eigenvalue_array(), w_want)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16],
                         ids=lambda t: str(t).split(".")[-1])
def test_predict_on_the_jacobi_route_from_16_bit_device_tensors(dtype):
  t = torch.from_numpy(so.blobs(100, 32, 3, seed=100)).to(dtype)
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=7, refinement_options=icassp_options(),
                            laplacian_type=sca.LaplacianType.GraphCut)
  want = c.predict(widened(t))
  w_want = c.last_diag.eigenvalue_array()
  assert c.last_diag.eig_path == 1  # SC_EIG_PATH_DENSE_JACOBI
  got = c.predict(t.cuda())
  assert np.array_equal(got, want)
  assert np.array_equal(c.last_diag.eigenvalue_array(), w_want)


def both(c, x32: np.ndarray, *args):
  """predict() on the device tensor and on NumPy given the same values."""
  want = c.predict(x32.astype(np.float64), *args)
  p_want = getattr(c, "last_best_p", None)
  got = c.predict(torch.from_numpy(x32).cuda(), *args)
  assert np.array_equal(got, want)
  assert getattr(c, "last_best_p", None) == p_want
  return got


def test_autotune_route_with_a_device_tensor():
  x = so.blobs(512, 64, 6, 512).astype(np.float32)
  tuner = sca.AutoTune(p_percentile_min=0.55, p_percentile_max=0.95,
                       init_search_step=0.025, search_level=1)
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=20, refinement_options=icassp_options(),
                            autotune=tuner, laplacian_type=sca.LaplacianType.GraphCut)
  both(c, x)
  assert c.last_best_p is not None


def test_constraint_band_route_with_a_device_tensor():
  x, _, scores = so.turn_blobs(300, 24, 4, seed=301, noise=1.0)
  c = copy.deepcopy(sca.configs.turntodiarize_clusterer)
  both(c, x.astype(np.float32), sca.ConstraintMatrix(list(scores), 1))


def test_single_cluster_condition_on_the_affinity_with_a_device_tensor():
  opts = sca.FallbackOptions(
      single_cluster_condition=sca.SingleClusterCondition.AllAffinity,
      single_cluster_affinity_threshold=0.9)
  c = sca.SpectralClusterer(min_clusters=1, max_clusters=7, refinement_options=icassp_options(),
                            fallback_options=opts, laplacian_type=sca.LaplacianType.GraphCut)
  several = so.blobs(200, 32, 3, seed=9).astype(np.float32)
  assert len(set(both(c, several))) > 1
  one = (np.ones((60, 8)) + 1e-3 * np.random.default_rng(1).standard_normal((60, 8)))
  assert set(both(c, one.astype(np.float32))) == {0}


# --- predict_batch() ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch_inputs():
  sizes = [20, 64, 128, 129, 300, 700] * 2
  halves = [torch.from_numpy(so.blobs(n, 32, 2 + i % 3, seed=4000 + i)).to(torch.float16)
            for i, n in enumerate(sizes)]
  return halves, [widened(t) for t in halves]


@pytest.mark.parametrize("mode", [dict(group=16), dict(streams=2)], ids=["group16", "streams2"])
def test_predict_batch_on_device_float16_and_host_float32(batch_inputs, mode):
  halves, wide = batch_inputs
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=7, refinement_options=icassp_options(),
                            laplacian_type=sca.LaplacianType.GraphCut)
  want = c.predict_batch(wide, **mode)
  routes = list(c.last_batch_routes)
  if "group" in mode:
    assert set(routes) == {_lib.BATCH_ROUTE_GROUP_JACOBI, _lib.BATCH_ROUTE_GROUP_LANCZOS}
  for utts in ([t.cuda() for t in halves], [t.float().numpy() for t in halves]):
    got = c.predict_batch(utts, **mode)
    assert c.last_batch_routes == routes
    assert len(got) == len(want)
    for i in range(len(want)):
      assert np.array_equal(got[i], want[i]), i


# --- the branches that need the embeddings on the host ---------------------------------------
def test_size_reduction_and_too_few_embeddings_with_a_device_tensor():
  x = so.blobs(300, 16, 3, seed=30).astype(np.float32)
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=7, max_spectral_size=100,
                            refinement_options=icassp_options(),
                            laplacian_type=sca.LaplacianType.GraphCut)
  both(c, x)
  few = so.blobs(12, 16, 2, seed=31).astype(np.float32)
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=7,
                            fallback_options=sca.FallbackOptions(spectral_min_embeddings=20))
  both(c, few)


# --- stream ordering --------------------------------------------------------------------------
def test_a_pending_write_on_another_stream_is_ordered_before_the_ingest():
  x = torch.from_numpy(so.blobs(400, 64, 4, seed=77).astype(np.float32))
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=7, refinement_options=icassp_options(),
                            laplacian_type=sca.LaplacianType.GraphCut)
  want = c.predict(x.numpy())
  staged = x.cuda()
  t = torch.zeros_like(staged)
  big = torch.empty(1 << 30, dtype=torch.float32, device="cuda")  # 4 GiB: a fill takes a while
  torch.cuda.synchronize()
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    big.fill_(1.0)
    big.fill_(2.0)
    t.copy_(staged)          # queued behind the fill, not yet done when predict() is called
    got = c.predict(t)       # no synchronisation by the caller
    kept = t.clone()
    del t                    # the library is done with it
  torch.cuda.synchronize()
  assert np.array_equal(got, want)
  assert torch.equal(kept.cpu(), x)  # the source was only read
  assert np.array_equal(c.predict(staged), want)  # ... and the same after a full synchronise


# --- the raw C ABI ----------------------------------------------------------------------------
def test_a_host_pointer_described_as_device_memory_is_refused(handle):
  lib = handle.lib
  x = so.blobs(50, 8, 2, seed=3)
  out = np.full((50, 8), -7.0)
  good = dict(data=x.ctypes.data, dtype=_lib.SC_DTYPE_F64, location=_lib.SC_MEM_HOST, rows=50,
              cols=8, row_stride=8, col_stride=1)
  lying = _lib.ScArray(**dict(good, location=_lib.SC_MEM_DEVICE))
  assert lib.sc_stage_ingest(handle.raw, ctypes.byref(lying), _lib.as_double_p(out)) == \
      _lib.SC_ERR_INVALID
  assert "not device memory" in handle.last_error()
  assert np.all(out == -7.0)  # nothing ran
  labels = np.full(50, -1, dtype=np.int64)
  cfg = sca.SpectralClusterer(min_clusters=2, max_clusters=4).build_config()
  lp = (ctypes.POINTER(ctypes.c_int64) * 1)(_lib.as_int64_p(labels))
  assert lib.sc_predict_batch_arrays(handle.raw, ctypes.byref(lying), 1, cfg, lp, None, 16,
                                     1) == _lib.SC_ERR_INVALID
  assert np.all(labels == -1)
  # the other descriptor checks, same status, nothing launched
  for bad in (dict(data=None), dict(rows=0), dict(cols=-1), dict(dtype=4), dict(dtype=-1),
              dict(location=2), dict(row_stride=-8), dict(col_stride=-1)):
    arr = _lib.ScArray(**dict(good, **bad))
    assert lib.sc_stage_ingest(handle.raw, ctypes.byref(arr), _lib.as_double_p(out)) == \
        _lib.SC_ERR_INVALID, bad
    assert handle.last_error()
  assert np.all(out == -7.0)
  # the handle still works, and HIP carries no sticky error
  ok = _lib.ScArray(**good)
  handle.check(lib.sc_stage_ingest(handle.raw, ctypes.byref(ok), _lib.as_double_p(out)))
  assert np.array_equal(out, x)
  handle.check(lib.sc_synchronize(handle.raw))
  torch.cuda.synchronize()
