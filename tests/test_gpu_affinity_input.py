"""GPU: an affinity taken where it is.  The ingest (`k_ingest_affinity` and its grouped form) is
checked bit for bit against PyTorch's CPU widening, padding included, and its symmetry flag
against `np.array_equal(A, A.T)`; `predict_affinity` against the way in the library had before
(`affinity_function = lambda _: A64`) with equalities, and against the oracle composed for an
affinity (`_affinity_ref.predict_from_affinity`) at the project's 1e-5 eigenvalue bar."""

import copy
import ctypes

import numpy as np
import pytest
# (at module level on purpose: PyTorch has to be in the process before the library is loaded,
#  so that both use one HIP runtime -- INTEGRATION.md section 6)
import torch

import spectral_oracle as so
from _affinity_ref import eigengap_margin, predict_from_affinity

import spectralcluster_amd as sca
from spectralcluster_amd import _dlpack
from spectralcluster_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32, torch.float16, torch.bfloat16]
# 1, 2: less than one load; 15 / 16 / 17: the 16-column padding rule; 63 / 64 / 65: the kernel's
# 64 x 64 tile; 128 / 129: two tiles and a third; 511 / 512 / 513: matrix_ld adds 16 at 512
SIZES = [1, 2, 15, 16, 17, 63, 64, 65, 128, 129, 511, 512, 513]


def matrix_ld(n: int) -> int:
  ld = (n + 15) // 16 * 16
  return ld + 16 if ld % 512 == 0 else ld


def widened(t: torch.Tensor) -> np.ndarray:
  return t.cpu().double().numpy()


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
  return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64),
                                               np.ascontiguousarray(b).view(np.int64))


def layouts(n, dtype, seed):
  """One non-symmetric (n, n) matrix in five layouts: name -> (base tensor on the CPU, function
  that takes the (n, n) view of a base -- applied to the base's device copy too)."""
  g = torch.Generator().manual_seed(seed)
  v = (torch.randn(n, n, generator=g, dtype=torch.float64) * 3).to(dtype)
  stepped = torch.zeros(2 * n, 2 * n, dtype=dtype)
  stepped[::2, ::2] = v
  shifted = torch.zeros(n + 1, n + 1, dtype=dtype)  # the view starts one element and one row in:
  shifted[1:, 1:] = v                               # its base is not 16-byte aligned
  columns = torch.zeros(n, 2 * n, dtype=dtype)
  columns[:, ::2] = v
  return v, {
      "contiguous": (v.clone(), lambda b: b),
      "transposed": (v.t().contiguous(), lambda b: b.t()),
      "step_2_2": (stepped, lambda b: b[::2, ::2]),
      "shifted_1_1": (shifted, lambda b: b[1:, 1:]),
      "column_step_2": (columns, lambda b: b[:, ::2]),
  }


def stage(handle, obj):
  """sc_stage_affinity_ingest: the (n, ld) rows the kernel left on NaN-filled memory, the flag."""
  src = _dlpack.describe(obj, lambda: handle, strided=True)
  try:
    n = src.shape[0]
    out = np.full((n, matrix_ld(n)), -7.0)
    flag = ctypes.c_int(-1)
    handle.check(handle.lib.sc_stage_affinity_ingest(handle.raw, ctypes.byref(src.array),
                                                     _lib.as_double_p(out), ctypes.byref(flag)))
    return out, flag.value
  finally:
    src.release()


def stage_group(handle, objs):
  """sc_stage_affinity_ingest_group on the members `objs`: [(rows, flag)] from ONE launch."""
  sources = [_dlpack.describe(o, lambda: handle, strided=True) for o in objs]
  try:
    count = len(sources)
    outs = [np.full((s.shape[0], matrix_ld(s.shape[0])), -7.0) for s in sources]
    flags = (ctypes.c_int * count)(*([-1] * count))
    handle.check(handle.lib.sc_stage_affinity_ingest_group(
        handle.raw, (_lib.ScArray * count)(*[s.array for s in sources]), count,
        (ctypes.POINTER(ctypes.c_double) * count)(*[_lib.as_double_p(o) for o in outs]), flags))
    return list(zip(outs, list(flags)))
  finally:
    for s in sources:
      s.release()


def check_rows(got, want: np.ndarray, what):
  rows, flag = got
  n = want.shape[0]
  assert same_bits(rows[:, :n], want), what
  # the padding columns: +0.0, every bit
  assert not rows[:, n:].view(np.int64).any(), what
  assert flag == int(np.array_equal(want, want.T)), what


# --- the ingest alone ---------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda t: str(t).split(".")[-1])
def test_ingest_is_exact_for_every_layout_from_device_and_host(handle, dtype, n):
  v, views = layouts(n, dtype, seed=7000 + n)
  want = widened(v)
  for name, (base, view) in views.items():
    t = view(base)
    assert tuple(t.shape) == (n, n) and torch.equal(t, v)
    dev = view(base.cuda())  # the same strides and offset in device memory
    assert dev.stride() == t.stride() and dev.storage_offset() == t.storage_offset()
    check_rows(stage(handle, dev), want, (name, "device"))
    check_rows(stage(handle, t), want, (name, "host"))
    if dtype != torch.bfloat16:  # ... and as the NumPy view of the same strides
      check_rows(stage(handle, t.numpy()), want, (name, "numpy"))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16],
                         ids=lambda t: str(t).split(".")[-1])
def test_every_bit_pattern_of_the_16_bit_formats(handle, dtype):
  bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).reshape(256, 256)
  t = bits.view(dtype)
  want = widened(t)
  nan = np.isnan(want)
  for obj in (t.cuda(), t, t.cuda().t()):
    rows, flag = stage(handle, obj)
    ref = want.T if obj.stride(0) == 1 else want
    assert np.array_equal(np.isnan(rows[:, :256]), np.isnan(ref))
    assert np.array_equal(rows[:, :256].view(np.int64)[~np.isnan(ref)],
                          ref.view(np.int64)[~np.isnan(ref)])
    assert flag == 0
  assert nan.sum() == (2046 if dtype == torch.float16 else 254)


def test_grouped_ingest_of_members_of_different_size_dtype_layout_and_location(handle):
  members, wants, names = [], [], []
  layout_names = ["contiguous", "transposed", "step_2_2", "shifted_1_1", "column_step_2"]
  for i, n in enumerate(SIZES + [200, 300, 130]):
    dtype = DTYPES[i % 4]
    v, views = layouts(n, dtype, seed=8000 + n)
    name = layout_names[i % 5]
    base, view = views[name]
    on_device = i % 3 != 0
    members.append(view(base.cuda()) if on_device else view(base))
    wants.append(widened(v))
    names.append((n, str(dtype), name, "device" if on_device else "host"))
  # one symmetric member among them: the flags are per member
  s = torch.randn(150, 150, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
  s = (s + s.t()).float()
  members.append(s.cuda())
  wants.append(widened(s))
  names.append((150, "float32", "symmetric", "device"))
  got = stage_group(handle, members)
  assert len(got) == len(members) <= 64
  for g, want, name in zip(got, wants, names):
    check_rows(g, want, name)
  assert got[-1][1] == 1 and all(flag == 0 for _, flag in got[:-1] if _.shape[0] > 1)
  # the same members through the single kernel: the same rows
  for m, g in zip(members, got):
    rows, flag = stage(handle, m)
    assert same_bits(rows, g[0]) and flag == g[1]


# --- the symmetry flag ----------------------------------------------------------------------
def symmetric_matrix(n, dtype, seed):
  g = np.random.default_rng(seed)
  a = g.random((n, n))
  return ((a + a.T) / 2).astype(dtype)  # (rounding a symmetric matrix keeps it symmetric)


@pytest.mark.parametrize("n", [128, 129, 200])
@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.float16],
                         ids=["float64", "float32", "float16"])
def test_symmetry_flag_sees_one_ulp_anywhere(handle, dtype, n):
  a = symmetric_matrix(n, dtype, seed=n)
  assert np.array_equal(a, a.T)
  for obj in (a, torch.from_numpy(a).cuda(), torch.from_numpy(a).cuda().t()):
    assert stage(handle, obj)[1] == 1
  # corners of the matrix, both sides of a 64-tile corner, both sides of the 128 / 129 edge
  spots = [(0, n - 1), (n - 1, 0), (63, 64), (64, 63), (0, 64), (65, 127), (n - 2, n - 1),
           (n - 1, n - 2), (127, n - 1), (n - 1, 127), (126, 127)]
  group, wants = [], []
  for (i, j) in spots:
    if i == j:
      continue
    b = a.copy()
    b[i, j] = np.nextafter(b[i, j], dtype(4.0))
    assert not np.array_equal(b, b.T)
    assert stage(handle, torch.from_numpy(b).cuda())[1] == 0, (i, j)
    group.append(torch.from_numpy(b).cuda() if len(group) % 2 else b)
    wants.append(0)
  assert stage(handle, b)[1] == 0  # the host route (fp64: the 2-D copy and the separate pass)
  # per member of one grouped launch
  group.insert(3, torch.from_numpy(a).cuda())
  wants.insert(3, 1)
  group.append(a)
  wants.append(1)
  assert [flag for _, flag in stage_group(handle, group)] == wants
  # a changed diagonal element does not make a matrix non-symmetric
  d = a.copy()
  d[n // 2, n // 2] = np.nextafter(d[n // 2, n // 2], dtype(4.0))
  assert stage(handle, torch.from_numpy(d).cuda())[1] == 1


# --- predict_affinity against the way in the library had ------------------------------------
def icassp_options():
  return sca.RefinementOptions(
      gaussian_blur_sigma=1, p_percentile=0.95, thresholding_soft_multiplier=0.01,
      thresholding_type=sca.ThresholdType.RowMax,
      refinement_sequence=sca.ICASSP2018_REFINEMENT_SEQUENCE)


def parent_way(c, a64: np.ndarray, constraint_matrix=None):
  """predict() on a copy of `c` whose affinity_function returns `a64`: labels, eigenvalues,
  the copy."""
  old = copy.deepcopy(c)
  old.affinity_function = lambda _: a64
  labels = old.predict(np.zeros((a64.shape[0], 2)), constraint_matrix)
  return labels, old.consumed_eigenvalues(), old


def check_against_parent_way(c, affinity, constraint_matrix=None):
  """predict_affinity(affinity) == the parent's way on the widened values: labels equal,
  consumed eigenvalues bit for bit."""
  if isinstance(affinity, torch.Tensor):
    a64 = widened(affinity)
  else:
    a64 = np.asarray(affinity, dtype=np.float64)
  want, w_want, old = parent_way(c, a64, constraint_matrix)
  new = copy.deepcopy(c)
  got = new.predict_affinity(affinity, constraint_matrix)
  assert np.array_equal(got, want)
  assert same_bits(new.consumed_eigenvalues(), w_want)
  return got, new, old


@pytest.mark.parametrize("n,k,max_clusters", [(200, 3, 7), (1000, 5, 20)])
def test_predict_affinity_icassp_host_float64_and_device_float32_float16(n, k, max_clusters):
  a64 = so.affinity(so.blobs(n, 32, k, seed=n))
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=max_clusters,
                            refinement_options=icassp_options(),
                            laplacian_type=sca.LaplacianType.GraphCut)
  got, new, _ = check_against_parent_way(c, a64)
  assert len(set(got)) == k
  assert isinstance(got, np.ndarray) and got.dtype == np.int64
  for dtype in (torch.float32, torch.float16):
    t = torch.from_numpy(a64).to(dtype).cuda()
    labels, _, _ = check_against_parent_way(c, t)
    assert so.adjusted_rand_index(labels, got) == 1.0
    check_against_parent_way(c, t.t())  # (a symmetric matrix: the same values, walked by columns)


def test_predict_affinity_turntodiarize_autotune_and_constraint_matrix():
  x, _, scores = so.turn_blobs(300, 24, 4, seed=301, noise=1.0)
  c = copy.deepcopy(sca.configs.turntodiarize_clusterer)
  cm = sca.ConstraintMatrix(list(scores), 1)
  a64 = so.affinity(x)
  for affinity in (a64, torch.from_numpy(a64).float().cuda()):
    _, new, old = check_against_parent_way(c, affinity, cm)
    assert new.last_best_p is not None and new.last_best_p == old.last_best_p


def test_predict_affinity_min_clusters_1_with_affinity_gmm_bic():
  opts = sca.FallbackOptions(
      single_cluster_condition=sca.SingleClusterCondition.AffinityGmmBic,
      single_cluster_affinity_diagonal_offset=2)
  c = sca.SpectralClusterer(min_clusters=1, max_clusters=7, refinement_options=icassp_options(),
                            fallback_options=opts, laplacian_type=sca.LaplacianType.GraphCut)
  several = so.affinity(so.blobs(200, 32, 3, seed=9))
  one = so.affinity(np.ones((60, 8)) + 1e-3 * np.random.default_rng(1).standard_normal((60, 8)))
  for a64, single in ((several, False), (one, True)):
    for affinity in (a64, torch.from_numpy(a64).float().cuda()):
      got, _, _ = check_against_parent_way(c, affinity)
      assert (set(got) == {0}) == single


def test_predict_affinity_non_symmetric_without_symmetrize_takes_the_general_path(handle):
  a = so.affinity(so.blobs(300, 32, 3, seed=33))
  g = np.random.default_rng(3)
  a = a * (1.0 + 0.05 * g.random(a.shape))  # no longer symmetric
  assert not np.array_equal(a, a.T)
  options = sca.RefinementOptions(
      p_percentile=0.9, thresholding_soft_multiplier=0.01,
      thresholding_type=sca.ThresholdType.RowMax,
      refinement_sequence=[sca.RefinementName.RowWiseThreshold])
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=7, refinement_options=options)
  for affinity in (a, torch.from_numpy(a).float().cuda(), torch.from_numpy(a).cuda().t()):
    got, new, old = check_against_parent_way(c, affinity)
    assert new.last_diag.eig_path == old.last_diag.eig_path
  assert stage(handle, a)[1] == 0


def test_a_user_affinity_function_may_return_float32_or_a_device_tensor():
  x = so.blobs(200, 32, 3, seed=200)
  a32 = so.affinity(x).astype(np.float32)
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=7, refinement_options=icassp_options(),
                            laplacian_type=sca.LaplacianType.GraphCut)
  want, w_want, _ = parent_way(c, a32.astype(np.float64))
  for result in (a32, torch.from_numpy(a32).cuda(), a32.astype(np.float64).tolist()):
    user = copy.deepcopy(c)
    user.affinity_function = lambda _: result
    assert np.array_equal(user.predict(x), want)
    assert same_bits(user.consumed_eigenvalues(), w_want)


# --- against the oracle, on affinities that are not a rescaled cosine -----------------------
def gaussian_kernel(x):
  sq = np.sum(x * x, axis=1)
  d2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * x @ x.T, 0.0)
  return np.exp(-d2 / (2.0 * np.median(d2)))


def raw_cosine(x):
  xn = x / np.linalg.norm(x, axis=1)[:, None]
  a = xn @ xn.T
  return (a + a.T) / 2


def eigenvalue_error(w, ref, n):
  """The project's figure -- max |w - ref| / max(|ref|, 1e-12) over the consumed eigenvalues --
  for the values the reference resolves.  A Laplacian of an affinity with negative entries has an
  eigenvalue that is zero up to rounding among the consumed ones (the oracle's own dense solver
  returns -4e-17, 3e-18 or 8e-15 for it, depending on the Laplacian): no relative bar applies to
  a value that is rounding noise in the reference itself.  Such values -- |ref| below
  n * 2^-52 * max|ref| -- are held to an absolute 1e-10 instead, the constant the eigengap rule
  adds to every denominator, and reported separately."""
  noise = np.abs(ref) < n * 2.0 ** -52 * np.max(np.abs(ref))
  rel = np.max(np.abs(w - ref)[~noise] / np.maximum(np.abs(ref[~noise]), 1e-12))
  zero = float(np.max(np.abs(w[noise]))) if noise.any() else 0.0
  return float(rel), zero


ORACLE_CASES = [("gaussian", so.LAPLACIAN_GRAPH_CUT), ("raw_cosine", so.LAPLACIAN_NONE),
                ("raw_cosine", so.LAPLACIAN_GRAPH_CUT)]
LAPLACIANS = {so.LAPLACIAN_NONE: None, so.LAPLACIAN_GRAPH_CUT: sca.LaplacianType.GraphCut}


@pytest.fixture(scope="module")
def oracle_cases():
  """(name, laplacian) -> (affinity, config, oracle labels, oracle dump); computed once."""
  x = so.blobs(300, 32, 4, seed=41)
  matrices = {"gaussian": gaussian_kernel(x), "raw_cosine": raw_cosine(x)}
  cases = {}
  for name, lap in ORACLE_CASES:
    cfg = so.icassp2018_config(laplacian_type=lap, max_clusters=7)
    dump = {}
    a = matrices[name]
    cases[name, lap] = (a, cfg, predict_from_affinity(a, cfg, dump=dump), dump)
  return cases


@pytest.mark.parametrize("name,lap", ORACLE_CASES)
def test_predict_affinity_against_the_oracle_on_other_affinities(oracle_cases, name, lap):
  a, cfg, want, dump = oracle_cases[name, lap]
  descend = lap == so.LAPLACIAN_NONE
  if name == "raw_cosine":
    assert (a < 0).mean() > 0.1  # negative entries reach CropDiagonal, the cut, the Laplacian
  assert eigengap_margin(dump["eigenvalues"], cfg, descend) > 0.05  # no near tie
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=7, refinement_options=icassp_options(),
                            laplacian_type=LAPLACIANS[lap])
  idx = so.consumed_eigen_indices(a.shape[0], 7, descend, dump["eigenvalues"], 1e-2)
  ref = dump["eigenvalues"][idx]
  for affinity in (a, torch.from_numpy(a).cuda()):
    got = c.predict_affinity(affinity)
    assert so.adjusted_rand_index(got, want) == 1.0
    rel, zero = eigenvalue_error(c.consumed_eigenvalues()[idx], ref, a.shape[0])
    print("%s, laplacian %d: eigenvalue relative error %.3g, |zero eigenvalue| %.3g"
          % (name, lap, rel, zero))
    assert rel < 1e-5 and zero < 1e-10


def test_crop_diagonal_of_a_row_of_negative_values_is_zero_as_in_the_reference():
  """The reference takes the row maximum AFTER the diagonal is set to 0: a row whose other
  entries are all negative gets 0, not its largest negative value."""
  a = raw_cosine(so.blobs(200, 32, 3, seed=42))
  a[17, :] = a[:, 17] = -np.abs(a[17, :])
  a[17, 17] = 1.0
  assert np.all(np.delete(a[17], 17) < 0) and so.crop_diagonal(a)[17, 17] == 0.0
  cfg = so.icassp2018_config(laplacian_type=so.LAPLACIAN_GRAPH_CUT, max_clusters=7)
  dump = {}
  predict_from_affinity(a, cfg, dump=dump)
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=7, refinement_options=icassp_options(),
                            laplacian_type=sca.LaplacianType.GraphCut)
  c.predict_affinity(torch.from_numpy(a).cuda())
  idx = so.consumed_eigen_indices(200, 7, False, dump["eigenvalues"], 1e-2)
  rel, zero = eigenvalue_error(c.consumed_eigenvalues()[idx], dump["eigenvalues"][idx], 200)
  print("negative row: eigenvalue relative error %.3g, |zero eigenvalue| %.3g" % (rel, zero))
  assert rel < 1e-5 and zero < 1e-10


# --- stream ordering --------------------------------------------------------------------------
def test_a_pending_write_on_another_stream_is_ordered_before_the_ingest():
  a = torch.from_numpy(so.affinity(so.blobs(400, 64, 4, seed=77)).astype(np.float32))
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=7, refinement_options=icassp_options(),
                            laplacian_type=sca.LaplacianType.GraphCut)
  want = c.predict_affinity(a.numpy())
  staged = a.cuda()
  t = torch.zeros_like(staged)
  big = torch.empty(1 << 30, dtype=torch.float32, device="cuda")  # 4 GiB: a fill takes a while
  torch.cuda.synchronize()
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    big.fill_(1.0)
    big.fill_(2.0)
    t.copy_(staged)              # queued behind the fill, not yet done when the call is made
    got = c.predict_affinity(t)  # no synchronisation by the caller
    kept = t.clone()
    del t                        # the library is done with it
  torch.cuda.synchronize()
  assert np.array_equal(got, want)
  assert torch.equal(kept.cpu(), a)  # the source was only read
  assert np.array_equal(c.predict_affinity(staged), want)  # ... the same after a synchronise


# --- the raw C ABI ----------------------------------------------------------------------------
def test_descriptors_that_are_not_square_or_not_valid_are_refused_before_any_launch(handle):
  lib = handle.lib
  a = so.affinity(so.blobs(50, 8, 2, seed=3))
  out = np.full((50, matrix_ld(50)), -7.0)
  flag = ctypes.c_int(-1)
  good = dict(data=a.ctypes.data, dtype=_lib.SC_DTYPE_F64, location=_lib.SC_MEM_HOST, rows=50,
              cols=50, row_stride=50, col_stride=1)
  for bad in (dict(cols=49), dict(rows=49), dict(data=None), dict(dtype=4), dict(location=2),
              dict(row_stride=-50), dict(location=_lib.SC_MEM_DEVICE)):
    arr = _lib.ScArray(**dict(good, **bad))
    assert lib.sc_stage_affinity_ingest(handle.raw, ctypes.byref(arr), _lib.as_double_p(out),
                                        ctypes.byref(flag)) == _lib.SC_ERR_INVALID, bad
    assert lib.sc_set_affinity_array(handle.raw, ctypes.byref(arr)) == _lib.SC_ERR_INVALID, bad
    assert handle.last_error()
  assert np.all(out == -7.0) and flag.value == -1  # nothing ran
  ok = _lib.ScArray(**good)
  handle.check(lib.sc_stage_affinity_ingest(handle.raw, ctypes.byref(ok), _lib.as_double_p(out),
                                            ctypes.byref(flag)))
  assert np.array_equal(out[:, :50], a) and flag.value == 1
  handle.check(lib.sc_synchronize(handle.raw))
  torch.cuda.synchronize()
