"""GPU: a dense constraint matrix taken where it is (`DenseConstraints`): single calls, the dense
last stage of the grouped ConstraintPropagation chain, and batches that carry dense constraints
inside the library call.

Widening fp32 / fp16 / bf16 to fp64 is exact, so a single call on `DenseConstraints(q)` is compared
bit for bit with the same call on the widened float64 ndarray, which takes the host route
(`sc_set_constraint`).  The grouped chain is compared with the CPU oracle under the single route's
`CP_TOL` / `max_err` (test_gpu_constraints.py); batches with per-utterance `predict(u, c)`.
A narrow constraint is generated in float64 and cast; the cast value widened back is the
reference input.  The symmetric constraints hold +1 / -1 on a third of all pairs and a few
fractional weights: more than n entries, which no entry-list route could have served."""

import copy
import ctypes
import functools
import warnings

import numpy as np
import pytest
# (at module level on purpose: PyTorch has to be in the process before the library is loaded,
#  so that both use one HIP runtime -- INTEGRATION.md section 6)
import torch

import spectral_oracle as so
from test_gpu_constraints import CP_TOL, max_err, toy_refinement

import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import constraint as con

pytestmark = pytest.mark.gpu

DTYPES = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
LAYOUTS = ("contiguous", "every_other_column", "transposed", "device")
SINGLE_SIZES = (1, 2, 17, 64, 65, 129, 300)


def same_bits(a, b):
  a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
  return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@functools.lru_cache(maxsize=None)
def problem(n, d=16, noise=0.3):
  """(embeddings, truth, turn scores, affinity) of size n; computed once, never written."""
  if n > 2:
    x, truth, scores = so.turn_blobs(n, d, 3, seed=900 + n, noise=noise)
  else:
    x, truth, scores = so.blobs(n, 4, 1, seed=n), np.zeros(n, dtype=np.int64), np.zeros(n)
  x = np.ascontiguousarray(x)
  a = so.affinity(x)
  for m in (x, a):
    m.setflags(write=False)
  return x, truth, scores, a


def dense_q(n, seed=0, symmetric=True, truth=None):
  """A dense constraint for problem(n): on a third of all pairs +1 (same speaker) / -1 (another),
  a few of them with fractional weights (0.3 and 0.7 round in the narrow dtypes); K > n entries
  for n >= 17.  `symmetric` False: the lower triangle is drawn on its own."""
  truth = problem(n)[1] if truth is None else truth
  rng = np.random.default_rng(7000 + 13 * n + seed)
  sign = np.where(truth[:, None] == truth[None, :], 1.0, -1.0)
  weight = rng.choice([1.0, 1.0, 1.0, 0.5, 0.3, 0.7], size=(n, n))
  q = np.where(rng.random((n, n)) < 1.0 / 3.0, sign * weight, 0.0)
  if symmetric:
    q = np.triu(q) + np.triu(q, 1).T
  elif n > 1:
    q[0, n - 1], q[n - 1, 0] = 1.0, -0.5  # (whatever was drawn: not symmetric)
    assert not np.array_equal(q, q.T)
  if n >= 17:
    assert np.count_nonzero(q) > n
  return q


def forms(q64, dtype_name, layout):
  """`q64` cast to the dtype and laid out as `layout` says -> (object to wrap, its value widened
  to float64).  Host objects are NumPy arrays (views of the torch memory) except bfloat16, which
  NumPy does not have: a CPU tensor, through DLPack."""
  dtype = DTYPES[dtype_name]
  t = torch.from_numpy(np.array(q64)).to(dtype)
  n = t.shape[0]
  value = t.double().numpy()
  if layout == "every_other_column":
    base = torch.full((n, 2 * n), 3.0, dtype=dtype)
    base[:, ::2] = t
    obj = base[:, ::2]
  elif layout == "transposed":
    obj = t.t().contiguous().t()
  elif layout == "device":
    return t.to("cuda"), value
  else:
    obj = t.clone()
  if dtype is not torch.bfloat16:
    obj = obj.numpy()
  return obj, value


def info(handle):
  kind, n = ctypes.c_int(-1), ctypes.c_int(-1)
  dense_bytes = ctypes.c_size_t(0)
  handle.check(handle.lib.sc_constraint_info(handle.raw, ctypes.byref(kind), ctypes.byref(n), None,
                                             ctypes.byref(dense_bytes)))
  return kind.value, n.value, dense_bytes.value


def matrix_ld(n):
  ld = (n + 15) // 16 * 16
  return ld + 16 if ld % 512 == 0 else ld


# --- 1. single calls, bit for bit ----------------------------------------------------------------
@pytest.mark.parametrize("n", SINGLE_SIZES)
def test_adjust_affinity_equals_the_host_route_bit_for_bit(n):
  a = problem(n)[3]
  operators = (con.ConstraintPropagation(0.4), con.AffinityIntegration(con.IntegrationType.Max),
               con.AffinityIntegration(con.IntegrationType.Average))
  checked = 0
  for symmetric in (True, False):
    q64 = dense_q(n, symmetric=symmetric)
    for dtype_name in DTYPES:
      for layout in LAYOUTS:
        obj, value = forms(q64, dtype_name, layout)
        assert dtype_name != "f64" or np.array_equal(value, q64)
        for op in operators:
          got = op.adjust_affinity(a, sca.DenseConstraints(obj))
          want = op.adjust_affinity(a, value)
          assert same_bits(got, want), (n, symmetric, dtype_name, layout, type(op).__name__)
          checked += 1
  assert checked == 96
  # ... and the operator is the oracle's
  q64 = dense_q(n)
  got = con.ConstraintPropagation(0.4).adjust_affinity(a, sca.DenseConstraints(q64))
  assert max_err(got, so.constraint_propagation(a, q64, 0.4)) < CP_TOL


def cp_clusterer():
  return copy.deepcopy(sca.configs.turntodiarize_clusterer)


def ai_after_clusterer():
  return sca.SpectralClusterer(
      min_clusters=2, max_clusters=7, refinement_options=toy_refinement(),
      constraint_options=sca.ConstraintOptions(
          constraint_name=sca.ConstraintName.AffinityIntegration, apply_before_refinement=False,
          integration_type=sca.IntegrationType.Max),
      laplacian_type=sca.LaplacianType.GraphCut, row_wise_renorm=True)


# Sizes at which predict() itself cannot cluster, with or without the wrapper: the Turn-to-Diarize
# preset's AutoTune search finds no candidate on one or two rows (its proxy divides by a zero
# max_delta_norm and the search returns nothing: a TypeError, as in the reference), and
# min_clusters = 2 exceeds the one eigenvector of a single row.  There both routes must raise the
# same error; everywhere else they must agree bit for bit.
PREDICT_RAISES = {("ttd", 1), ("ttd", 2), ("integ-after", 1)}


def outcome(clusterer, x, constraint):
  try:
    with warnings.catch_warnings():
      # (AutoTune's proxy on one or two rows divides by a zero max_delta_norm: see above)
      warnings.simplefilter("ignore", RuntimeWarning)
      labels = clusterer.predict(x, constraint)
  except Exception as e:  # pylint: disable=broad-except
    return "raises", type(e), str(e)
  return "ok", labels, clusterer.consumed_eigenvalues()


@pytest.mark.parametrize("name", ["ttd", "integ-after"])
@pytest.mark.parametrize("n", SINGLE_SIZES)
def test_predict_equals_predict_on_the_widened_ndarray_bit_for_bit(n, name):
  """Every size x dtype x layout of the single-call grid, on the Turn-to-Diarize preset and on
  AffinityIntegration after refinement: labels and consumed eigenvalues are those of predict() on
  the widened float64 ndarray, bit for bit -- or, at the sizes of PREDICT_RAISES, its error."""
  make = {"ttd": cp_clusterer, "integ-after": ai_after_clusterer}[name]
  x = problem(n)[0]
  q64 = dense_q(n)
  checked = 0
  for dtype_name in DTYPES:
    for layout in LAYOUTS:
      obj, value = forms(q64, dtype_name, layout)
      wrapped, plain = make(), make()
      got = outcome(wrapped, x, sca.DenseConstraints(obj))
      want = outcome(plain, x, value)
      where = (n, name, dtype_name, layout)
      assert got[0] == want[0] == ("raises" if (name, n) in PREDICT_RAISES else "ok"), (
          where, got, want)
      if got[0] == "raises":
        assert got[1:] == want[1:], where  # the same exception type and message
      else:
        np.testing.assert_array_equal(got[1], want[1], err_msg=str(where))
        assert same_bits(got[2], want[2]), where
        assert getattr(wrapped, "last_best_p", None) == getattr(plain, "last_best_p", None)
        kind, qn, dense_bytes = info(wrapped._handle())
        assert (kind, qn) == (1, n) and dense_bytes >= n * matrix_ld(n) * 8
      checked += 1
  assert checked == 16
  # without constraint_options the wrapper is inert, like every other constraint
  if n >= 17:
    bare = sca.SpectralClusterer(min_clusters=2, max_clusters=7,
                                 refinement_options=toy_refinement())
    np.testing.assert_array_equal(bare.predict(x, sca.DenseConstraints(q64)), bare.predict(x))


def test_predict_affinity_and_compute_eigenvectors_take_the_wrapper():
  n = 129
  x, _, _, a = problem(n)
  q64 = dense_q(n)
  obj, value = forms(q64, "f32", "device")
  c = ai_after_clusterer()
  got = c.predict_affinity(torch.from_numpy(np.array(a)).to("cuda"), sca.DenseConstraints(obj))
  w = c.consumed_eigenvalues()
  np.testing.assert_array_equal(got, c.predict_affinity(a, value))
  assert same_bits(w, c.consumed_eigenvalues())
  _, k1, delta1 = c._compute_eigenvectors_ncluster(a, sca.DenseConstraints(obj))
  _, k2, delta2 = c._compute_eigenvectors_ncluster(a, value)
  assert (k1, delta1) == (k2, delta2)
  with pytest.raises(ValueError, match="same shape"):
    c.predict(x, sca.DenseConstraints(dense_q(65)))


def test_state_does_not_leak_between_constraint_forms():
  n = 129
  x, _, scores, _ = problem(n)
  obj, _ = forms(dense_q(n), "f16", "device")
  # (no AutoTune here: its search leaves p_percentile where it ended, so two identical calls on
  #  one clusterer object need not evaluate the same values)
  c = batch_clusterer(CP_BEFORE)
  first = c.predict(x, sca.DenseConstraints(obj))
  first_w = c.consumed_eigenvalues()
  assert info(c._handle())[0] == 1
  c.predict(x, sca.ConstraintMatrix(list(scores), 1))
  assert info(c._handle())[0] == 2
  c.predict(x)
  assert info(c._handle())[0] == 0
  again = c.predict(x, sca.DenseConstraints(obj))
  np.testing.assert_array_equal(again, first)
  assert same_bits(c.consumed_eigenvalues(), first_w)
  assert info(c._handle())[:2] == (1, n)


# --- 2. the grouped chain against the oracle -----------------------------------------------------
def run_dense_group(ns, alpha, idle=()):
  count = len(ns)
  cfg = _lib.ScConfig()
  _lib.load().sc_config_default(cfg)
  cfg.constraint_name = sca.ConstraintName.ConstraintPropagation.value
  cfg.constraint_before_refinement = 1
  cfg.constraint_alpha = float(alpha)
  affs = [np.array(problem(n)[3]) if n else np.zeros((0, 0)) for n in ns]
  qs = [np.ascontiguousarray(dense_q(n, seed=z)) if n else np.zeros((0, 0))
        for z, n in enumerate(ns)]
  outs = [np.full((n, n) if n else (3, 3), -7.0) for n in ns]
  dp = ctypes.POINTER(ctypes.c_double)
  ap = (dp * count)(*[_lib.as_double_p(a) if a.size else None for a in affs])
  qp = (dp * count)(*[_lib.as_double_p(q) if q.size and z not in idle else None
                      for z, q in enumerate(qs)])
  op = (dp * count)(*[_lib.as_double_p(o) for o in outs])
  handle = _lib.default_handle()
  handle.check(handle.lib.sc_stage_constraint_dense_group(
      handle.raw, cfg, count, (ctypes.c_int32 * count)(*ns), ap, qp, op))
  return outs, affs, qs


@pytest.mark.parametrize("alpha", [0.4, 0.6])
@pytest.mark.parametrize("ns", [(300, 129, 0, 257, 130), (1, 2, 17, 128), tuple(range(129, 145))],
                         ids=["mixed", "small", "sixteen"])
def test_grouped_dense_chain_vs_oracle(ns, alpha):
  outs, affs, qs = run_dense_group(ns, alpha)
  for z, n in enumerate(ns):
    if n == 0:
      assert np.all(outs[z] == -7.0)  # idle: its output is untouched
      continue
    assert not np.isnan(outs[z]).any()  # (the padding was NaN: nothing outside a matrix was read)
    err = max_err(outs[z], so.constraint_propagation(affs[z], qs[z], alpha))
    single = con.ConstraintPropagation(alpha).adjust_affinity(affs[z], qs[z])
    print("n=%d alpha=%g grouped vs oracle %.3e; vs the single route: max |diff| %.3e" % (
        n, alpha, err, float(np.max(np.abs(outs[z] - single)))))
    assert err < CP_TOL
    # Every size here is <= 512, where the single route's GEMMs take whole-K tiles as the grouped
    # ones always do (gemm_f64.hip launch_variant), and the full-output product runs the tile body
    # of the single route's T Q^T: the chain's result is the single route's, bit for bit.
    assert same_bits(outs[z], single), "n=%d alpha=%g" % (n, alpha)
    # symmetric up to the rounding of (d_i a_ij) d_j vs (d_j a_ji) d_i: the dense suite's bound
    np.testing.assert_allclose(outs[z], outs[z].T, rtol=0, atol=1e-14)


def test_grouped_dense_chain_idle_members_and_refusals():
  outs, affs, qs = run_dense_group((40, 33, 0, 150), 0.4, idle=(1,))
  assert np.all(outs[1] == -7.0) and np.all(outs[2] == -7.0)
  for z in (0, 3):
    assert max_err(outs[z], so.constraint_propagation(affs[z], qs[z], 0.4)) < CP_TOL
  with pytest.raises(sca.UnsupportedOnDeviceError):
    run_dense_group((60,), 1.0)
  # the chain's dense stage is the symmetric one
  handle = _lib.default_handle()
  cfg = _lib.ScConfig()
  handle.lib.sc_config_default(cfg)
  cfg.constraint_name = sca.ConstraintName.ConstraintPropagation.value
  cfg.constraint_before_refinement = 1
  a, q, out = np.array(problem(40)[3]), dense_q(40, symmetric=False), np.full((40, 40), -7.0)
  dp = ctypes.POINTER(ctypes.c_double)
  assert handle.lib.sc_stage_constraint_dense_group(
      handle.raw, cfg, 1, (ctypes.c_int32 * 1)(40), (dp * 1)(_lib.as_double_p(a)),
      (dp * 1)(_lib.as_double_p(q)), (dp * 1)(_lib.as_double_p(out))) == _lib.SC_ERR_INVALID
  assert np.all(out == -7.0)


# --- 3. batches -------------------------------------------------------------------------------
BATCH_SIZES = (40, 100, 128, 129, 200, 300, 450, 700)
BATCH_ROUTES = [2, 2, 2, 1, 1, 1, 1, 1]
ASYMMETRIC = 4  # (the utterance of n = 200 carries an asymmetric dense constraint)
CP_BEFORE = (sca.ConstraintName.ConstraintPropagation, True)
CP_AFTER = (sca.ConstraintName.ConstraintPropagation, False)
AI_AFTER = (sca.ConstraintName.AffinityIntegration, False)


def batch_clusterer(variant):
  name, before = variant
  options = toy_refinement()
  options.p_percentile = 0.9
  return sca.SpectralClusterer(
      min_clusters=2, max_clusters=7, refinement_options=options,
      laplacian_type=sca.LaplacianType.GraphCut, row_wise_renorm=True,
      constraint_options=sca.ConstraintOptions(
          constraint_name=name, apply_before_refinement=before,
          integration_type=sca.IntegrationType.Max, constraint_propagation_alpha=0.4))


def oracle_config(variant):
  name, before = variant
  return so.turntodiarize_config(
      min_clusters=2, max_clusters=7, p_percentile=0.9, constraint_name=name.value,
      apply_before_refinement=before, integration_type=so.INTEGRATION_MAX,
      constraint_propagation_alpha=0.4)


def batch_problem(n):
  """Well-separated speakers (d = 32, noise 0.2): the oracle's labels are the truth for every size,
  operator and constraint form below (test_predict_batch_... checks it), so that label equality
  between two device routes is no coin toss."""
  return problem(n, 32, 0.2)


def batch_inputs():
  """Utterances and one constraint each: DenseConstraints as host f64 / host f32 / device f16,
  a ConstraintMatrix, a PairwiseConstraints and None mixed over both routes; each with the dense
  float64 matrix it stands for (None: no constraint)."""
  us, cs, dense = [], [], []
  for i, n in enumerate(BATCH_SIZES):
    x, truth, scores, _ = batch_problem(n)
    us.append(x)
    q64 = dense_q(n, seed=i, symmetric=i != ASYMMETRIC, truth=truth)
    kind = ("f64", "f32", "f16-device", "band", "f64", "pairs", "none", "f16-device")[i]
    if kind == "band":
      cm = sca.ConstraintMatrix(list(scores), 1)
      cs.append(cm), dense.append(cm.compute_diagonals())
    elif kind == "pairs":
      same = [(j, j + 2) for j in range(0, n - 2, 7) if truth[j] == truth[j + 2]]
      other = [(j, j + 2) for j in range(0, n - 2, 7) if truth[j] != truth[j + 2]]
      pc = sca.PairwiseConstraints(n, must_link=same, cannot_link=other)
      cs.append(pc), dense.append(pc.to_dense())
    elif kind == "none":
      cs.append(None), dense.append(None)
    else:
      obj, value = forms(q64, kind[:3], "device" if kind.endswith("device") else "contiguous")
      cs.append(sca.DenseConstraints(obj)), dense.append(value)
  return us, cs, dense


@pytest.mark.parametrize("variant", [CP_BEFORE, CP_AFTER, AI_AFTER],
                         ids=["cp-before", "cp-after", "integ-after"])
def test_predict_batch_with_dense_constraints_equals_per_call_predict(variant):
  us, cs, dense = batch_inputs()
  if variant == CP_BEFORE:
    # label equality is no coin toss: the oracle separates these inputs perfectly
    for i, n in enumerate(BATCH_SIZES):
      want = so.predict(us[i], oracle_config(variant), constraint_matrix=dense[i])
      assert so.adjusted_rand_index(want, batch_problem(n)[1]) == 1.0
  single = batch_clusterer(variant)
  want = [single.predict(u, c) for u, c in zip(us, cs)]
  batch = batch_clusterer(variant)
  got = batch.predict_batch(us, constraint_matrices=cs)
  routes = list(batch.last_batch_routes)
  print("routes:", routes)
  # The asymmetric member is inside the call too.  Before refinement the sequence symmetrises
  # what its operator leaves and it stays on its route; after refinement the adjusted matrix is
  # not symmetric and the member leaves the group for the general solver (route 0), as a member
  # with an asymmetric entry list does.
  expect = list(BATCH_ROUTES)
  if variant != CP_BEFORE:
    expect[ASYMMETRIC] = 0
  assert routes == expect
  for i, (g, w) in enumerate(zip(got, want)):
    np.testing.assert_array_equal(g, w, err_msg="utterance %d (n=%d)" % (i, BATCH_SIZES[i]))
  assert info(batch._handle())[0] == 0  # nothing stays resident
  again = batch.predict_batch(us, constraint_matrices=cs)
  assert list(batch.last_batch_routes) == routes
  for g, w in zip(again, got):
    np.testing.assert_array_equal(g, w)
  # a matrix of another n: predict()'s ValueError, before anything is launched
  wrong = list(cs)
  wrong[-1] = sca.DenseConstraints(np.eye(BATCH_SIZES[-1] + 1, dtype=np.float32))
  with pytest.raises(ValueError, match="same shape"):
    batch.predict_batch(us, constraint_matrices=wrong)


def test_predict_affinity_batch_with_dense_constraints_equals_per_call():
  us, cs, _ = batch_inputs()
  affinities = [torch.from_numpy(np.array(batch_problem(n)[3])).to(torch.float32).to("cuda")
                for n in BATCH_SIZES]
  single = batch_clusterer(CP_BEFORE)
  want = [single.predict_affinity(a, c) for a, c in zip(affinities, cs)]
  batch = batch_clusterer(CP_BEFORE)
  got = batch.predict_affinity_batch(affinities, cs)
  print("routes:", list(batch.last_batch_routes))
  assert list(batch.last_batch_routes) == BATCH_ROUTES
  for i, (g, w) in enumerate(zip(got, want)):
    np.testing.assert_array_equal(g, w, err_msg="affinity %d (n=%d)" % (i, BATCH_SIZES[i]))


def test_a_raw_ndarray_constraint_still_sends_the_batch_through_the_loop():
  us, cs, dense = batch_inputs()
  us, cs, dense = us[:4], list(cs[:4]), dense[:4]
  cs[1] = dense[1]  # a raw ndarray: today's behaviour
  batch = batch_clusterer(CP_BEFORE)
  got = batch.predict_batch(us, constraint_matrices=cs)
  assert list(batch.last_batch_routes) == [_lib.BATCH_ROUTE_SINGLE] * 4
  single = batch_clusterer(CP_BEFORE)
  for g, u, c in zip(got, us, cs):
    np.testing.assert_array_equal(g, single.predict(u, c))


# --- 4. errors before launch -------------------------------------------------------------------
def test_batch_entry_point_validates_every_dense_source_before_launch():
  n = 40
  x = np.array(problem(n)[0])
  q = np.ascontiguousarray(dense_q(n))
  clusterer = batch_clusterer(CP_BEFORE)
  handle = clusterer._handle()
  lib, cfg = handle.lib, clusterer.build_config()
  arrays = (_lib.ScArray * 2)()
  for arr in arrays:
    arr.data = x.ctypes.data
    arr.dtype, arr.location = _lib.SC_DTYPE_F64, _lib.SC_MEM_HOST
    arr.rows, arr.cols, arr.row_stride, arr.col_stride = n, x.shape[1], x.shape[1], 1
  dense = (_lib.ScArray * 2)()
  dense[1].data = q.ctypes.data
  dense[1].dtype, dense[1].location = _lib.SC_DTYPE_F64, _lib.SC_MEM_HOST
  dense[1].rows, dense[1].cols, dense[1].row_stride, dense[1].col_stride = n, n, n, 1
  labels = [np.full(n, -1, dtype=np.int64) for _ in range(2)]
  lp = (ctypes.POINTER(ctypes.c_int64) * 2)(*[_lib.as_int64_p(l) for l in labels])
  cons = (_lib.ScConstraintDesc * 2)()

  def call(group=16):
    return lib.sc_predict_batch_constraint_arrays(handle.raw, arrays, cons, dense, 2, cfg, lp,
                                                  None, group, 0)

  dense[1].rows = n - 1  # not square
  assert call() == _lib.SC_ERR_INVALID
  dense[1].rows, dense[1].cols = n - 1, n - 1  # square, but not the utterance's n
  assert call() == _lib.SC_ERR_INVALID
  dense[1].rows, dense[1].cols = n, n
  dense[1].dtype = 17  # unknown dtype
  assert call() == _lib.SC_ERR_INVALID
  dense[1].dtype = _lib.SC_DTYPE_F64
  band = np.zeros(n - 1)
  cons[1].kind, cons[1].band = 2, _lib.as_double_p(band)  # both a dense source and a kind
  assert call() == _lib.SC_ERR_INVALID
  cons[1].kind = 0
  assert call(group=1) == _lib.SC_ERR_INVALID  # the grouped form only
  assert all((l == -1).all() for l in labels)
  handle.check(call())
  assert all((l >= 0).all() for l in labels)
  assert list(clusterer_routes(handle, 2)) == [2, 2]
  # dense == NULL: exactly the existing call
  for l in labels:
    l[:] = -1
  handle.check(lib.sc_predict_batch_constraint_arrays(handle.raw, arrays, None, None, 2, cfg, lp,
                                                      None, 16, 0))
  assert all((l >= 0).all() for l in labels)


def clusterer_routes(handle, count):
  routes = (ctypes.c_int32 * count)()
  handle.check(handle.lib.sc_last_batch_routes(handle.raw, routes, count))
  return routes
