"""GPU: a constraint matrix given as must-link / cannot-link pairs (`PairwiseConstraints`,
`sc_set_constraint_pairs`).  The K directed entries travel, 16 bytes each; ConstraintPropagation
forms T Q T = U V^T from two (n, round_up(K, 16)) panels inside the kernel that adjusts A
(`k_cp_pair_panels`, `k_cp_pairs_adjust`) while K <= n and scatters the entries into the dense
buffer on the device above that (`k_pairs_to_dense`); AffinityIntegration patches K entries.

Reference of every check: the CPU oracle fed the DENSE matrix `pc.to_dense()`
(`so.constraint_propagation`, `np.maximum`, `0.5 * (a + q)`).  `CP_TOL` and `max_err` are the
dense suite's (test_gpu_constraints.py: condition number of I - alpha A_norm; the stage that sets
it, the Neumann chain, is the dense route's); AffinityIntegration is elementwise, hence bit-exact.
"""

import copy
import ctypes

import numpy as np
import pytest

import spectral_oracle as so
from conftest import golden
from test_gpu_constraints import CP_TOL, max_err, toy_refinement

import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import constraint as con

pytestmark = pytest.mark.gpu


def info(handle):
  kind, n, count = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
  band_bytes, dense_bytes, pair_bytes = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
  handle.check(handle.lib.sc_constraint_info(
      handle.raw, ctypes.byref(kind), ctypes.byref(n), ctypes.byref(band_bytes),
      ctypes.byref(dense_bytes)))
  handle.check(handle.lib.sc_constraint_pairs_info(handle.raw, ctypes.byref(count),
                                                   ctypes.byref(pair_bytes)))
  return kind.value, n.value, dense_bytes.value, count.value, pair_bytes.value


def affinity_of(n):
  x = so.turn_blobs(n, 16, 3, seed=n)[0] if n > 2 else so.blobs(n, 4, 1, seed=n)
  return so.affinity(x)


def make_pairs(n, k, seed=0):
  """A `PairwiseConstraints` of exactly `k` directed entries: a diagonal entry when k is odd, then
  k // 2 pairs.  The entries touch row 0 and row n - 1 (where k allows both: a single diagonal
  entry sits at n - 1), the first pair being {0, n - 1}; the rest is random, with must-link,
  cannot-link and weighted pairs mixed."""
  rng = np.random.default_rng(1000 * n + k + seed)
  pairs, values = [], []
  if k % 2:
    d = n - 1 if k == 1 else 0
    pairs.append((d, d))
    values.append(1.0 if k == 1 else -0.75)
  want = k // 2
  assert want <= n * (n - 1) // 2, "k does not fit in n"
  seen = set()
  if want:
    seen.add((0, n - 1))
  while len(seen) < want:
    i, j = sorted(int(v) for v in rng.integers(0, n, size=2))
    if i != j:
      seen.add((i, j))
  for i, j in sorted(seen, key=lambda p: (p != (0, n - 1), p)):
    pairs.append((j, i) if rng.integers(0, 2) else (i, j))
    values.append(float(rng.choice([1.0, -1.0, 0.5, -0.25])))
  pc = sca.PairwiseConstraints(n, pairs=np.array(pairs, dtype=np.int64).reshape(-1, 2),
                               values=np.array(values))
  assert len(pc.entries()[0]) == k
  return pc


def directed_counts(n):
  """0, one diagonal entry, 2, the panel padding's edge 15 / 16 / 17, and the route rule's edge
  n - 1 / n / n + 1 (n + 1: scatter + the dense stage) -- those that fit in an n x n matrix."""
  ks = sorted({0, 1, 2, 15, 16, 17, n - 1, n, n + 1})
  return [k for k in ks if 0 <= k <= n + 1 and k // 2 <= n * (n - 1) // 2 and
          (k % 2 == 0 or n >= 1)]


def stage_pairs(a, rows, cols, vals, alpha=None, integration=None):
  """sc_stage_constraint_pairs on explicit entry arrays (the C entry point takes asymmetric
  lists; the Python class never builds one)."""
  src = np.ascontiguousarray(a, dtype=np.float64)
  rows = np.ascontiguousarray(rows, dtype=np.int32)
  cols = np.ascontiguousarray(cols, dtype=np.int32)
  vals = np.ascontiguousarray(vals, dtype=np.float64)
  cfg = _lib.ScConfig()
  _lib.load().sc_config_default(cfg)
  cfg.constraint_before_refinement = 1
  if alpha is not None:
    cfg.constraint_name = sca.ConstraintName.ConstraintPropagation.value
    cfg.constraint_alpha = float(alpha)
  else:
    cfg.constraint_name = sca.ConstraintName.AffinityIntegration.value
    cfg.integration_type = integration.value
  out = np.empty_like(src)
  handle = _lib.default_handle()
  handle.check(handle.lib.sc_stage_constraint_pairs(
      handle.raw, cfg, _lib.as_double_p(src), _lib.as_int32_p(rows), _lib.as_int32_p(cols),
      _lib.as_double_p(vals), len(vals), src.shape[0], _lib.as_double_p(out)))
  return out


# --- ConstraintPropagation against the oracle ------------------------------------------------
@pytest.mark.parametrize("n,alpha", [(1, 0.6), (2, 0.6), (17, 0.4), (129, 0.6), (300, 0.4),
                                     (1000, 0.6)])
def test_constraint_propagation_pairs_vs_oracle(n, alpha):
  """Sizes at which a tile edge (64), the panel padding (16) or the GEMM's 128-tile changes; a
  symmetric affinity, so what the pair kernel writes must be EXACTLY symmetric (the handle then
  marks the adjusted affinity symmetric and later kernels read one triangle)."""
  a = affinity_of(n)
  assert np.array_equal(a, a.T)
  op = con.ConstraintPropagation(alpha)
  ks = directed_counts(n)
  assert ks[0] == 0 and (n < 2 or n + 1 in ks)
  for k in ks:
    pc = make_pairs(n, k)
    rows, _, _ = pc.entries()
    if k >= 2:
      assert 0 in rows and n - 1 in rows
    got = op.adjust_affinity(a, pc)
    err = max_err(got, so.constraint_propagation(a, pc.to_dense(), alpha))
    print("n=%d alpha=%g K=%d (%s) vs oracle: %.3e" % (
        n, alpha, k, "pairs" if k <= n else "scatter + dense", err))
    assert err < CP_TOL
    if k <= n:
      assert np.array_equal(got, got.T), "K=%d" % k
    else:
      # the dense stage, unchanged: its diagonal GEMM tiles are symmetric up to rounding only
      # (the bound of test_gpu_constraints.py::test_ops_vs_reference_golden)
      print("K=%d dense side: max |out - out^T| %.3e" % (k, float(np.max(np.abs(got - got.T)))))
      np.testing.assert_allclose(got, got.T, rtol=0, atol=1e-14)
    if k == 0:
      assert np.array_equal(got, a)
    elif n > 1:  # (n = 1: a = [[1]] is a fixed point of the adjustment)
      assert not np.array_equal(got, a)  # the entries did something


def test_constraint_propagation_pairs_alpha_zero_and_unsupported_alpha():
  a = affinity_of(60)
  pc = make_pairs(60, 17)
  # alpha = 0: T = I, F = Q
  got = con.ConstraintPropagation(0.0).adjust_affinity(a, pc)
  assert max_err(got, so.constraint_propagation(a, pc.to_dense(), 0.0)) < 1e-15
  for k in (17, 0, 62):  # (refused whichever side of the route rule, and before Q = 0 returns)
    with pytest.raises(sca.UnsupportedOnDeviceError):
      con.ConstraintPropagation(1.0).adjust_affinity(a, make_pairs(60, k))


@pytest.mark.parametrize("alpha", [0.4, 0.6])
def test_constraint_propagation_pairs_general_affinity_and_asymmetric_list(alpha):
  """A non-symmetric affinity (U is built from T^T, every tile is computed), with a symmetric
  list, an asymmetric one on the pair side (K = 23 <= 40) and one on the dense side (K = 57)."""
  a = golden("constraint_ops_n40.npz")["a_gen"]
  n = a.shape[0]
  assert not np.array_equal(a, a.T)
  pc = make_pairs(n, 17)
  got = con.ConstraintPropagation(alpha).adjust_affinity(a, pc)
  assert max_err(got, so.constraint_propagation(a, pc.to_dense(), alpha)) < CP_TOL
  rng = np.random.default_rng(40)
  sym_a = affinity_of(n)
  for k in (23, 57):
    at = rng.choice(n * n, size=k, replace=False)
    rows, cols = at // n, at % n
    rows[0], cols[0], rows[1], cols[1] = 0, n - 1, n - 1, 3  # (unless drawn already: see below)
    assert len(set(zip(rows.tolist(), cols.tolist()))) == k
    vals = rng.choice([1.0, -1.0, 0.5], size=k)
    q = np.zeros((n, n))
    q[rows, cols] = vals
    assert not np.array_equal(q, q.T)
    for src in (a, sym_a):
      got = stage_pairs(src, rows, cols, vals, alpha=alpha)
      err = max_err(got, so.constraint_propagation(src, q, alpha))
      print("asymmetric list K=%d, symmetric affinity %s, alpha=%g: %.3e" % (
          k, src is sym_a, alpha, err))
      assert err < CP_TOL


def test_constraint_propagation_pairs_is_deterministic():
  for n, k in ((300, 17), (300, 300), (129, 130)):
    a = affinity_of(n)
    pc = make_pairs(n, k)
    first = con.ConstraintPropagation(0.4).adjust_affinity(a, pc)
    again = con.ConstraintPropagation(0.4).adjust_affinity(a, pc)
    assert np.array_equal(first, again)


def test_band_written_as_pairs():
  """The speaker-turn band as a ConstraintMatrix and as the equivalent PairwiseConstraints: the
  whole band has K = 2 (non-zeros) > n and takes the dense side, a thinned band the pair side."""
  n, alpha = 300, 0.4
  x, _, scores = so.turn_blobs(n, 16, 3, seed=n)
  a = so.affinity(x)
  band = sca.ConstraintMatrix(list(scores), 1).band()
  at = np.flatnonzero(band)
  assert 2 * len(at) > n
  for keep, side in ((at, "dense"), (at[::3], "pairs")):
    thin = np.zeros_like(band)
    thin[keep] = band[keep]
    # the turn scores that give this band: no turn (+1), a confident one (-1), a weak one (0)
    cm = sca.ConstraintMatrix([0.0] + [{1.0: 0.0, -1.0: 2.0, 0.0: 0.5}[b] for b in thin], 1)
    assert np.array_equal(cm.band(), thin)
    pc = sca.PairwiseConstraints(n, pairs=np.stack([keep, keep + 1], axis=1), values=band[keep])
    assert np.array_equal(pc.to_dense(), cm.compute_diagonals())
    k = len(pc.entries()[0])
    assert (k > n) == (side == "dense")
    want = so.constraint_propagation(a, pc.to_dense(), alpha)
    got_band = con.ConstraintPropagation(alpha).adjust_affinity(a, cm)
    got_pairs = con.ConstraintPropagation(alpha).adjust_affinity(a, pc)
    print("band as pairs, K=%d (%s side): band %.3e pairs %.3e" % (
        k, side, max_err(got_band, want), max_err(got_pairs, want)))
    assert max_err(got_band, want) < CP_TOL
    assert max_err(got_pairs, want) < CP_TOL


# --- AffinityIntegration -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 40, 300, 1000])
def test_affinity_integration_pairs_is_bit_exact(n):
  a = affinity_of(n)
  pc = make_pairs(n, min(n + 1, 41) if n > 2 else n)
  rows, cols, _ = pc.entries()
  if n >= 40:
    a[rows[1], cols[1]] = np.nan      # on a constrained entry (its twin keeps its value)
    a[rows[5], cols[5]] = -0.0        # signed zero under an entry
    free = np.argwhere(pc.to_dense() == 0)
    a[tuple(free[7])] = np.nan        # off the entries
    a[tuple(free[11])] = -0.0
  q = pc.to_dense()
  for kind, want in ((con.IntegrationType.Max, np.maximum(a, q)),
                     (con.IntegrationType.Average, 0.5 * (a + q))):
    got = con.AffinityIntegration(kind).adjust_affinity(a, pc)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(np.isnan(got), np.isnan(a))
    # the dense route, bit for bit (signs of zero included)
    dense = con.AffinityIntegration(kind).adjust_affinity(a, q)
    assert np.array_equal(got.view(np.int64), dense.view(np.int64))
  # no entries at all
  none = sca.PairwiseConstraints(n)
  got = con.AffinityIntegration(con.IntegrationType.Max).adjust_affinity(a, none)
  assert np.array_equal(got, np.maximum(a, 0.0), equal_nan=True)


# --- the grouped stage entry ---------------------------------------------------------------------
def run_pair_group(ns, ks, alpha):
  count = len(ns)
  cfg = _lib.ScConfig()
  _lib.load().sc_config_default(cfg)
  cfg.constraint_name = sca.ConstraintName.ConstraintPropagation.value
  cfg.constraint_before_refinement = 1
  cfg.constraint_alpha = float(alpha)
  affs = [np.ascontiguousarray(affinity_of(n)) if n else np.zeros((0, 0)) for n in ns]
  pcs = [make_pairs(n, k, seed=z) if n else None for z, (n, k) in enumerate(zip(ns, ks))]
  ents = [pc.entries() if pc is not None else None for pc in pcs]
  # (an idle member gets an output buffer too: it must stay as it is)
  outs = [np.full((n, n) if n else (3, 3), -7.0) for n in ns]
  dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
  ap = (dp * count)(*[_lib.as_double_p(a) if a.size else None for a in affs])
  rp = (ip * count)(*[_lib.as_int32_p(e[0]) if e else None for e in ents])
  cp = (ip * count)(*[_lib.as_int32_p(e[1]) if e else None for e in ents])
  vp = (dp * count)(*[_lib.as_double_p(e[2]) if e else None for e in ents])
  op = (dp * count)(*[_lib.as_double_p(o) if o.size else None for o in outs])
  handle = _lib.default_handle()
  handle.check(handle.lib.sc_stage_constraint_pairs_group(
      handle.raw, cfg, count, (ctypes.c_int32 * count)(*ns), ap, rp, cp, vp,
      (ctypes.c_int32 * count)(*ks), op))
  return outs, affs, pcs


def test_grouped_pair_stage_equals_the_single_stage_bit_for_bit():
  """16 members of mixed size.  Every live size here is <= 512, where the single route's GEMMs
  take whole-K tiles (gemm_f64.hip launch_variant: K <= 512 and less than one wave of tiles is
  never split) as the grouped ones always do: the chain's T is the same, and the pair stage is one
  tile body with a fixed K order -- so n = 2, 17, 129 and 300 are all the bit-equal case.  The
  device memory of the entry point is NaN-filled: nothing outside a matrix or a list is read."""
  ns = [300, 2, 0, 17, 129, 17, 300, 0, 129, 2, 17, 129, 300, 2, 17, 129]
  ks = [16, 2, 0, 17, 129, 0, 300, 0, 15, 1, 1, 128, 17, 2, 16, 2]
  alpha = 0.4
  outs, affs, pcs = run_pair_group(ns, ks, alpha)
  for z, n in enumerate(ns):
    if n == 0:
      assert np.all(outs[z] == -7.0)  # idle: its output is untouched
      continue
    assert not np.isnan(outs[z]).any()
    want = so.constraint_propagation(affs[z], pcs[z].to_dense(), alpha)
    err = max_err(outs[z], want)
    single = con.ConstraintPropagation(alpha).adjust_affinity(affs[z], pcs[z])
    print("member %d n=%d K=%d grouped vs oracle %.3e; bit-equal to the single stage: %s" % (
        z, n, ks[z], err, np.array_equal(outs[z], single)))
    assert err < CP_TOL
    assert np.array_equal(outs[z], single)
    assert np.array_equal(outs[z], outs[z].T)
    if ks[z] == 0:
      assert np.array_equal(outs[z], affs[z])
  handle = _lib.default_handle()
  # more entries than n is the dense route: not grouped
  with pytest.raises(sca.UnsupportedOnDeviceError):
    run_pair_group([17], [18], alpha)
  with pytest.raises(sca.UnsupportedOnDeviceError):
    run_pair_group([60], [4], 1.0)
  assert info(handle)[0] == 0


# --- state of the handle -------------------------------------------------------------------------
def test_pairs_only_handle_never_holds_a_dense_constraint(monkeypatch):
  n = 400
  x, _, _ = so.turn_blobs(n, 24, 4, seed=n + 1, noise=1.0)
  device = _lib.default_handle().device
  fresh = _lib.Handle(device)
  monkeypatch.setitem(_lib._default_handles, device, fresh)
  try:
    assert info(fresh) == (0, 0, 0, 0, 0)
    clusterer = copy.deepcopy(sca.configs.turntodiarize_clusterer)
    assert clusterer._handle() is fresh
    pc = make_pairs(n, 16)
    clusterer.predict(x, pc)
    kind, qn, dense_bytes, count, pair_bytes = info(fresh)
    assert (kind, qn, count) == (3, n, 16)
    assert 16 * 16 <= pair_bytes <= 16 * n
    assert dense_bytes == 0
    con.AffinityIntegration(con.IntegrationType.Max).adjust_affinity(so.affinity(x),
                                                                     make_pairs(n, n + 1))
    assert info(fresh)[2] == 0  # AffinityIntegration takes the list whatever K is
    # pairs -> band -> pairs -> dense -> none
    clusterer.predict(x, sca.ConstraintMatrix([0.0] * n, 1))
    assert info(fresh)[:2] == (2, n) and info(fresh)[3] == 0
    clusterer.predict(x, pc)
    assert info(fresh)[:2] == (3, n)
    clusterer.predict(x, pc.to_dense())
    assert info(fresh)[:2] == (1, n) and info(fresh)[3] == 0
    clusterer.predict(x)
    assert info(fresh)[:2] == (0, 0)
  finally:
    monkeypatch.undo()
    fresh.close()


def test_pairs_do_not_leak_into_the_next_call():
  x, _, _ = so.turn_blobs(150, 16, 3, seed=3, noise=1.0)
  pc = make_pairs(150, 40)
  clusterer = sca.SpectralClusterer(
      min_clusters=2, max_clusters=7, refinement_options=toy_refinement(),
      constraint_options=copy.deepcopy(sca.configs.turntodiarize_constraint_options),
      laplacian_type=sca.LaplacianType.GraphCut, row_wise_renorm=True)
  first = clusterer.predict(x)
  clusterer.predict(x, pc)
  assert info(clusterer._handle())[0] == 3
  again = clusterer.predict(x)
  np.testing.assert_array_equal(first, again)
  assert info(clusterer._handle())[0] == 0
  clusterer.predict(x, pc)
  batch = clusterer.predict_batch([x, x], streams=1)
  np.testing.assert_array_equal(batch[0], first)
  np.testing.assert_array_equal(batch[1], first)
  # without constraint_options a PairwiseConstraints is inert, like a dense matrix
  plain = sca.SpectralClusterer(
      min_clusters=2, max_clusters=7, refinement_options=toy_refinement(),
      laplacian_type=sca.LaplacianType.GraphCut, row_wise_renorm=True)
  np.testing.assert_array_equal(plain.predict(x, pc), first)


def test_pair_entry_point_errors():
  handle = _lib.default_handle()
  lib = handle.lib
  i32 = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
  f64 = lambda *v: np.array(v, dtype=np.float64)  # noqa: E731

  def set_pairs(rows, cols, vals, n):
    return lib.sc_set_constraint_pairs(handle.raw, _lib.as_int32_p(rows), _lib.as_int32_p(cols),
                                       _lib.as_double_p(vals), len(vals), n)

  handle.check(lib.sc_clear_constraint(handle.raw))
  assert set_pairs(i32(0, 5), i32(1, 0), f64(1, 1), 5) == _lib.SC_ERR_INVALID   # row = n
  assert set_pairs(i32(0, 1), i32(-1, 0), f64(1, 1), 5) == _lib.SC_ERR_INVALID  # col < 0
  assert set_pairs(i32(0, 1), i32(1, 0), f64(1, np.nan), 5) == _lib.SC_ERR_INVALID
  assert set_pairs(i32(0, 1), i32(1, 0), f64(np.inf, 1), 5) == _lib.SC_ERR_INVALID
  assert set_pairs(i32(0, 0), i32(1, 1), f64(1, 1), 5) == _lib.SC_ERR_INVALID   # one position twice
  assert set_pairs(i32(), i32(), f64(), 0) == _lib.SC_ERR_INVALID
  assert info(handle)[0] == 0  # a refused list leaves nothing resident
  handle.check(lib.sc_set_constraint_pairs(handle.raw, None, None, None, 0, 5))  # Q = 0
  assert info(handle)[:2] == (3, 5) and info(handle)[3] == 0
  handle.check(set_pairs(i32(0, 1, 2), i32(1, 0, 2), f64(1, 1, -1), 5))
  assert info(handle)[:2] == (3, 5) and info(handle)[3] == 3
  handle.check(lib.sc_clear_constraint(handle.raw))
  assert info(handle)[0] == 0 and info(handle)[3] == 0
  # the Python side: predict()'s ValueError for a list of another n
  x = so.blobs(50, 8, 2, seed=1)
  clusterer = copy.deepcopy(sca.configs.turntodiarize_clusterer)
  with pytest.raises(ValueError, match="same shape"):
    clusterer.predict(x, make_pairs(49, 8))
  with pytest.raises(ValueError, match="same shape"):
    clusterer._compute_eigenvectors_ncluster(so.affinity(x), make_pairs(51, 8))
  with pytest.raises(ValueError, match="same shape"):
    con.ConstraintPropagation(0.4).adjust_affinity(so.affinity(x), make_pairs(49, 8))
  with pytest.raises(RuntimeError):
    sca.SpectralClusterer(max_spectral_size=20).predict(x, make_pairs(50, 8))


# --- predict(): both operators, before and after refinement ----------------------------------------
@pytest.mark.parametrize("before", [True, False], ids=["before", "after"])
@pytest.mark.parametrize("name", [sca.ConstraintName.ConstraintPropagation,
                                  sca.ConstraintName.AffinityIntegration], ids=["cp", "integ"])
@pytest.mark.parametrize("k", [24, 301], ids=["K<=n", "K>n"])
def test_predict_pairs_equals_predict_dense(name, before, k):
  n = 300
  x, _, _ = so.turn_blobs(n, 24, 3, seed=n, noise=1.0)
  pc = make_pairs(n, k)

  def clusterer():
    return sca.SpectralClusterer(
        min_clusters=2, max_clusters=7, refinement_options=toy_refinement(),
        constraint_options=sca.ConstraintOptions(
            constraint_name=name, apply_before_refinement=before,
            integration_type=sca.IntegrationType.Max, constraint_propagation_alpha=0.4),
        laplacian_type=sca.LaplacianType.GraphCut, row_wise_renorm=True)

  paired, dense = clusterer(), clusterer()
  got = paired.predict(x, pc)
  want = dense.predict(x, pc.to_dense())
  np.testing.assert_array_equal(got, want)
  # the bound test_compute_eigenvectors_ncluster_band_equals_dense uses for this comparison
  np.testing.assert_allclose(paired.consumed_eigenvalues(), dense.consumed_eigenvalues(),
                             rtol=1e-9)
  assert paired.last_diag.symmetry_state == dense.last_diag.symmetry_state


def test_compute_eigenvectors_ncluster_pairs_equals_dense():
  x, _, _ = so.turn_blobs(200, 16, 3, 17)
  opts = toy_refinement()
  opts.p_percentile = 0.9
  clusterer = sca.SpectralClusterer(
      max_clusters=6, refinement_options=opts,
      constraint_options=sca.ConstraintOptions(
          constraint_name=sca.ConstraintName.ConstraintPropagation,
          apply_before_refinement=True, constraint_propagation_alpha=0.4),
      laplacian_type=sca.LaplacianType.GraphCut, row_wise_renorm=True)
  a = so.affinity(x)
  pc = make_pairs(200, 30)
  _, k_pairs, delta_pairs = clusterer._compute_eigenvectors_ncluster(a, pc)
  assert clusterer.last_diag.symmetry_state == 1  # symmetric pairs keep the matrix symmetric
  _, k_dense, delta_dense = clusterer._compute_eigenvectors_ncluster(a, pc.to_dense())
  assert k_pairs == k_dense
  np.testing.assert_allclose(delta_pairs, delta_dense, rtol=1e-9)


def test_turntodiarize_autotune_with_pairs_equals_dense():
  """The AutoTune search inside predict() works on the resident constraint, whatever its form."""
  n = 400
  x, _, _ = so.turn_blobs(n, 24, 4, seed=n + 1, noise=1.0)
  pc = make_pairs(n, 40)
  paired = copy.deepcopy(sca.configs.turntodiarize_clusterer)
  dense = copy.deepcopy(sca.configs.turntodiarize_clusterer)
  np.testing.assert_array_equal(paired.predict(x, pc), dense.predict(x, pc.to_dense()))
  assert paired.last_best_p == dense.last_best_p


BATCH_SIZES = (20, 600, 75, 310, 128, 129, 450, 33, 260, 97, 520, 64, 200, 380, 110, 150, 570, 48,
               340, 127, 230, 490, 88, 410)


@pytest.mark.parametrize("name,before", [(sca.ConstraintName.ConstraintPropagation, True),
                                         (sca.ConstraintName.ConstraintPropagation, False),
                                         (sca.ConstraintName.AffinityIntegration, False)],
                         ids=["cp-before", "cp-after", "integ-after"])
def test_predict_batch_with_pairs_equals_per_call_predict(name, before):
  """24 utterances, n from 20 to 600: both batch routes (short waves up to n = 128, groups above),
  with None, ConstraintMatrix and PairwiseConstraints mixed in every group, and one entry list
  longer than its utterance, which takes the dense stage and must run as a single call."""
  inputs = [so.turn_blobs(n, 24, 3, seed=70 + n, noise=1.0) for n in BATCH_SIZES]
  us = [x for x, _, _ in inputs]
  cs = []
  for i, (n, (_, _, scores)) in enumerate(zip(BATCH_SIZES, inputs)):
    if i % 3 == 0:
      cs.append(make_pairs(n, min(n, (8, 17, 16, 30)[(i // 3) % 4])))
    elif i % 3 == 1:
      cs.append(sca.ConstraintMatrix(list(scores), 1))
    else:
      cs.append(None)
  long_list = BATCH_SIZES.index(200)
  cs[long_list] = make_pairs(200, 201)
  cs[BATCH_SIZES.index(33)] = make_pairs(33, 0)  # a list without entries: Q = 0
  assert sum(isinstance(c, sca.PairwiseConstraints) for c in cs) >= 8

  def clusterer():
    return sca.SpectralClusterer(
        min_clusters=2, max_clusters=7, refinement_options=toy_refinement(),
        constraint_options=sca.ConstraintOptions(
            constraint_name=name, apply_before_refinement=before,
            integration_type=sca.IntegrationType.Max, constraint_propagation_alpha=0.4),
        laplacian_type=sca.LaplacianType.GraphCut, row_wise_renorm=True)

  single = clusterer()
  want = [single.predict(u, c) for u, c in zip(us, cs)]
  batch = clusterer()
  got = batch.predict_batch(us, constraint_matrices=cs)
  routes = batch.last_batch_routes
  print("routes:", routes)
  assert routes[long_list] == 0
  assert set(routes) == {0, 1, 2} and routes.count(0) == 1
  for i, (g, w) in enumerate(zip(got, want)):
    np.testing.assert_array_equal(g, w, err_msg="utterance %d (n=%d)" % (i, BATCH_SIZES[i]))
  assert info(batch._handle())[0] == 0  # nothing stays resident
  again = batch.predict_batch(us, constraint_matrices=cs)
  assert batch.last_batch_routes == routes
  for g, w in zip(again, got):
    np.testing.assert_array_equal(g, w)
  # a list of another n: predict()'s ValueError, before anything is launched
  wrong = list(cs)
  wrong[-1] = make_pairs(BATCH_SIZES[-1] + 1, 8)
  with pytest.raises(ValueError, match="same shape"):
    batch.predict_batch(us, constraint_matrices=wrong)
  # without entry lists the batch is the band-only call it was
  band_only = [c if not isinstance(c, sca.PairwiseConstraints) else None for c in cs]
  got = batch.predict_batch(us, constraint_matrices=band_only)
  for g, u, c in zip(got[:6], us[:6], band_only[:6]):
    np.testing.assert_array_equal(g, single.predict(u, c))


def test_batch_entry_point_validates_every_list_before_launch():
  x = np.ascontiguousarray(so.blobs(40, 8, 2, seed=1))
  clusterer = sca.SpectralClusterer(
      min_clusters=2, max_clusters=7, refinement_options=toy_refinement(),
      constraint_options=copy.deepcopy(sca.configs.turntodiarize_constraint_options))
  handle = clusterer._handle()
  arrays = (_lib.ScArray * 2)()
  for arr in arrays:
    arr.data = x.ctypes.data
    arr.dtype, arr.location = _lib.SC_DTYPE_F64, _lib.SC_MEM_HOST
    arr.rows, arr.cols, arr.row_stride, arr.col_stride = 40, 8, 8, 1
  labels = [np.full(40, -1, dtype=np.int64) for _ in range(2)]
  lp = (ctypes.POINTER(ctypes.c_int64) * 2)(*[_lib.as_int64_p(l) for l in labels])
  rows, cols = np.array([0, 40], dtype=np.int32), np.array([39, 0], dtype=np.int32)
  vals = np.array([1.0, 1.0])
  cons = (_lib.ScConstraintDesc * 2)()
  cons[1].kind, cons[1].count = 3, 2
  cons[1].rows, cons[1].cols = _lib.as_int32_p(rows), _lib.as_int32_p(cols)
  cons[1].vals = _lib.as_double_p(vals)
  lib = handle.lib
  cfg = clusterer.build_config()
  assert lib.sc_predict_batch_constraints(handle.raw, arrays, cons, 2, cfg, lp, None,
                                          16) == _lib.SC_ERR_INVALID  # row 40 of 40
  assert all((l == -1).all() for l in labels)
  cons[1].kind = 1  # a dense matrix does not travel in a batch
  assert lib.sc_predict_batch_constraints(handle.raw, arrays, cons, 2, cfg, lp, None,
                                          16) == _lib.SC_ERR_INVALID
  assert lib.sc_predict_batch_constraints(handle.raw, arrays, cons, 2, cfg, lp, None,
                                          1) == _lib.SC_ERR_INVALID  # the grouped form only
  rows[1] = 39
  cons[1].kind = 3
  handle.check(lib.sc_predict_batch_constraints(handle.raw, arrays, cons, 2, cfg, lp, None, 16))
  assert all((l >= 0).all() for l in labels)
