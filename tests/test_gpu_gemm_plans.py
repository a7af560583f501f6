"""GPU: the fp64 MFMA GEMM (csrc/gemm_f64.hip) on every launch plan of `launch_variant`.

The planner picks one of several launch plans from the tile count against the co-resident
workgroup slots (g_slots = CUs x 2), K, symmetry and the tile map:

  P1  whole tiles only (k_gemm_nt)
  P2  every tile split over K (partials + k_gemm_reduce), no whole-tile wave
  P3  full waves of whole tiles + a split-K tail (k_gemm_reduce, k_gemm_tail_stats)
  P4  P3 with persistent workgroups drawing items from a work queue (K >= 1024, tile map)
  P5  split-K tail whose trailing K chunks are empty (they write zero partials)
  P6  non-symmetric full waves + split-K tail (constraint propagation)
  P7  row statistics reduced without LDS staging (more than 120 tile columns)

`plans()` below is a copy of that planning; every case asserts the plan its id names, so a
retune of the planner fails here instead of silently moving coverage.

Inputs are chosen so that fp64 GEMM arithmetic is exact in any summation order (entries
+-1 / 2^j with 4^j nonzeros per row for the affinity, small multiples of 1/16 or small
integers for Diffuse): the references are exact and the assertions are `np.array_equal`.
A missing, stale, doubled, shifted or wrongly mirrored tile is a nonzero difference.  Above
n = 8000 the Diffuse inputs are m = U V^T with integer U, V of width 8, so the reference
S = U (V^T V) U^T costs seconds on the host while the device still runs the whole K = n loop.

The concurrency tests run the persistent plan (P4) on two handles of one device at once:
its work-queue counters belong to the caller's split-K workspace, not to the process.
"""

import ctypes
import functools
import threading

import numpy as np
import pytest

import spectral_oracle as so

import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import constraint as con
from spectralcluster_amd import refinement as rf

pytestmark = pytest.mark.gpu

BM, BK = 128, 16
STAT_MAX_TILES = 120  # kStatMaxTiles: the LDS-staged row statistics up to 120 tile columns
CP_TOL = 1e-11
EXPLICIT = 1          # sc_stage_diffuse_rowstats: the explicit fp64 product
LOWRANK_FROM = 8000   # Diffuse inputs m = U V^T from here on


@functools.lru_cache(maxsize=None)
def g_slots():
  lib = _lib.load()
  name = ctypes.create_string_buffer(128)
  arch = ctypes.create_string_buffer(128)
  cus = ctypes.c_int(0)
  mem = ctypes.c_int64(0)
  assert lib.sc_device_info(0, name, 128, arch, 128, ctypes.byref(cus), ctypes.byref(mem)) == 0
  assert cus.value > 0
  return 2 * cus.value


def plans(n, k, sym):
  """The launch plans of an (n x K) (n x K)^T product (launch_variant): symmetric products
  always carry the tile map, non-symmetric ones never do."""
  g = g_slots()
  tm = (n + BM - 1) // BM
  tiles = tm * (tm + 1) // 2 if sym else tm * tm
  ktiles = (k + BK - 1) // BK
  full = tiles // g * g
  rem = tiles - full
  ksplit = 1
  if rem > 0:
    ksplit = min(g // rem, max(1, ktiles // 8))
    if k <= 512 and full == 0:
      ksplit = 1
    if ksplit < 2:
      full, rem, ksplit = tiles, 0, 1
  xcd_chunk = full // 8 if (sym and full % 8 == 0 and full >= 512) else 0
  persist = k >= 1024 and xcd_chunk > 0 and rem > 0 and sym
  kper = (ktiles + ksplit - 1) // ksplit
  out = set()
  if rem == 0:
    out.add("P1")
  elif full == 0:
    out.add("P2")
  else:
    out.add("P4" if persist else "P3")
  if rem > 0 and (ksplit - 1) * kper >= ktiles:
    out.add("P5")
  if not sym and rem > 0 and full > 0:
    out.add("P6")
  if tm > STAT_MAX_TILES:
    out.add("P7")
  return out


def expect_plans(ids, n, k, sym):
  want = set(ids.split("+"))
  got = plans(n, k, sym)
  assert want <= got, ("planner moved", n, k, sym, sorted(got))


# --- exact inputs -------------------------------------------------------------------------
def ternary_embeddings(n, d, seed):
  """Entries in {-1, 0, +1}, exactly 4^j nonzeros per row (the largest 4^j <= d), the zeros in
  different columns per row: unit rows are +-2^-j exactly, every cosine a multiple of 4^-j."""
  rng = np.random.default_rng(seed)
  nnz = 4 ** int(np.floor(np.log(d) / np.log(4) + 1e-9))
  x = rng.choice([-1.0, 1.0], size=(n, d))
  if nnz < d:
    order = np.argsort(rng.random((n, d)), axis=1)
    np.put_along_axis(x, order[:, :d - nnz], 0.0, axis=1)
  assert np.all(np.count_nonzero(x, axis=1) == nnz)
  return x


@functools.lru_cache(maxsize=None)
def _factors(n, seed):
  """U (n x 8) integer in [-2, 2] on odd rows, [0, 2] on even rows, the last row all 2;
  V (n x 8) in [0, 2]; W = V^T V (exact)."""
  rng = np.random.default_rng(seed)
  u = rng.integers(-2, 3, size=(n, 8)).astype(np.float64)
  u[0::2] = np.abs(u[0::2])
  u[-1] = 2.0
  v = rng.integers(0, 3, size=(n, 8)).astype(np.float64)
  return u, v, v.T @ v


def diffuse_input(n, seed):
  """Even rows non-negative, odd rows signed, the last row the elementwise largest: every even
  row's maximum of m m^T lies in the last column (the ragged last tile when n % 128 != 0).
  n < LOWRANK_FROM: entries k / 16 with |k| <= 8 (every partial sum a multiple of 2^-8 far
  below 2^53); above: m = U V^T with small integer factors (see _factors)."""
  if n >= LOWRANK_FROM:
    u, v, _ = _factors(n, seed)
    return u @ v.T
  rng = np.random.default_rng(seed)
  m = rng.integers(-8, 9, size=(n, n)).astype(np.float64)
  m[0::2] = np.abs(m[0::2])
  m[-1] = 8.0
  return m / 16.0


def exact_gram_blocks(m, seed, rows=2048):
  """(r0, r1, S[r0:r1]) of S = m m^T, exactly."""
  n = m.shape[0]
  if n >= LOWRANK_FROM:
    u, _, w = _factors(n, seed)
    uw = u @ w
    for r0 in range(0, n, rows):
      r1 = min(n, r0 + rows)
      yield r0, r1, uw[r0:r1] @ u.T
  else:
    s = m @ m.T
    yield 0, n, s


def exact_rowstats(m, seed):
  n = m.shape[0]
  rmax, rsum = np.empty(n), np.empty(n)
  for r0, r1, blk in exact_gram_blocks(m, seed):
    rmax[r0:r1] = blk.max(axis=1)
    rsum[r0:r1] = blk.sum(axis=1)
  # the construction: even rows peak in the last column
  last = m @ m[-1]
  assert np.array_equal(rmax[0::2], last[0::2])
  return rmax, rsum


# --- device calls on a given handle -------------------------------------------------------
def diffuse_on(h, m):
  cfg = _lib.ScConfig()
  h.lib.sc_config_default(cfg)
  out = np.empty_like(m)
  h.check(h.lib.sc_stage_refine(h.raw, rf.RefinementName.Diffuse.value, cfg,
                                _lib.as_double_p(m), m.shape[0], _lib.as_double_p(out)))
  return out


def rowstats_on(h, m):
  n = m.shape[0]
  rmax, rsum = np.empty(n), np.empty(n)
  info = (ctypes.c_int32 * 6)()
  h.check(h.lib.sc_stage_diffuse_rowstats(h.raw, _lib.as_double_p(m), n, EXPLICIT,
                                          _lib.as_double_p(rmax), _lib.as_double_p(rsum), info))
  return rmax, rsum


def propagate_on(h, a, q, alpha):
  cfg = _lib.ScConfig()
  h.lib.sc_config_default(cfg)
  cfg.constraint_name = con.ConstraintName.ConstraintPropagation.value
  cfg.constraint_before_refinement = 1
  cfg.integration_type = 0
  cfg.constraint_alpha = float(alpha)
  out = np.empty_like(a)
  h.check(h.lib.sc_stage_constraint(h.raw, cfg, _lib.as_double_p(a), _lib.as_double_p(q),
                                    a.shape[0], _lib.as_double_p(out)))
  return out


# --- affinity: K = d, epilogue (c + 1) / 2 ---------------------------------------------------
AFFINITY = [
    ("P2", 2048, 1025),
    ("P1", 2817, 17),
    ("P3", 4096, 256),
    ("P3", 4097, 257),
    ("P4", 4097, 1025),
    ("P1", 6000, 16),
    ("P4", 6000, 1025),
    ("P1", 8193, 17),
    ("P3", 8193, 257),
    ("P1+P7", 15400, 1),
    ("P3+P7", 15400, 256),
]


@pytest.mark.parametrize("plan,n,d", AFFINITY,
                         ids=["%s-n%d-d%d" % c for c in AFFINITY])
def test_affinity_exact_on_every_plan(plan, n, d):
  expect_plans(plan, n, d, True)
  x = ternary_embeddings(n, d, seed=n + d)
  got = sca.utils.compute_affinity_matrix(x)
  want = so.affinity(x)
  assert got.shape == (n, n)
  bad = np.argwhere(got != want)
  assert bad.size == 0, (len(bad), bad[:4].tolist())
  assert np.array_equal(got, got.T)


# --- explicit Diffuse: S = m m^T, K = n -------------------------------------------------------
DIFFUSE = [
    ("P2", 2048),
    ("P4+P5", 3969),
    ("P4+P5", 4000),
    ("P4", 4096),
    ("P4", 4097),
    ("P4", 6000),
    ("P4", 8193),
    ("P1", 12000),
    ("P4+P7", 15400),
]


@pytest.mark.parametrize("plan,n", DIFFUSE, ids=["%s-n%d" % c for c in DIFFUSE])
def test_diffuse_exact_on_every_plan(plan, n):
  expect_plans(plan, n, n, True)
  m = diffuse_input(n, seed=n)
  got = rf.Diffuse().refine(m)
  for r0, r1, want in exact_gram_blocks(m, seed=n):
    bad = np.argwhere(got[r0:r1] != want)
    assert bad.size == 0, (r0, len(bad), (bad[:4] + [r0, 0]).tolist())
  assert np.array_equal(got, got.T)


# --- row statistics of S from the GEMM epilogue (stats mode 1) -------------------------------
ROWSTATS = [("P4", 4097), ("P4", 8193), ("P4+P7", 15400)]


@pytest.mark.parametrize("plan,n", ROWSTATS, ids=["%s-n%d" % c for c in ROWSTATS])
def test_diffuse_rowstats_exact_on_every_plan(plan, n):
  """Whole tiles (epilogue statistics), split-tail tiles (k_gemm_tail_stats, both halves of a
  mirrored tile), the ragged last tile column, and the per-row reduction (LDS-staged, or
  k_gemm_stats_reduce above 120 tile columns)."""
  expect_plans(plan, n, n, True)
  assert n % BM != 0  # the even rows' maxima sit in a ragged tile
  m = diffuse_input(n, seed=n + 1)
  want_max, want_sum = exact_rowstats(m, seed=n + 1)
  rmax, rsum = rowstats_on(_lib.default_handle(), m)
  assert np.array_equal(rmax, want_max), np.flatnonzero(rmax != want_max)[:8]
  assert np.array_equal(rsum, want_sum), np.flatnonzero(rsum != want_sum)[:8]


# --- constraint propagation: symmetric and non-symmetric products, kEpiAdd --------------------
def cp_inputs(n, kind, seed):
  x, _, scores = so.turn_blobs(n, 16, 3, seed=seed)
  a = so.affinity(x)
  q = so.constraint_matrix_diagonals(list(scores), 1)
  rng = np.random.default_rng(seed)
  if kind in ("symA_genQ", "genA_genQ"):
    q = q + 0.5 * (rng.random((n, n)) < 2.0 / n)  # a few one-sided entries
  if kind == "genA_genQ":
    a = a * (1.0 + 0.01 * rng.random((n, n)))
  return a, q


CP = [
    ("P1", "P5+P6", 2817, "symA_symQ"),
    ("P1", "P5+P6", 2817, "genA_genQ"),
    ("P4", "P6", 4097, "symA_symQ"),
    ("P4", "P6", 4097, "symA_genQ"),
    ("P4", "P6", 4097, "genA_genQ"),
    ("P4", "P6", 6000, "symA_genQ"),
    ("P4", "P6", 6000, "genA_genQ"),
]


@pytest.mark.parametrize("sym_plan,gen_plan,n,kind", CP,
                         ids=["sym%s-gen%s-n%d-%s" % c for c in CP])
def test_constraint_propagation_on_every_plan(sym_plan, gen_plan, n, kind):
  expect_plans(sym_plan, n, n, True)
  expect_plans(gen_plan, n, n, False)
  a, q = cp_inputs(n, kind, seed=n)
  assert np.array_equal(a, a.T) == kind.startswith("symA")
  assert np.array_equal(q, q.T) == kind.endswith("symQ")
  alpha = 0.6
  got = con.ConstraintPropagation(alpha).adjust_affinity(a, q)
  want = so.constraint_propagation(a, q, alpha)
  err = float(np.max(np.abs(got - want)) / max(1.0, np.max(np.abs(want))))
  assert err < CP_TOL, err


# --- CropDiagonal's fill value from the affinity epilogue (stats mode 2), end to end ----------
@pytest.mark.parametrize("n,mode", [(6000, 1), (8193, 1), (15400, 0)])
def test_icassp_with_split_affinity_tail(n, mode):
  """d = 256: the affinity runs full waves + a split-K tail, so CropDiagonal's value of the
  tail rows comes from k_gemm_tail_stats (mode 2); diffuse_mode 1: the explicit Diffuse runs
  the persistent plan with row statistics (mode 1).  n = 15400 (default route): CropDiagonal's
  value reduced by k_gemm_stats_reduce."""
  d, maxc = 256, 7
  expect_plans("P3+P7" if n > STAT_MAX_TILES * BM else "P3", n, d, True)
  if mode == 1:
    expect_plans("P4", n, n, True)
  x = so.blobs(n, d, 5, seed=n)
  want, w_ref = so.predict_algorithm_matched(x, so.icassp2018_config(max_clusters=maxc))
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=maxc,
                            refinement_options=sca.configs.icassp2018_refinement_options)
  c.diffuse_mode = mode
  got = c.predict(x)
  if mode == 1:
    assert c.last_diag.diffuse_path == _lib.DIFFUSE_PATH_EXPLICIT
  idx = so.consumed_eigen_indices(n, maxc, True, w_ref, 1e-2)
  w = c.last_diag.eigenvalue_array()
  assert np.max(np.abs(w[idx] - w_ref[idx]) / np.maximum(np.abs(w_ref[idx]), 1e-9)) < 1e-6
  assert so.adjusted_rand_index(got, want) == 1.0


# --- two handles of one device at once --------------------------------------------------------
def run_pair(fn, args):
  """fn(handle, *args[i]) on two fresh handles, one thread each, started together; three
  rounds.  Returns results[round][thread]."""
  handles = [_lib.Handle(0), _lib.Handle(0)]
  try:
    results = []
    for _ in range(3):
      barrier = threading.Barrier(2)
      out = [None, None]
      err = [None, None]

      def work(i):
        try:
          barrier.wait()
          out[i] = fn(handles[i], *args[i])
        except BaseException as e:  # re-raised in the main thread
          err[i] = e

      threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
      for t in threads:
        t.start()
      for t in threads:
        t.join()
      for e in err:
        if e is not None:
          raise e
      results.append(out)
    return results
  finally:
    for h in handles:
      h.close()


def test_concurrent_persistent_diffuse_on_two_handles():
  n = 8192
  expect_plans("P4", n, n, True)
  seeds = (11, 12)
  ms = [diffuse_input(n, seed=s) for s in seeds]
  results = run_pair(diffuse_on, [(m,) for m in ms])
  for i, s in enumerate(seeds):
    for r0, r1, want in exact_gram_blocks(ms[i], seed=s):
      for rnd in range(3):
        bad = np.count_nonzero(results[rnd][i][r0:r1] != want)
        assert bad == 0, ("round", rnd, "thread", i, "rows", r0, bad)


def test_concurrent_constraint_propagation_on_two_handles():
  n = 4097
  expect_plans("P4", n, n, True)
  inputs = [cp_inputs(n, "symA_symQ", seed=21), cp_inputs(n, "symA_genQ", seed=22)]
  single = [propagate_on(_lib.default_handle(), a, q, 0.6) for a, q in inputs]
  results = run_pair(propagate_on, [(a, q, 0.6) for a, q in inputs])
  for rnd in range(3):
    for i in range(2):
      assert np.array_equal(results[rnd][i], single[i]), ("round", rnd, "thread", i)


def test_predict_batch_on_two_streams_with_explicit_diffuse():
  sizes = (4097, 4500, 6000, 8192)
  for n in sizes:
    assert plans(n, n, True) & {"P4"}
  utts = [so.blobs(n, 64, 4, seed=n) for n in sizes]

  def labels(streams):
    c = sca.SpectralClusterer(min_clusters=2, max_clusters=7,
                              refinement_options=sca.configs.icassp2018_refinement_options)
    c.diffuse_mode = 1
    return c.predict_batch(utts, streams=streams)

  one = labels(1)
  two = labels(2)
  for n, a, b in zip(sizes, one, two):
    assert np.array_equal(a, b), n
