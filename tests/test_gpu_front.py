"""GPU: the fused refinement front, directly, on every route that runs it (`sc_stage_front`).

`predict()` does not run the per-op kernels tests/test_gpu_stages.py holds to the oracle bit for
bit; it runs a fused front -- CropDiagonal's value out of the affinity GEMM's epilogue, the blur
with the diagonal override and per-strip row maxima, the cut vector from those partials, threshold
+ symmetrise in one pass over tile pairs (which also writes the 8-bit digits of the matrix-free
Diffuse), the row statistics and the scaling vectors -- from three drivers: the single call
(api.hip), the grouped batch (enqueue_front_grouped) and the round body of the AutoTune sweep.
`sc_stage_front` runs each driver's own front, stops before the eigensolver and copies out what it
left; these tests compare that with the CPU chain of tests/_front_ref.py applied to the affinity
the DEVICE returned, so that nothing depends on GEMM rounding:

  * cropval, cut and a: `np.array_equal` (a max, a compare, a multiply by a constant, an average
    of two values; the blur keeps scipy's summation order, as the per-op tests already demand);
  * a exactly symmetric, every output finite;
  * s (where the route formed it) against a_ref a_ref^T at rtol 2e-14 (test_diffuse_vs_oracle's
    tolerance), and equal to its own transpose;
  * rowmax / rowsum within check_rowstats' tolerances (tests/test_gpu_diffuse_free.py): 1e-13 and
    1e-12 of the row's scale;
  * c, p, t within 4 ulp of the formulas above scaling_vectors_body (rowops.hip) evaluated in
    NumPy on the rowmax / rowsum the device returned: at most five fp64 operations each, and the
    library is built with -ffp-contract=off and no fast-math flag, so division and sqrt are
    correctly rounded and nothing is fused;
  * info names the kernels and branches the case was built to reach: a case that went down
    another path fails.
"""

import ctypes
import dataclasses
import os

import numpy as np
import pytest

import spectral_oracle as so

import _front_ref as fr
from spectralcluster_amd import _lib
from spectralcluster_amd import refinement as rf

pytestmark = pytest.mark.gpu

SINGLE, GROUPED, SWEEP = (_lib.SC_FRONT_ROUTE_SINGLE, _lib.SC_FRONT_ROUTE_GROUPED,
                          _lib.SC_FRONT_ROUTE_SWEEP)
NONE, EXPLICIT, FREE = 0, 1, 2                    # SC_DIFFUSE_PATH_*
GENERIC, TILE, STREAM, NO_BLUR = 0, 1, 2, -1      # SC_FRONT_INFO_BLUR_KERNEL
CROP_NONE, CROP_EPILOGUE, CROP_KERNEL = 0, 1, 2   # SC_FRONT_INFO_CROP_SOURCE
CUT_PARTIALS, CUT_ROWS, CUT_PERCENTILE = 1, 2, 3  # SC_FRONT_INFO_CUT_KERNEL
MATRICES = ("a0", "a", "s")

ICASSP = so.icassp2018_config()
TTD = so.turntodiarize_config(constraint_name=so.CONSTRAINT_NONE)


# ------------------------------------------------------------------------- the entry
def sc_config(ocfg, diffuse_mode=0):
  lib = _lib.load()
  cfg = _lib.ScConfig()
  lib.sc_config_default(cfg)
  cfg.n_ops = len(ocfg.sequence)
  for i, op in enumerate(ocfg.sequence):
    cfg.ops[i] = op
  # (the binding's own way: the blur weights are scipy's NumPy expression, bit for bit;
  #  sc_gaussian_weights goes through libm's exp and is 1 ulp off NumPy's at sigma 2, 4 and 8)
  rf.fill_config(cfg, sigma=ocfg.gaussian_blur_sigma, p_percentile=ocfg.p_percentile,
                 multiplier=ocfg.soft_multiplier,
                 threshold_type=rf.ThresholdType(ocfg.threshold_type),
                 binarize=ocfg.binarize, preserve_diagonal=ocfg.preserve_diagonal,
                 symmetrize_type=rf.SymmetrizeType(ocfg.symmetrize_type))
  cfg.laplacian_type = ocfg.laplacian_type
  cfg.min_clusters = ocfg.min_clusters or 0
  cfg.max_clusters = ocfg.max_clusters or 0
  cfg.diffuse_mode = diffuse_mode
  return cfg


def run_front(route, ocfg, xs=None, affinity=None, ps=None, diffuse_mode=0):
  """-> one dict per member: the arrays sc_stage_front wrote (absent: not written) + "info"."""
  h = _lib.default_handle()
  cfg = sc_config(ocfg, diffuse_mode)
  if xs is not None:
    xs = [np.ascontiguousarray(x, dtype=np.float64) for x in xs]
    d = xs[0].shape[1]
    sizes = [x.shape[0] for x in xs]
    xs_p = (_lib._c_double_p * len(xs))(*[_lib.as_double_p(x) for x in xs])
  else:
    affinity = np.ascontiguousarray(affinity, dtype=np.float64)
    d, sizes, xs_p = 0, [affinity.shape[0]], None
  count = len(ps) if route == SWEEP else len(sizes)
  member_n = [sizes[0]] * count if route == SWEEP else sizes
  ns = (ctypes.c_int32 * len(sizes))(*sizes)
  ps_arr = np.ascontiguousarray(ps, dtype=np.float64) if ps is not None else None
  outs = (_lib.ScFrontOut * count)()
  arrays = []
  for z in range(count):
    n = member_n[z]
    member = {name: np.full((n, n) if name in MATRICES else (n,), np.nan)
              for name in _lib.FRONT_OUTPUTS}
    for name, arr in member.items():
      setattr(outs[z], name, _lib.as_double_p(arr))
    arrays.append(member)
  h.check(h.lib.sc_stage_front(
      h.raw, route, ctypes.byref(cfg), count, ns, d, xs_p,
      _lib.as_double_p(affinity) if affinity is not None else None,
      _lib.as_double_p(ps_arr) if ps_arr is not None else None, outs))
  members = []
  for z in range(count):
    info = dict(zip(_lib.FRONT_INFO_NAMES, outs[z].info))
    got = {name: arr for i, (name, arr) in enumerate(arrays[z].items())
           if info["written"] >> i & 1}
    got["info"] = info
    members.append(got)
  return members


# ------------------------------------------------------------------- the launcher's rule
def stream_rows_per_wave(wave_rows_total, radius):
  """blur.hip stream_rows_per_wave: whole rounds of resident workgroups, 16 .. 128 rows."""
  slots = 256 * (3 if radius == 4 else 2) * 4
  rounds = 1
  while True:
    rows = -(-wave_rows_total // (slots * rounds))
    if rows <= 128:
      return max(rows, 16)
    rounds += 1


def strips(n, radius):
  return -(-n // (256 - 2 * radius))


def single_blur(n, radius):
  """(kernel, rows per wave) of launch_gaussian_blur_fused."""
  if radius not in (4, 8) or n < 128:
    return GENERIC, 0
  if n < 512:
    return TILE, 0
  rows = stream_rows_per_wave(strips(n, radius) * n, radius)
  per_round = 256 * (3 if radius == 4 else 2)
  while rows < 128:
    wgs = strips(n, radius) * -(-n // (4 * rows))
    if wgs <= per_round or wgs % per_round == 0 or wgs % per_round > per_round * 3 // 4:
      break
    rows += 1
  return STREAM, rows


def group_blur(sizes, radius):
  return STREAM, stream_rows_per_wave(sum(strips(n, radius) * n for n in sizes), radius)


def free_expected(n, diffuse_mode, in_group=False):
  """free_diffuse_wanted for the presets' eigen request (max_clusters = 7)."""
  mode = diffuse_mode or {"explicit": 1, "free": 2}.get(os.environ.get("SC_DIFFUSE"), 0)
  if mode == 1 or n <= 128:
    return False
  if mode == 2:
    return True
  return n >= int(os.environ.get("SC_DIFFUSE_FREE_MIN_N", 1536 if in_group else 2048))


# ------------------------------------------------------------------------ the checks
def ulps(got, want):
  """(np.spacing(0) is the smallest subnormal: where `want` is 0 only an exact 0 passes)"""
  return np.abs(got - want) / np.spacing(np.abs(want))


def check_member(got, ocfg, expect, name, ref=None, plateau=False):
  """One member's front against the reference chain on its own a0; `expect`: info entries the
  case was built to reach.  Returns the reference (to share between members with one input).
  `plateau`: the case is built so that the candidate search of the matrix-free route cannot
  prune (rows of S full of near-ties): more rows go over the candidate cap than the exact-row
  route takes, the solver forms S after all and recomputes both statistics -- the row maxima
  the front left are provisional then, and only then, and are not compared here:
  check_solver_corrects_plateau holds what the solver makes of them to the reference."""
  info = got["info"]
  print("front:", name, {k: v for k, v in info.items() if k != "written"})  # (pytest -s)
  for key, value in expect.items():
    assert info[key] == value, (name, key, info)
  a0 = got["a0"]
  if ref is None:
    ref = fr.front(a0, ocfg)
  for key, arr in got.items():
    if key != "info":
      assert np.all(np.isfinite(arr)), (name, key)
  # cropval / cut / a: bit for bit
  assert ("cropval" in got) == (info["crop_source"] != CROP_NONE), (name, info)
  if "cropval" in got:
    assert np.array_equal(got["cropval"], ref.cropval), (
        name, np.abs(got["cropval"] - ref.cropval).max())
  assert np.array_equal(got["cut"], ref.cut), (name, np.abs(got["cut"] - ref.cut).max(),
                                               np.flatnonzero(got["cut"] != ref.cut)[:8])
  a = got["a"]
  assert np.array_equal(a, ref.a), (name, np.abs(a - ref.a).max(),
                                    np.argwhere(a != ref.a)[:8])
  assert np.array_equal(a, a.T), name
  # s, where the route formed it
  assert ("s" in got) == (info["diffuse_path"] == EXPLICIT), (name, info)
  if "s" in got:
    np.testing.assert_allclose(got["s"], ref.s, rtol=2e-14, atol=0, err_msg=name)
    assert np.array_equal(got["s"], got["s"].T), name
  # the row statistics the scaling kernel read (check_rowstats' expressions)
  last = ref.a if ref.s is None else ref.s
  scale = np.abs(last).max()
  if plateau:
    assert info["free_op"] and info["free_forms_s"] == 1, (name, info)
  elif info["free_op"]:
    # (rows over the candidate cap get their exact maximum at the solver's first
    #  synchronisation: the front's statistics are final only without them)
    assert info["free_overflow_rows"] == 0 and info["free_forms_s"] == 0, (name, info)
    assert 0 < info["free_candidates"], (name, info)
  if not plateau:
    tol = 1e-13 * np.maximum(np.abs(ref.rowmax), 1e-3 * scale)
    assert np.all(np.abs(got["rowmax"] - ref.rowmax) <= tol), (
        name, np.abs(got["rowmax"] - ref.rowmax).max())
  tols = 1e-12 * np.maximum(np.abs(ref.rowsum), np.abs(last).sum(axis=1))
  assert np.all(np.abs(got["rowsum"] - ref.rowsum) <= tols), (
      name, np.abs(got["rowsum"] - ref.rowsum).max())
  # c / p / t from the statistics the device itself read
  assert bool(info["folded_rownorm"]) == ref.folded_rownorm and info["symmetric"] == 1, info
  c, p, t = fr.scaling_vectors(got["rowmax"], got["rowsum"], ocfg.laplacian_type,
                               ref.folded_rownorm)
  for key, want in (("c", c), ("p", p), ("t", t)):
    worst = ulps(got[key], want).max()
    assert worst <= 4, (name, key, worst)
  return ref


def check_solver_corrects_plateau(x, ocfg, diffuse_mode, ref, name):
  """The full call on a plateau case: the solver's first synchronisation sees more overflow rows
  than the exact-row route takes, forms S after all (diffuse_path FREE_THEN_EXPLICIT) and rebuilds
  the scaling vectors from its epilogue's statistics.  c and p of the solve (sc_stage_krylov_state)
  against the formulas on the REFERENCE statistics: rowmax and rowsum are held to 1e-13 / 1e-12 of
  the row's scale above, c = sqrt(1 / rowmax) carries half the relative error of rowmax and p the
  sum of both, so 1e-12 relative bounds either."""
  h = _lib.default_handle()
  cfg = sc_config(ocfg, diffuse_mode)
  x = np.ascontiguousarray(x, dtype=np.float64)
  n, d = x.shape
  h.check(h.lib.sc_set_embeddings(h.raw, _lib.as_double_p(x), n, d))
  h.check(h.lib.sc_compute_affinity(h.raw))
  diag = _lib.ScDiag()
  h.check(h.lib.sc_eig_ncluster(h.raw, ctypes.byref(cfg), ctypes.byref(diag)))
  assert diag.diffuse_path == 3, (name, diag.diffuse_path)   # SC_DIFFUSE_PATH_FREE_THEN_EXPLICIT
  assert diag.free_overflow_rows > 64, (name, diag.free_overflow_rows)
  state = (ctypes.c_int32 * 8)()
  c, p = np.empty(n), np.empty(n)
  h.check(h.lib.sc_stage_krylov_state(h.raw, state, None, None, None, _lib.as_double_p(c),
                                      _lib.as_double_p(p)))
  assert state[1] == n and state[2] == 0, (name, list(state))  # S itself, not A applied twice
  want_c, want_p, _ = fr.scaling_vectors(ref.rowmax, ref.rowsum, ocfg.laplacian_type,
                                         ref.folded_rownorm)
  np.testing.assert_allclose(c, want_c, rtol=1e-12, atol=0, err_msg=name)
  np.testing.assert_allclose(p, want_p, rtol=1e-12, atol=0, err_msg=name)


def icassp_expect(n, radius, diffuse_mode=0, preserve_diagonal=False, embeddings=True,
                  blur=None, in_group=False, percentile=False):
  """info of the ICASSP2018 front for one member."""
  kernel, rows = blur if blur is not None else single_blur(n, radius)
  free = free_expected(n, diffuse_mode, in_group)
  fused_crop = kernel != GENERIC
  return {
      "blur_kernel": kernel, "blur_rows": rows,
      "crop_source": (CROP_EPILOGUE if embeddings else CROP_KERNEL) if fused_crop else CROP_NONE,
      "cut_kernel": CUT_PERCENTILE if percentile else (
          CUT_PARTIALS if fused_crop and not preserve_diagonal else CUT_ROWS),
      "diffuse_path": FREE if free else EXPLICIT, "free_op": int(free),
      # the threshold pass writes the digits when max|a| is known from the cut vector: a cosine
      # affinity computed from embeddings, RowMax, p > 0
      "digits_fused": int(free and embeddings and not percentile),
      "folded_rownorm": 1,
  }


def embeddings(n, seed=None, d=None):
  d = 16 + (n % 17) if d is None else d  # 16 .. 32
  return so.blobs(n, d, 3 + n % 3, seed=n if seed is None else seed)


# ---------------------------------------------------------------- single route, ICASSP2018
SINGLE_SIZES = {
    1: [100, 128, 200, 257, 511, 512, 777, 1300, 3600],
    2: [100, 128, 200, 257, 511, 512, 777, 1300, 3300],
}


@pytest.mark.parametrize("sigma,n", [(s, n) for s in (1, 2) for n in SINGLE_SIZES[s]])
def test_single_icassp(sigma, n):
  """n = 100: generic blur, unfused crop, k_cut_from_rows; 128 .. 511: the tile kernel (56- /
  48-column tiles, ragged last tile column, ragged last 64-row band); 512 .. 1300: the streaming
  kernel at 16 rows per wave, ragged last strip; 3600 (sigma 1) / 3300 (sigma 2): the smallest
  single calls whose wave wraps its 12- / 20-slot register ring with a remainder (18 / 23 rows
  per wave) -- and, above n = 2048, the matrix-free route with the digits out of the threshold
  pass."""
  radius = 4 * sigma
  ocfg = dataclasses.replace(ICASSP, gaussian_blur_sigma=sigma)
  expect = icassp_expect(n, radius)
  if n == 100:
    assert (expect["blur_kernel"], expect["cut_kernel"]) == (GENERIC, CUT_ROWS)
  if n in (3600, 3300):
    assert expect["blur_rows"] == (18 if sigma == 1 else 23) and expect["digits_fused"] == 1
  got, = run_front(SINGLE, ocfg, xs=[embeddings(n)])
  check_member(got, ocfg, expect, "single n=%d sigma=%d" % (n, sigma))


# ------------------------------------------------------------ single route, further cases
@pytest.mark.parametrize("lap", [so.LAPLACIAN_NONE, so.LAPLACIAN_GRAPH_CUT])
@pytest.mark.parametrize("mode", [EXPLICIT, FREE])
@pytest.mark.parametrize("n", [200, 520, 1153])
def test_single_diffuse_routes(n, mode, lap):
  """diffuse_mode 1: the explicit product, s returned, statistics from its epilogue;
  diffuse_mode 2: the statistics come from the digits the threshold pass wrote."""
  ocfg = dataclasses.replace(ICASSP, laplacian_type=lap)
  expect = icassp_expect(n, 4, diffuse_mode=mode)
  assert expect["diffuse_path"] == mode and expect["digits_fused"] == int(mode == FREE)
  got, = run_front(SINGLE, ocfg, xs=[embeddings(n)], diffuse_mode=mode)
  check_member(got, ocfg, expect, "single n=%d mode=%d lap=%d" % (n, mode, lap))


@pytest.mark.parametrize("lap", [so.LAPLACIAN_UNNORMALIZED, so.LAPLACIAN_RANDOM_WALK])
def test_single_scaling_vectors_of_the_other_laplacians(lap):
  n = 257
  ocfg = dataclasses.replace(ICASSP, laplacian_type=lap)
  got, = run_front(SINGLE, ocfg, xs=[embeddings(n)])
  check_member(got, ocfg, icassp_expect(n, 4), "single n=%d lap=%d" % (n, lap))


def test_single_free_prune_list_on_and_off():
  """The tile skip list of the digit product changes which tiles run, never a statistic."""
  n = 1153
  h = _lib.default_handle()
  x = embeddings(n)
  expect = icassp_expect(n, 4, diffuse_mode=FREE)
  results = []
  for prune in (0, 1):
    h.check(h.lib.sc_set_free_prune(h.raw, prune))
    try:
      got, = run_front(SINGLE, ICASSP, xs=[x], diffuse_mode=FREE)
    finally:
      h.check(h.lib.sc_set_free_prune(h.raw, -1))
    check_member(got, ICASSP, expect, "prune=%d" % prune)
    results.append(got)
  for key in ("rowmax", "rowsum", "c", "p", "t", "a", "cut"):
    assert np.array_equal(results[0][key], results[1][key]), key


OPTIONS = {
    "average": dict(symmetrize_type=so.SYMMETRIZE_AVERAGE),
    "binarize": dict(binarize=True),
    # (the blur's partials include the diagonal: k_cut_from_rows runs with it zeroed)
    "preserve_diagonal": dict(preserve_diagonal=True),
    "average_binarize_preserve": dict(symmetrize_type=so.SYMMETRIZE_AVERAGE, binarize=True,
                                      preserve_diagonal=True),
    # (Percentile cut of the blurred matrix inside the ICASSP2018 sequence: max|a| is not known
    #  from the cut vector, the matrix-free route quantises in a pass of its own)
    "percentile": dict(threshold_type=so.THRESHOLD_PERCENTILE, p_percentile=0.9),
    "p95": dict(p_percentile=0.95),
    "p30": dict(p_percentile=0.3),
    "p100": dict(p_percentile=1.0),
}


@pytest.mark.parametrize("mode", [EXPLICIT, FREE])
@pytest.mark.parametrize("option", sorted(OPTIONS))
@pytest.mark.parametrize("n", [257, 777])
def test_single_options(n, option, mode):
  ocfg = dataclasses.replace(ICASSP, **OPTIONS[option])
  expect = icassp_expect(n, 4, diffuse_mode=mode, preserve_diagonal=ocfg.preserve_diagonal,
                         percentile=ocfg.threshold_type == so.THRESHOLD_PERCENTILE)
  if ocfg.preserve_diagonal and ocfg.threshold_type == so.THRESHOLD_ROW_MAX:
    assert expect["cut_kernel"] == CUT_ROWS
  got, = run_front(SINGLE, ocfg, xs=[embeddings(n)], diffuse_mode=mode)
  # (a binarised matrix of a few tight clusters: its rows inside a cluster are equal up to the
  #  soft entries, and so are the entries of S along them)
  plateau = ocfg.binarize and mode == FREE
  name = "single n=%d %s mode=%d" % (n, option, mode)
  ref = check_member(got, ocfg, expect, name, plateau=plateau)
  if plateau:
    check_solver_corrects_plateau(embeddings(n), ocfg, mode, ref, name)


def duplicated_affinity(n, seed):
  """A symmetric affinity with 10 % of every row set to one value: duplicates around the
  order statistic, as test_percentile_threshold_bit_exact_vs_oracle builds them."""
  rng = np.random.default_rng(seed)
  m = rng.random((n, n))
  m = 0.5 * (m + m.T)
  mask = rng.random((n, n)) < 0.05
  m[mask | mask.T] = 0.25
  np.fill_diagonal(m, 1.0)
  return m


@pytest.mark.parametrize("p", [0.95, 0.5, 0.4, 0.123])
@pytest.mark.parametrize("n", [257, 777])
def test_single_turntodiarize(n, p):
  """[RowWiseThreshold, Symmetrize]: Percentile cut, binarisation, preserved diagonal, Average;
  GraphCut scaling vectors from the row sums of the symmetrised matrix itself."""
  ocfg = dataclasses.replace(TTD, p_percentile=p)
  expect = {"blur_kernel": NO_BLUR, "crop_source": CROP_NONE, "cut_kernel": CUT_PERCENTILE,
            "diffuse_path": NONE, "free_op": 0, "digits_fused": 0, "folded_rownorm": 0}
  got, = run_front(SINGLE, ocfg, affinity=duplicated_affinity(n, n))
  assert np.array_equal(got["a0"], duplicated_affinity(n, n))
  check_member(got, ocfg, expect, "single ttd n=%d p=%g" % (n, p))


def test_single_supplied_affinity_with_negative_entries():
  """A caller's affinity: no epilogue value, k_crop_value runs and clamps at 0 on rows whose
  off-diagonal entries are all negative; max|a| is not known from the cut vector, so the
  matrix-free route quantises in a pass of its own (digits_fused 0)."""
  n = 300
  rng = np.random.default_rng(300)
  m = rng.standard_normal((n, n))
  m = 0.5 * (m + m.T)
  negative = [0, 17, 150, 299]
  for i in negative:
    m[i, :] = -np.abs(m[i, :]) - 0.01
    m[:, i] = m[i, :]
  np.fill_diagonal(m, 1.0)
  expect = icassp_expect(n, 4, diffuse_mode=FREE, embeddings=False)
  assert expect["crop_source"] == CROP_KERNEL and expect["digits_fused"] == 0
  got, = run_front(SINGLE, ICASSP, affinity=m, diffuse_mode=FREE)
  assert np.array_equal(got["a0"], m)
  assert np.all(got["cropval"][negative] == 0.0) and np.count_nonzero(got["cropval"] == 0.0) == 4
  check_member(got, ICASSP, expect, "single supplied affinity")


# ------------------------------------------------------------------------ grouped route
def check_group(sizes, ocfg, diffuse_mode, expect_rows, name, seeds=None):
  radius = 4 * ocfg.gaussian_blur_sigma
  blur = group_blur(sizes, radius)
  if expect_rows is not None:
    assert blur[1] == expect_rows
  seeds = seeds or list(sizes)
  xs = [embeddings(n, seed=s, d=24) for n, s in zip(sizes, seeds)]  # (one width per batch)
  members = run_front(GROUPED, ocfg, xs=xs, diffuse_mode=diffuse_mode)
  refs = {}
  for z, (n, got) in enumerate(zip(sizes, members)):
    expect = icassp_expect(n, radius, diffuse_mode=diffuse_mode, blur=blur, in_group=True)
    key = (n, seeds[z])
    refs[key] = check_member(got, ocfg, expect, "%s member %d n=%d" % (name, z, n),
                             ref=refs.get(key))
  return members


GROUP_A = [256, 300, 411, 520, 640, 777, 1000, 1300]
GROUP_B = [1200, 900, 1300, 1000, 777, 1500, 640, 520]


@pytest.mark.parametrize("sigma", [1, 2])
def test_grouped_small_members(sigma):
  """Rows per wave 16; the smallest member is one strip high."""
  check_group(GROUP_A, dataclasses.replace(ICASSP, gaussian_blur_sigma=sigma), 0, 16,
              "group A sigma=%d" % sigma)


@pytest.mark.parametrize("sigma,rows", [(1, 26), (2, 39)])
def test_grouped_sixteen_members(sigma, rows):
  """Rows per wave from the whole group's work: 26 (sigma 1) / 39 (sigma 2), above the 12- /
  20-slot ring.  Members z and z + 8 are the same utterance at two positions of the group:
  bit-identical results."""
  sizes = GROUP_B + GROUP_B
  members = check_group(sizes, dataclasses.replace(ICASSP, gaussian_blur_sigma=sigma), 0, rows,
                        "group B sigma=%d" % sigma)
  for z in range(8):
    for key in _lib.FRONT_OUTPUTS:
      assert np.array_equal(members[z][key], members[z + 8][key]), (z, key)


def test_grouped_mixed_diffuse_routes():
  """Default routing: the members from n = 1536 on are matrix-free, the others explicit, and
  all four share one k_threshold_symmetrize_digits_g launch."""
  sizes = [1600, 1536, 1300, 520]
  members = check_group(sizes, ICASSP, 0, None, "group mixed")
  assert [m["info"]["digits_fused"] for m in members] == [1, 1, 0, 0]
  assert [m["info"]["diffuse_path"] for m in members] == [FREE, FREE, EXPLICIT, EXPLICIT]


def test_grouped_all_matrix_free():
  members = check_group(GROUP_A, ICASSP, FREE, 16, "group A free")
  assert all(m["info"]["digits_fused"] == 1 for m in members)


def test_grouped_graph_cut_and_a_member_twice():
  """GraphCut scaling vectors through k_scaling_vectors_g; one utterance at positions 0 and 3."""
  sizes, seeds = [411, 777, 300, 411], [411, 777, 300, 411]
  ocfg = dataclasses.replace(ICASSP, laplacian_type=so.LAPLACIAN_GRAPH_CUT)
  members = check_group(sizes, ocfg, 0, 16, "group graphcut", seeds=seeds)
  for key in _lib.FRONT_OUTPUTS:
    assert np.array_equal(members[0][key], members[3][key]), key


# -------------------------------------------------------------------------- sweep route
SWEEP_P = (0.95, 0.9, 0.7, 0.4, 0.3)


@pytest.mark.parametrize("mode", [EXPLICIT, FREE])
@pytest.mark.parametrize("n", [520, 1153])
def test_sweep_icassp(n, mode):
  """One blur, then per value: the cut from the shared partials with p_own, the grouped
  threshold pass (with the digits in matrix-free mode), Diffuse or its statistics."""
  ocfg = dataclasses.replace(ICASSP, laplacian_type=so.LAPLACIAN_GRAPH_CUT)
  members = run_front(SWEEP, ocfg, xs=[embeddings(n)], ps=SWEEP_P, diffuse_mode=mode)
  assert len(members) == len(SWEEP_P)
  for p, got in zip(SWEEP_P, members):
    at_p = dataclasses.replace(ocfg, p_percentile=p)
    expect = icassp_expect(n, 4, diffuse_mode=mode)
    check_member(got, at_p, expect, "sweep n=%d mode=%d p=%g" % (n, mode, p))
    assert np.array_equal(got["a0"], members[0]["a0"])
    assert np.array_equal(got["cropval"], members[0]["cropval"])


@pytest.mark.parametrize("n", [520, 1153])
def test_sweep_turntodiarize(n):
  """[RowWiseThreshold, Symmetrize] alone: k_row_percentile_cut_g with p_own per member.  A
  tenth of the utterance's frames are copies of other frames: every row of the affinity then
  holds runs of equal values for the order statistic to land in."""
  x = embeddings(n)
  rng = np.random.default_rng(n)
  copies = rng.choice(n, n // 10, replace=False)
  x[copies] = x[rng.choice(np.setdiff1d(np.arange(n), copies), n // 10)]
  expect = {"blur_kernel": NO_BLUR, "crop_source": CROP_NONE, "cut_kernel": CUT_PERCENTILE,
            "diffuse_path": NONE, "free_op": 0, "digits_fused": 0, "folded_rownorm": 0}
  members = run_front(SWEEP, TTD, xs=[x], ps=SWEEP_P)
  for p, got in zip(SWEEP_P, members):
    check_member(got, dataclasses.replace(TTD, p_percentile=p), expect,
                 "sweep ttd n=%d p=%g" % (n, p))


# ------------------------------------------------- what the grouped code does not cover
def test_uncovered_configurations_are_refused():
  """The entry never takes another path quietly."""
  with pytest.raises(_lib.UnsupportedOnDeviceError):     # a member below n = 256
    run_front(GROUPED, ICASSP, xs=[embeddings(300, d=16), embeddings(200, d=16)])
  with pytest.raises(_lib.UnsupportedOnDeviceError):     # not the ICASSP2018 sequence
    run_front(GROUPED, TTD, xs=[embeddings(300, d=16), embeddings(400, d=16)])
  with pytest.raises(_lib.UnsupportedOnDeviceError):     # a sweep below n = 512
    run_front(SWEEP, ICASSP, xs=[embeddings(300)], ps=SWEEP_P)
  with pytest.raises(_lib.UnsupportedOnDeviceError):     # one value: evaluated on its own
    run_front(SWEEP, ICASSP, xs=[embeddings(600)], ps=(0.95,))
