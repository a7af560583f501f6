"""GPU: the kernels of the dense symmetric route (csrc/eig_dense.hip), each alone, through the
launchers the route calls (`sc_stage_tridiag`, `sc_stage_tridiag_values`,
`sc_stage_td_backtransform`; references in tests/_tridiag_ref.py, pinned on the CPU by
test_tridiag_reference_host.py).  Every entry fills the padding columns, the panel, the work
vectors and the results with NaNs first.

A. Tridiagonalisation (k_td_materialize, k_tdb_column, k_tdb_symv, k_tdb_panel_end, the in-place
   MFMA trailing update).  With T from the returned d, e and Q accumulated in longdouble from the
   returned reflectors:
     (i)   |Q^T Q - I|_max            <= max(8 x LAPACK's figure, n eps)
     (ii)  |Q^T M Q - T|_max / ||M||_2 <= max(8 x LAPACK's figure, n eps)
     (iii) tau[j] in {0} u [1, 2], tau[n-1] = 0, e[n-1] = 0, v_j[j+1] = 1 as stored
     (iv)  d, e, tau and the reflectors are finite
   LAPACK's figures are those of scipy.linalg.hessenberg(M, calc_q=True) on the same matrix,
   evaluated by the same fp64 products; n eps is the order of the textbook bound of a Householder
   reduction and stands in where LAPACK's figure is 0 (diagonal input).  eps = 2.22e-16.
   Sizes: a last panel of 1, 2, 31, 32 columns and one column into the next (129 .. 193), trailing
   blocks across the GEMM's 128-tiles (255 .. 257), 32 rows per column workgroup and idle column
   workgroups (513, 545), more than 64 rows per column workgroup (2081: eigenvalues of T against
   eigvalsh(M), five back-transformed eigenvectors by residual -- Q in longdouble would take a
   minute there).

B. Sturm multisection alone (k_td_bounds, k_td_bisect, td_rcp) on tridiagonals given directly:
   max|got - dstebz| <= 8 eps G, G the Gershgorin norm (the IEEE-division restatement holds
   1.28 eps G on these inputs; the rest is for the reciprocal with two Newton steps), sorted
   descending; the zero matrix to 1e-270 (pivmin governs).

C. Back-transform alone (k_td_backtransform<true> / <false>): |got - Q z|_max <= n eps for unit
   columns, Q z in longdouble; the LDS kernel with one and two entries per thread, above 64 KB of
   dynamic LDS (n = 8200) and the global-memory kernel, forced, bit for bit the LDS kernel's.

Measured on an MI355X when this file was written (every test prints its figures; -s shows them).
A, device / LAPACK, (i) orthogonality | (ii) reduction -- the bar is 8:
  gaussian   129 0.71|0.60  130 1.00|0.67  159 0.79|0.80  160 0.92|0.82  161 0.92|1.00
             192 0.67|0.83  193 0.75|0.87  255 0.83|0.87  256 1.33|0.90  257 1.00|1.00
             513 0.71|0.89  545 0.83|1.09
  n =              161         300                        161         300
  diagonal       0 = 0       0 = 0        tridiagonal   0 = 0       0 = 0     (both sides exact)
  block_diagonal 1.00|0.75   1.00|0.86    rank3         1.10|2.50   1.00|1.27
  graded         0.90|1.25   1.17|0.60    zero_border   0.57|1.14   0.88|0.78
  scaled         0.83|0.67   0.64|0.85    tiny (1e-150) 0.71|1.29   1.00|1.18
  huge (1e+150)  0.70|1.14   1.17|0.93
  (absolute: (i) 8e-16 .. 1.8e-15, (ii) 2.4e-16 .. 1.2e-15; the n eps floor, 2.9e-14 .. 1.2e-13,
  decides only where LAPACK's figure is 0.)  n = 2081: eigenvalues 1.6e-16 scale sqrt(n) (bar
  1e-12), residual of the five vectors 2.0e-16 ||M|| (bar 3.7e-12).
B: at most 1.28 eps G (clement200; wilkinson101 1.26), and on every input the same error as the
  IEEE-division restatement to three digits.  The unscaled squares of k_tdb_column / k_td_bounds
  hold at 1e+-150 and 1e+-100; nothing was changed in the kernels.
C: Z = I 0.0081 / 0.0039 / 0.0013 n eps at n = 129 / 300 / 1025; n = 8200 1.4e-5 n eps; the
  global-memory kernel bit for bit the LDS kernel's at 300 and 1025.
"""

import functools

import numpy as np
import pytest
import scipy.linalg

import _tridiag_ref as tr
from spectralcluster_amd import _lib

pytestmark = pytest.mark.gpu

EPS = tr.EPS
GLOBAL_KERNEL = 1   # SC_TD_BACKTRANSFORM_GLOBAL


# ------------------------------------------------------------------------------ entries
def tridiagonalize(handle, m, c=None, p=None):
  """-> d, e, tau (n each), reflectors (n, n) of Op = diag(p) + diag(c) m diag(c)."""
  n = m.shape[0]
  m = np.ascontiguousarray(m, dtype=np.float64)
  d, e, tau = (np.full(n, np.nan) for _ in range(3))
  refl = np.full((n, n), np.nan)
  vec = lambda a: None if a is None else _lib.as_double_p(np.ascontiguousarray(a, dtype=np.float64))
  handle.check(handle.lib.sc_stage_tridiag(
      handle.raw, _lib.as_double_p(m), n, vec(c), vec(p), _lib.as_double_p(d),
      _lib.as_double_p(e), _lib.as_double_p(tau), _lib.as_double_p(refl)))
  return d, e, tau, refl


def tridiagonal_values(handle, d, e):
  n = len(d)
  d = np.ascontiguousarray(d, dtype=np.float64)
  e = np.ascontiguousarray(e, dtype=np.float64)
  out = np.full(n, np.nan)
  handle.check(handle.lib.sc_stage_tridiag_values(
      handle.raw, _lib.as_double_p(d), _lib.as_double_p(e) if n > 1 else None, n,
      _lib.as_double_p(out)))
  return out


def back_transform(handle, refl, tau, z, flags=0):
  n, cols = z.shape
  out = np.ascontiguousarray(z, dtype=np.float64).copy()
  refl = np.ascontiguousarray(refl, dtype=np.float64)
  tau = np.ascontiguousarray(tau, dtype=np.float64)
  handle.check(handle.lib.sc_stage_td_backtransform(
      handle.raw, _lib.as_double_p(refl), _lib.as_double_p(tau), n, _lib.as_double_p(out), cols,
      flags))
  return out


def only_reflectors(refl):
  """What the back-transform may read: row j, columns j+1 .. n-1.  Everything else -> NaN."""
  out = np.full_like(refl, np.nan)
  iu = np.triu_indices(refl.shape[0], 1)
  out[iu] = refl[iu]
  return out


# ------------------------------------------------------------------------------ A
def check_outputs(n, d, e, tau, refl):
  """(iii) and (iv)."""
  iu = np.triu_indices(n, 1)
  assert np.all(np.isfinite(d)) and np.all(np.isfinite(e)) and np.all(np.isfinite(tau)), \
      "NaN padding or workspace reached d / e / tau"
  assert np.all(np.isfinite(refl[iu])), "NaN padding or workspace reached a reflector"
  assert tau[n - 1] == 0.0 and e[n - 1] == 0.0
  assert np.all((tau == 0.0) | ((tau >= 1.0) & (tau <= 2.0))), tau[(tau != 0) & ((tau < 1) | (tau > 2))]
  assert np.all(refl[np.arange(n - 1), np.arange(1, n)] == 1.0)


def reduction_figures(op, q, t):
  norm = float(np.abs(np.linalg.eigvalsh(op)).max())
  orth = float(np.abs(q.T @ q - np.eye(op.shape[0])).max())
  res = float(np.abs(q.T @ op @ q - t).max()) / norm
  return orth, res


def check_reduction(handle, name, m, c=None, p=None):
  n = m.shape[0]
  op = tr.materialized(m, c, p)
  d, e, tau, refl = tridiagonalize(handle, m, c, p)
  check_outputs(n, d, e, tau, refl)
  orth, res = reduction_figures(op, tr.q_from_reflectors(refl, tau), tr.tridiag(d, e))
  hl, ql = scipy.linalg.hessenberg(op, calc_q=True)
  orth_l, res_l = reduction_figures(op, ql, hl)
  floor = n * EPS
  print("%s n=%d: |Q^T Q - I| %.3g (LAPACK %.3g, ratio %.2f)  |Q^T M Q - T| / ||M|| %.3g "
        "(LAPACK %.3g, ratio %.2f)  floor n eps %.3g" % (
            name, n, orth, orth_l, orth / orth_l if orth_l else np.inf, res, res_l,
            res / res_l if res_l else np.inf, floor))
  assert orth <= max(8 * orth_l, floor), (name, n, "orthogonality", orth, orth_l)
  assert res <= max(8 * res_l, floor), (name, n, "reduction", res, res_l)
  return d, e, tau, refl


GAUSSIAN_SIZES = (129, 130, 159, 160, 161, 192, 193, 255, 256, 257, 513, 545)


@pytest.mark.parametrize("n", GAUSSIAN_SIZES)
def test_tridiagonalisation_gaussian(handle, n):
  check_reduction(handle, "gaussian", tr.gaussian_sym(n, n))


@pytest.mark.parametrize("n", tr.STRUCTURE_SIZES)
@pytest.mark.parametrize("name", tr.STRUCTURES)
def test_tridiagonalisation_structured(handle, name, n):
  m, c, p = tr.structure(name, n)
  d, e, tau, refl = check_reduction(handle, name, m, c, p)
  if name == "diagonal":
    assert not tau.any() and not e.any() and np.array_equal(d, np.diag(m))
  if name == "tridiagonal":
    # nothing to eliminate: T is the input, bit for bit, whatever sign LAPACK would give e
    assert not tau.any() and np.array_equal(d, np.diag(m)) and np.array_equal(e[:-1], np.diag(m, 1))
  if name == "block_diagonal":
    ends = np.cumsum(tr.block_sizes(n))[:-1]
    assert not tau[ends - 2].any() and np.all(e[ends - 2] != 0.0)   # tau = 0 with alpha != 0
    assert not e[ends - 1].any()                                     # the blocks stay apart
  if name == "scaled":
    # Materialisation: the columns of the first panel below row 32 are never written by the
    # reduction (only the trailing block is updated), so they still hold what k_td_materialize
    # left there: (c_i c_j) m_ij to the bit, hence exactly symmetric -- and d[0] carries p.
    op = tr.materialized(m, c, p)
    assert np.array_equal(refl[32:, :32], op[32:, :32])
    assert np.array_equal(refl[32:, :32], op[:32, 32:].T)
    assert d[0] == op[0, 0]


def test_tridiagonalisation_2081(handle):
  """Rows > 2048: more than 64 rows per workgroup of k_tdb_column."""
  n = 2081
  m = tr.gaussian_sym(n, n)
  d, e, tau, refl = tridiagonalize(handle, m)
  check_outputs(n, d, e, tau, refl)
  want = np.linalg.eigvalsh(m)
  scale = np.abs(want).max()
  got = scipy.linalg.eigvalsh_tridiagonal(d, e[:-1])
  err = np.abs(got - want).max()
  # five eigenvectors of T (LAPACK dstein) back-transformed on the device: unit columns whose
  # residual against M carries the backward error of the reduction, c n eps ||M||, with c = 8
  # as in the bars above
  pairs = [scipy.linalg.eigh_tridiagonal(d, e[:-1], select="i", select_range=(i, i))
           for i in (0, 1, n // 2, n - 2, n - 1)]
  w = np.array([pw[0] for pw, _ in pairs])
  z = np.stack([pz[:, 0] for _, pz in pairs], axis=1)
  x = back_transform(handle, only_reflectors(refl), tau, z)
  res = np.abs(m @ x - x * w).max()
  norms = np.linalg.norm(x, axis=0)
  print("n=2081: eigenvalues of T vs eigvalsh(M) %.3g of scale sqrt(n); residual of 5 "
        "back-transformed vectors %.3g ||M|| (bar %.3g); column norms - 1: %.3g" % (
            err / (scale * np.sqrt(n)), res / scale, 8 * n * EPS, np.abs(norms - 1).max()))
  assert err < 1e-12 * scale * np.sqrt(n)
  assert res <= 8 * n * EPS * scale
  assert np.abs(norms - 1).max() <= n * EPS


# ------------------------------------------------------------------------------ B
TRIDIAGONALS = tr.tridiagonal_cases()


@pytest.mark.parametrize("name", sorted(TRIDIAGONALS))
def test_sturm_multisection(handle, name):
  d, e = TRIDIAGONALS[name]
  n = len(d)
  got = tridiagonal_values(handle, d, e)
  assert np.all(np.isfinite(got)), "NaN workspace reached an eigenvalue"
  assert np.all(np.diff(got) <= 0.0), "not sorted descending"
  want = (scipy.linalg.eigvalsh_tridiagonal(d, e, lapack_driver="stebz")[::-1] if n > 1
          else np.array(d))
  g = tr.gershgorin_norm(d, e)
  err = float(np.abs(got - want).max())
  emu = float(np.abs(tr.sturm_multisection(d, e) - want).max())
  print("%s n=%d: error %.3g = %.3g eps G (IEEE-division restatement: %.3g eps G)" % (
      name, n, err, err / (EPS * g) if g else 0.0, emu / (EPS * g) if g else 0.0))
  if g == 0.0:
    assert err <= 1e-270
  else:
    assert err <= 8 * EPS * g
  if name == "toeplitz300":
    closed = np.sort(tr.toeplitz_eigenvalues(n))[::-1]
    assert np.abs(got - closed).max() <= 8 * EPS * g


# ------------------------------------------------------------------------------ C
@functools.lru_cache(maxsize=None)
def _device_reflectors(n):
  """Reflectors of a Gaussian matrix as the device reduction leaves them (held by A at these
  sizes' neighbours), cut down to what the back-transform may read."""
  d, e, tau, refl = tridiagonalize(_lib.default_handle(), tr.gaussian_sym(n, 31 + n))
  return only_reflectors(refl), tau


@pytest.mark.parametrize("n", [129, 300])
def test_back_transform_identity(handle, n):
  refl, tau = _device_reflectors(n)
  got = back_transform(handle, refl, tau, np.eye(n))
  want = tr.apply_q(refl, tau, np.eye(n))
  err = float(np.abs(got.astype(tr.LD) - want).max())
  print("n=%d: |Q I - Q|_max %.3g = %.3g n eps" % (n, err, err / (n * EPS)))
  assert np.all(np.isfinite(got)) and err <= n * EPS
  # (c) the global-memory kernel: the same operations in the same order
  if n == 300:
    assert np.array_equal(back_transform(handle, refl, tau, np.eye(n), GLOBAL_KERNEL), got)


def test_back_transform_identity_1025(handle):
  """Thread 0 owns two entries, 0 and 1024 (never both under one reflector: several entries per
  thread and reflector are the n = 8200 and n = 2081 cases).  All 1025 columns run; the
  longdouble product of all of them takes ten seconds on the host, so 63 columns (the first,
  the last, both sides of entry 1024 and a spread) are held to n eps against longdouble and ALL
  columns to 2 n eps against the same accumulation in fp64 -- n eps for the device, n eps for
  that reference's own rounding."""
  n = 1025
  refl, tau = _device_reflectors(n)
  got = back_transform(handle, refl, tau, np.eye(n))
  assert np.all(np.isfinite(got))
  cols = np.unique(np.concatenate([[0, 1, 2, 1022, 1023, 1024], np.arange(7, n, 18)]))
  assert cols.size == 63 and cols[-1] == 1024
  want = tr.apply_q(refl, tau, np.eye(n)[:, cols])
  err = float(np.abs(got[:, cols].astype(tr.LD) - want).max())
  q64 = np.eye(n)
  for j in range(n - 2, -1, -1):
    v = refl[j, j + 1:]
    q64[j + 1:, j + 1:] -= tau[j] * np.outer(v, v @ q64[j + 1:, j + 1:])
  err64 = float(np.abs(got - q64).max())
  print("n=1025: 63 columns vs longdouble %.3g n eps; all columns vs fp64 %.3g n eps" % (
      err / (n * EPS), err64 / (n * EPS)))
  assert err <= n * EPS
  assert err64 <= 2 * n * EPS
  # (c) the global-memory kernel: the same operations in the same order
  assert np.array_equal(back_transform(handle, refl, tau, np.eye(n), GLOBAL_KERNEL), got)


def test_back_transform_above_64k_of_lds(handle):
  """n = 8200: 65600 bytes of dynamic LDS, past the default limit (the opt-in path).  About
  forty synthetic reflectors -- the first, the last, and those whose leading entry j + 1 is 0, 1
  or 1023 (mod 1024), where the entry a thread starts from changes -- every other tau = 0 and
  every other row NaN."""
  n = 8200
  rng = np.random.default_rng(8200)
  js = {0, n - 2}
  for k in range(1, 9):
    js |= {1024 * k - 1, 1024 * k, 1024 * k - 2}
  js = sorted(j for j in js if j <= n - 2)
  js = sorted(set(js) | set(int(j) for j in rng.choice(n - 2, 42 - len(js), replace=False)))
  refl = np.full((n, n), np.nan)
  tau = np.zeros(n)
  for j in js:
    v = np.concatenate([[1.0], rng.standard_normal(n - j - 2)])
    refl[j, j + 1:] = v
    tau[j] = 2.0 / (v @ v)
  z = rng.standard_normal((n, 3))
  z /= np.linalg.norm(z, axis=0)
  got = back_transform(handle, refl, tau, z)
  err = float(np.abs(got.astype(tr.LD) - tr.apply_q(refl, tau, z)).max())
  print("n=8200, %d reflectors: error %.3g = %.3g n eps" % (len(js), err, err / (n * EPS)))
  assert np.all(np.isfinite(got)) and err <= n * EPS
