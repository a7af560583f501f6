"""CPU: the references of the dense-route GPU tests (tests/_tridiag_ref.py) against LAPACK, so
that what the device kernels are compared with is itself pinned.

  * the reflector convention: q_from_reflectors / apply_q on the output of dsytrd(lower)
    reproduce dorgtr, and Q^T M Q is the tridiagonal dsytrd returned;
  * sturm_multisection (k_td_bounds + k_td_bisect with IEEE division) stays inside the bar the
    device is held to, 8 eps G of LAPACK's bisection dstebz, on every input of the GPU test;
  * the generated inputs are what their names say."""

import numpy as np
import pytest
from scipy.linalg import eigvalsh_tridiagonal, lapack

import _tridiag_ref as tr


def stebz(d, e):
  """Every eigenvalue of tridiag(d, e) by LAPACK's bisection, descending."""
  if len(d) == 1:
    return np.array(d, dtype=np.float64)
  return eigvalsh_tridiagonal(d, e, lapack_driver="stebz")[::-1]


def lapack_reflectors(m):
  """dsytrd(uplo='L') in the storage of launch_tridiagonalize_blocked."""
  n = m.shape[0]
  c, d, e, tau, info = lapack.dsytrd(m, lower=1)
  assert info == 0
  r = np.full((n, n), np.nan)          # nothing but row j, columns j+1 .. n-1 may be read
  for j in range(n - 1):
    r[j, j + 1] = 1.0
    r[j, j + 2:] = c[j + 2:, j]
  return c, d, e, np.concatenate([tau, [0.0]]), r


def dorgtr_lower(c, tau):
  """LAPACK's dorgtr(uplo='L'), which SciPy does not wrap, as dorgtr itself computes it: the
  reflectors shifted one column to the left, dorgqr on the trailing (n-1, n-1) block, a leading
  1 on the diagonal."""
  n = c.shape[0]
  q = np.eye(n)
  q[1:, 1:], _, info = lapack.dorgqr(c[1:, :n - 1], tau)
  assert info == 0
  return q


@pytest.mark.parametrize("n", [2, 3, 33, 130])
def test_reflector_convention_reproduces_dorgtr(n):
  m = tr.gaussian_sym(n, n)
  c, d, e, tau, r = lapack_reflectors(m)
  want = dorgtr_lower(c, tau[:n - 1])
  q = tr.q_from_reflectors(r, tau)
  assert np.max(np.abs(q - want)) <= n * tr.EPS
  assert np.max(np.abs(q.T @ q - np.eye(n))) <= n * tr.EPS
  scale = np.abs(np.linalg.eigvalsh(m)).max()
  assert np.max(np.abs(q.T @ m @ q - tr.tridiag(d, e))) <= 4 * n * tr.EPS * scale
  # apply_q is the same product, column by column
  z = np.eye(n)[:, [0, n // 2, n - 1]]
  assert np.max(np.abs(tr.apply_q(r, tau, z).astype(np.float64) - want[:, [0, n // 2, n - 1]])) \
      <= n * tr.EPS
  assert np.array_equal(tr.apply_q(r, tau, np.eye(n)).astype(np.float64), q)


def test_zero_tau_is_the_identity():
  n = 40
  r = np.full((n, n), np.nan)
  tau = np.zeros(n)
  assert np.array_equal(tr.q_from_reflectors(r, tau), np.eye(n))
  z = np.random.default_rng(0).standard_normal((n, 3))
  assert np.array_equal(tr.apply_q(r, tau, z).astype(np.float64), z)


def test_tridiag_and_gershgorin():
  d, e = np.array([1.0, -2.0, 3.0]), np.array([0.5, -4.0, 99.0])   # (a longer e is cut)
  t = tr.tridiag(d, e)
  assert np.array_equal(t, np.array([[1.0, 0.5, 0.0], [0.5, -2.0, -4.0], [0.0, -4.0, 3.0]]))
  assert tr.gershgorin_norm(d, e) == 7.0
  assert tr.gershgorin_norm(np.array([-3.0]), np.zeros(0)) == 3.0
  assert tr.gershgorin_norm(np.zeros(5), np.zeros(4)) == 0.0


CASES = tr.tridiagonal_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_multisection_emulation_within_the_device_bar(name):
  d, e = CASES[name]
  got = tr.sturm_multisection(d, e)
  want = stebz(d, e)
  assert got.shape == want.shape and np.all(np.diff(got) <= 0.0)
  g = tr.gershgorin_norm(d, e)
  err = float(np.max(np.abs(got - want)))
  print("%s: n=%d  error %.3g = %.3g eps G" % (name, len(d), err, err / (tr.EPS * g) if g else 0))
  assert err <= (8 * tr.EPS * g if g > 0 else 1e-270)


def test_multisection_emulation_on_closed_forms():
  d, e = CASES["toeplitz300"]
  want = np.sort(tr.toeplitz_eigenvalues(300))[::-1]
  assert np.max(np.abs(tr.sturm_multisection(d, e) - want)) <= 8 * tr.EPS * 4.0
  d, e = CASES["clement200"]
  want = np.arange(199, -200, -2, dtype=np.float64)
  assert np.max(np.abs(tr.sturm_multisection(d, e) - want)) <= 8 * tr.EPS * tr.gershgorin_norm(d, e)
  assert np.array_equal(tr.sturm_multisection(np.array([2.5]), np.zeros(0)), [2.5])


def test_generated_inputs():
  assert tr.block_sizes(300) == [70, 80, 90, 60] and sum(tr.block_sizes(161)) == 161
  for n in tr.STRUCTURE_SIZES:
    for name in tr.STRUCTURES:
      m, c, p = tr.structure(name, n)
      op = tr.materialized(m, c, p)
      assert op.shape == (n, n) and np.array_equal(op, op.T) and np.all(np.isfinite(op)), name
    m, _, _ = tr.structure("block_diagonal", n)
    s = tr.block_sizes(n)
    assert not m[:s[0], s[0]:].any() and m[:s[0], :s[0]].all()
    m, c, p = tr.structure("scaled", n)
    assert c.min() > 0 and c.max() / c.min() > 1e4 and (p < 0).any() and (p > 0).any()
  for n in tr.SPECTRA_SIZES:
    for name in tr.SPECTRA:
      m, descend = tr.spectrum_case(name, n)
      assert m.shape == (n, n) and np.array_equal(m, m.T), name
    w = np.linalg.eigvalsh(tr.spectrum_case("laplacian4", n)[0])
    assert np.abs(w[:4]).max() < 1e-14 and w[4] > 0.1
    w = np.linalg.eigvalsh(tr.spectrum_case("multiplicity70", n)[0])
    assert np.abs(w[-70:] - 2.0).max() < 1e-13 and w[-71] < 1.6
  d, e = tr.glued_wilkinson(10, 1e-14)
  assert d.shape == (210,) and e.shape == (209,) and np.count_nonzero(e == 1e-14) == 9
