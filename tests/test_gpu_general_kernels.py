"""GPU: the kernels of the general (non-symmetric) eigen path, each alone, through the launchers
the path calls (`sc_stage_hessenberg`, `sc_stage_general_ritz`, `sc_stage_arnoldi_state`;
references in tests/_hessenberg_ref.py and tests/_krylov_ref.py, pinned on the CPU by
test_hessenberg_reference_host.py and test_krylov_reference_host.py).  The first two entries fill
the padding columns, the work vectors and the results with NaNs first.

A. Hessenberg reduction (k_hess_first, k_hess_right, k_hess_left with the next reflector formed
   by workgroup 0, the max|a| read-back and the power-of-two scaling of the dense general route).
   H is the returned matrix cut to Hessenberg form, Q accumulated in longdouble from the returned
   reflectors:
     (i)   |Q^T Q - I|_max                   <= max(8 x LAPACK's figure, n eps)
     (ii)  |Q^T M Q - H scale|_max / ||M||_2  <= max(8 x LAPACK's figure, n eps)
     (iii) tau[k] in {0} u [1, 2], tau[n-2] = tau[n-1] = 0, everything finite, |v| <= 1 below
           the subdiagonal
     (iv)  a second call returns the same bits (every sum has a fixed order)
   LAPACK's figures are those of scipy.linalg.hessenberg(M, calc_q=True) on the same matrix,
   evaluated by the same function; n eps stands in where LAPACK's figure is 0.  eps = 2.22e-16.
   The scaling cases are Gaussians brought to max|a| in [0.5, 1) by a power of two first, so that
   "x 2^k" has the binary exponent k the driver's threshold (beyond 2^+-400) counts.
   A first column whose part below the subdiagonal is ~1e-170 next to entries of order 1 (only
   the first column can stay that small: the left updates mix every later one with its O(1)
   rows) is SKIPPED by hess_reflector (tau = 0): its squares underflow to 0, where dlarfg would rescale.  That is the
   kernel's behaviour and it is harmless: the entries left below the subdiagonal are below
   1e-160 ||M||, far under eps ||M||, and H cut to Hessenberg form meets (i) and (ii) like any
   other -- the cut is a backward error of 1e-170.

B. Rayleigh-Ritz kernels on given data (k_gen_ritz, k_gen_residual + k_gen_residual_reduce,
   k_gen_phase, k_gen_gather), u = 2^-53, gamma_k = k u / (1 - k u), exact = longdouble complex:
     Ritz vectors  |got - exact| <= gamma_m (|Q| |Y|) per entry; the identity form bit for bit
     residuals     |resid - ||r||_2| <= ||delta||_2 + gamma_{n+2} ||r||_2,
                   delta_i = gamma_{m+4} ((|OpQ| |y|)_i + |theta| (|Q| |y|)_i)   (absolute)
     phase         unit norm, pivot (first index of largest magnitude) real and positive with
                   |imaginary part| <= 4 u of it, every entry within phase_bound (15.5 u at
                   n <= 512, derived in the reference module) of v conj(v_p) / (|v_p| ||v||);
                   E bit-equal to the real part; a column with zero imaginary part keeps it
                   zero and is +-v / ||v||
     pivot ties    exactly representable ties at (5, 300), (255, 256), (300, 261), (0, n-1) and,
                   within one thread, (5, 261)
   m in {8, 24, 64, 128} x cols in {1, 31, 32, 33, 64} (cols <= m) x n in {65, 129, 263}; three
   kinds of data per shape: Gaussian Op with the eigenpairs of Q^T Op Q, small-integer Q and H
   with OpQ := Q H exactly (every pair converged, residual ~1e-13), six decades with signs.

C. What a block Arnoldi solve leaves behind (sc_stage_arnoldi_state): Q, Op Q, H, the scalings,
   held to rounding-level invariants; the bounds and the cases are at section C below.

Measured on an MI355X when this file was written (every test prints its figures; -s shows them).
A, device / LAPACK, (i) orthogonality | (ii) reduction -- the bar is 8:
  gaussian   3 1.00|1.00  4 1.00|1.00  5 0.33|0.75  33 1.00|1.00  34 0.62|0.75  35 0.83|0.62
             64 0.75|0.62  65 0.88|0.80  66 0.60|0.83  67 0.88|1.14  129 1.00|1.00
             257 1.20|0.77  258 0.83|0.73  259 0.92|0.71  300 0.71|1.20  512 1.09|1.00
             545 0.83|0.86   (n = 1, 2: nothing runs, 0 = 0)
  n =                 67          300                       67          300
  hessenberg, triangular, diagonal   0 = 0 (output = input bit for bit, every tau 0)
  block_diagonal  0.62|0.50   0.80|0.80    rank_one      1.12|1.18   0.93|1.06
  graded_rows     0.50|0.67   1.07|0.78    zero_border   0.69|0.80   0.86|0.83
  affinity        0.75|1.00   1.00|1.00    random_walk   0.88|1.00   1.08|1.00
  n = 67: 2^+-399 and 2^+-401 0.88|1.14 (the same bits up to the power of two; scale 1 and
  2^+-400)  1e-170 0.60|0.75  1e+160 1.00|1.00  tiny first column 0.75|1.00 (tau[0] = 0, the
  column left as it came, 2.9e-170 below the subdiagonal)
  (absolute: (i) 1.1e-16 .. 1.8e-15, (ii) 7e-17 .. 1.8e-15; the n eps floor decides only where
  LAPACK's figure is 0.)  Nothing was changed in the kernels.
B, worst error / bound over the 36 shapes:   Ritz vectors   residuals   phase
  gaussian                                      0.221        0.0029      0.292
  converged (||r|| 2e-12 .. 7e-12)              0.182        0.0016      0.346
  six decades                                   0.479        0.0176      0.319
  -- to three digits the figures of the fp64 restatements on the CPU
  (test_hessenberg_reference_host.py); |norm - 1| <= 4.4e-16; identity form: copied bit for
  bit, phase 0.116 (n = 17) and 0.158 (n = 64); all five ties resolved to the first index.
C, measured | bound:  orthonormality 4.2e-16 .. 1.5e-15 | 5.4e-14 .. 2.6e-13 (the reference chain:
  5.4e-16 .. 1.8e-15);  Op Q 0.003 .. 0.060 of its bound;  H - Q^T OpQ 2e-16 .. 6.3e-15, at most
  0.005 of its bound;  Arnoldi property 1.5e-16 .. 7.3e-15 (reference chain 1e-16 .. 3.5e-15), at
  most 0.005 of its bound.  Restart cycles: 0 (cap56, pitch129), 1 (affinity, n = 300), 3 (the
  Laplacians at n = 520), 4 (wide, basis 128), 6 (the tight non-normal cluster).  The restarted
  bases are as clean as the others: the 1e-12 m max|H| allowance was not needed by any of them.
"""

import ctypes
import functools

import numpy as np
import pytest
import scipy.linalg

import _hessenberg_ref as hr
from spectralcluster_amd import _lib

pytestmark = pytest.mark.gpu

EPS = hr.EPS
U = hr.U


# ------------------------------------------------------------------------------ entries
def hessenberg(handle, m):
  """-> packed (n, n), tau (n), scale."""
  n = m.shape[0]
  m = np.ascontiguousarray(m, dtype=np.float64)
  packed, tau, scale = np.full((n, n), np.nan), np.full(n, np.nan), np.full(1, np.nan)
  handle.check(handle.lib.sc_stage_hessenberg(
      handle.raw, _lib.as_double_p(m), n, _lib.as_double_p(packed), _lib.as_double_p(tau),
      _lib.as_double_p(scale)))
  return packed, tau, float(scale[0])


def general_ritz(handle, q, opq, yre, yim, tre=None, tim=None, codes=None, seed=0):
  """-> dict of vre, vim, resid (when theta is given), pre, pim, e, w (when codes are given)."""
  m, cols = yre.shape
  n = m if q is None else q.shape[0]
  c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
  p = lambda a: None if a is None else _lib.as_double_p(a)
  q, opq, yre, yim, tre, tim = c(q), c(opq), c(yre), c(yim), c(tre), c(tim)
  out = {k: np.full((n, cols), np.nan) for k in ("vre", "vim", "pre", "pim", "e")}
  out["resid"] = None if tre is None else np.full(cols, np.nan)
  out["w"] = None if codes is None else np.full((n, hr.B), np.nan)
  cd = None
  if codes is not None:
    cd = np.ascontiguousarray(codes, dtype=np.int32)
    assert cd.shape == (hr.B,)
  handle.check(handle.lib.sc_stage_general_ritz(
      handle.raw, p(q), p(opq), n, m, p(yre), p(yim), p(tre), p(tim), cols, p(out["vre"]),
      p(out["vim"]), p(out["resid"]), p(out["pre"]), p(out["pim"]), p(out["e"]),
      None if cd is None else cd.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), seed,
      p(out["w"])))
  return out


# ------------------------------------------------------------------------------ A
def check_shape(n, packed, tau):
  """(iii)."""
  assert np.all(np.isfinite(packed)) and np.all(np.isfinite(tau)), \
      "NaN padding or workspace reached the result"
  assert np.all((tau == 0.0) | ((tau >= 1.0) & (tau <= 2.0))), tau[(tau != 0) & ((tau < 1) | (tau > 2))]
  assert not tau[max(n - 2, 0):].any()
  assert np.all(np.abs(np.tril(packed, -2)) <= 1.0)


def check_reduction(handle, name, m, expect_scaled=None):
  n = m.shape[0]
  packed, tau, scale = hessenberg(handle, m)
  check_shape(n, packed, tau)
  if expect_scaled is not None:
    if expect_scaled:
      amax = float(np.abs(m).max())
      assert scale == hr.power_of_two_below(amax) and 1.0 <= amax / scale < 2.0, (name, scale)
    else:
      assert scale == 1.0, (name, scale)
  again = hessenberg(handle, m)
  assert np.array_equal(again[0], packed) and np.array_equal(again[1], tau) and again[2] == scale, \
      "two calls differ: the reduction is not a deterministic function of its input"   # (iv)
  orth, res = hr.reduction_figures(m, hr.q_from_packed(packed, tau), hr.hessenberg_part(packed),
                                   scale)
  hl, ql = scipy.linalg.hessenberg(m, calc_q=True)
  orth_l, res_l = hr.reduction_figures(m, ql, hl)
  floor = n * EPS
  print("%s n=%d: |Q^T Q - I| %.3g (LAPACK %.3g, ratio %.2f)  |Q^T M Q - H| / ||M|| %.3g "
        "(LAPACK %.3g, ratio %.2f)  floor n eps %.3g  scale %g" % (
            name, n, orth, orth_l, orth / orth_l if orth_l else np.inf, res, res_l,
            res / res_l if res_l else np.inf, floor, scale))
  assert orth <= max(8 * orth_l, floor), (name, n, "orthogonality", orth, orth_l)
  assert res <= max(8 * res_l, floor), (name, n, "reduction", res, res_l)
  return packed, tau, scale


@pytest.mark.parametrize("n", hr.GAUSSIAN_SIZES)
def test_hessenberg_gaussian(handle, n):
  m = hr.gaussian(n)
  packed, tau, scale = check_reduction(handle, "gaussian", m, expect_scaled=False)
  if n <= 2:   # nothing runs: the output is the input
    assert np.array_equal(packed, m) and not tau.any()
  else:
    assert np.all(tau[:n - 2] >= 1.0)


@pytest.mark.parametrize("n", hr.STRUCTURE_SIZES)
@pytest.mark.parametrize("name", hr.STRUCTURES)
def test_hessenberg_structured(handle, name, n):
  m = hr.structure(name, n)
  packed, tau, scale = check_reduction(handle, name, m, expect_scaled=False)
  if name in ("hessenberg", "triangular", "diagonal"):
    # nothing to annihilate: every tau is 0 and the output is the input bit for bit
    assert not tau.any() and np.array_equal(packed, m)
  if name == "block_diagonal":
    ends = np.cumsum(hr.block_sizes(n))[:-1]
    # column e - 2 of a block that ends before row e has nothing below its subdiagonal entry
    # but zeros of the next block: tau = 0 with a non-zero alpha; the zeros across blocks stay
    # exact zeros
    assert not tau[ends - 2].any() and np.all(packed[ends - 1, ends - 2] != 0.0)
    assert not tau[ends - 1].any()   # column e - 1: everything from row e on is zero
    for e in ends:
      assert not packed[e:, :e].any() and not packed[:e, e:].any(), "a zero across blocks moved"
  if name == "zero_border":
    assert not tau[:40].any() and not packed[:, :40].any() and not packed[:40].any()


@pytest.mark.parametrize("name", hr.SCALINGS)
def test_hessenberg_scaling(handle, name):
  m, rescaled = hr.scaled(name, 67)
  check_reduction(handle, name, m, expect_scaled=rescaled)


def test_hessenberg_underflowing_column_is_skipped(handle):
  """See the module docstring (A, last paragraph)."""
  n = 67
  m = hr.tiny_column(n)
  packed, tau, scale = check_reduction(handle, "tiny_column", m, expect_scaled=False)
  below = np.abs(packed[2:, 0])
  print("tiny column: tau[0] = %g, max below the subdiagonal %.3g" % (tau[0], below.max()))
  # skipped: tau = 0 and the column is the input's, bit for bit
  assert tau[0] == 0.0 and np.array_equal(packed[:, 0], m[:, 0]) and below.max() < 1e-160
  assert np.all(tau[1:n - 2] >= 1.0)


# ------------------------------------------------------------------------------ B
def _complex(re, im):
  return re.astype(hr.LD) + 1j * im.astype(hr.LD)


def check_phase(n, out, label):
  """The phase kernel on the device's own Ritz vectors (vre, vim) -> (pre, pim, e)."""
  vre, vim, pre, pim, e = (out[k] for k in ("vre", "vim", "pre", "pim", "e"))
  cols = vre.shape[1]
  assert all(np.all(np.isfinite(a)) for a in (pre, pim, e)), "NaN padding reached the phase"
  assert np.array_equal(e, pre), "E is not the real part as written"
  gap = hr.phase_pivot_gap(vre, vim)
  assert gap.min() >= 1e-6, (label, "input: the pivot is a rounding matter", gap.min())
  piv = hr.phase_pivot(vre, vim)
  exact = hr.phase_exact(vre, vim)
  got = _complex(pre, pim)
  real_col = ~vim.any(axis=0)
  # a zero-imaginary column: stays real, +-v / ||v||; LAPACK fixes no sign and neither do we
  assert not pim[:, real_col].any()
  sign = np.where(real_col & (np.sign(pre[piv, np.arange(cols)]) < 0), -1.0, 1.0)
  err = np.abs(got * sign[None, :] - exact).astype(np.float64)
  bound = hr.phase_bound(n, exact).astype(np.float64)
  ok = bound > 0
  ratio = float((err[ok] / bound[ok]).max())
  assert not err[~ok].any()
  norms = np.sqrt(np.sum(got.real ** 2 + got.imag ** 2, axis=0)).astype(np.float64)
  pr, pi = pre[piv, np.arange(cols)], pim[piv, np.arange(cols)]
  cplx = ~real_col
  assert np.all(pr[cplx] > 0.0), (label, "the pivot component is not positive")
  assert np.all(np.abs(pi[cplx]) <= 4 * U * pr[cplx]), (label, "the pivot component is not real")
  assert np.abs(norms - 1.0).max() <= hr.phase_terms(n) * U, (label, "not unit norm")
  assert ratio <= 1.0, (label, "phase", ratio)
  return ratio, float(np.abs(norms - 1.0).max())


@pytest.mark.parametrize("n,m,cols", hr.ritz_shapes())
def test_ritz_kernels(handle, n, m, cols):
  for kind in hr.RITZ_KINDS:
    label = (kind, n, m, cols)
    q, opq, yre, yim, tre, tim = hr.ritz_case(kind, n, m, cols)
    if kind != "decades" and cols > 2:
      assert tim.any(), "no complex pair among the inputs"
    out = general_ritz(handle, q, opq, yre, yim, tre, tim)
    assert all(np.all(np.isfinite(out[k])) for k in ("vre", "vim", "resid")), \
        (label, "NaN padding or workspace reached a result")
    err = np.abs(_complex(out["vre"], out["vim"]) - hr.ritz_exact(q, yre, yim)).astype(np.float64)
    r_ritz = float((err / hr.ritz_bound(q, yre, yim)).max())
    want = hr.residual_exact(q, opq, yre, yim, tre, tim).astype(np.float64)
    rb = hr.residual_bound(q, opq, yre, yim, tre, tim)
    r_res = float((np.abs(out["resid"] - want) / rb).max())
    r_phase, norm_err = check_phase(n, out, label)
    print("%s n=%d m=%d cols=%d: error / bound  ritz %.3f  residual %.4f (||r|| %.2e .. %.2e)  "
          "phase %.3f  |norm - 1| %.2e" % (kind, n, m, cols, r_ritz, r_res, want.min(),
                                           want.max(), r_phase, norm_err))
    assert r_ritz <= 1.0, (label, "ritz", r_ritz)
    assert r_res <= 1.0, (label, "residual", r_res)
    if kind == "converged":
      assert want.max() < 1e-9 * np.abs(opq).max()


@pytest.mark.parametrize("n", [17, 64])
def test_ritz_identity_form(handle, n):
  """Q == nullptr (the dense solver, n <= 64): V = Y, copied; then the phase."""
  rng = np.random.default_rng(n)
  w, y = np.linalg.eig(rng.standard_normal((n, n)))
  assert np.iscomplex(w).any() and not np.iscomplex(w).all()
  yre, yim = np.ascontiguousarray(y.real), np.ascontiguousarray(y.imag)
  out = general_ritz(handle, None, None, yre, yim)
  assert np.array_equal(out["vre"], yre) and np.array_equal(out["vim"], yim)
  ratio, norm_err = check_phase(n, out, ("identity", n))
  print("identity n=%d: phase error / bound %.3f, |norm - 1| %.2e" % (n, ratio, norm_err))


TIES = ((5, 300), (255, 256), (300, 5 + 256), (0, 332), (5, 5 + 256))


def test_phase_pivot_ties(handle):
  """Columns whose largest magnitude is taken twice, exactly: across threads, across the
  256-thread stride, first and last entry, and twice within one thread.  The columns reach the
  kernel as exact products: Q = [Vre | Vim], Yre = [I; 0], Yim = [0; I]."""
  n, k = 333, len(TIES)
  cols = [hr.tie_column(n, a, b, t) for t, (a, b) in enumerate(TIES)]
  vr = np.stack([c[0] for c in cols], axis=1)
  vi = np.stack([c[1] for c in cols], axis=1)
  eye, zero = np.eye(k), np.zeros((k, k))
  out = general_ritz(handle, np.concatenate([vr, vi], axis=1), None,
                     np.concatenate([eye, zero], axis=0), np.concatenate([zero, eye], axis=0))
  assert np.array_equal(out["vre"], vr) and np.array_equal(out["vim"], vi)
  check_phase(n, out, "ties")
  for c, (a, b) in enumerate(TIES):
    first, last = min(a, b), max(a, b)
    got = complex(out["pre"][first, c], out["pim"][first, c])
    other = complex(out["pre"][last, c], out["pim"][last, c])
    print("tie %s: pivot entry %r, the tied entry %r" % ((a, b), got, other))
    assert got.real > 0 and abs(got.imag) <= 4 * U * got.real, ((a, b), got)
    # the tied entry (+-0.5 + 0.5i against -+0.5 + 0.5i) is a quarter turn away from the pivot
    assert abs(other.real) <= 4 * U * abs(other.imag) and abs(abs(other.imag) - got.real) <= 4 * U


def test_restart_block_gather(handle):
  n, m, cols = 129, 24, 5
  q, opq, yre, yim, tre, tim = hr.ritz_case("gaussian", n, m, cols)
  codes = [2 * 0, 2 * 3 + 1, -1, 2 * 4, 2 * 4 + 1, -1, 2 * 1, 2 * 1 + 1]
  seed = 0x9E3779B97F4A7C16
  out = general_ritz(handle, q, opq, yre, yim, codes=codes, seed=seed)
  w = out["w"]
  assert np.all(np.isfinite(w))
  for j, code in enumerate(codes):
    if code >= 0:
      src = out["pim"] if code & 1 else out["pre"]
      assert np.array_equal(w[:, j], src[:, code >> 1]), (j, code)
    else:
      assert np.all((w[:, j] >= -1.0) & (w[:, j] < 1.0)) and np.unique(w[:, j]).size > n // 2
      assert np.array_equal(w[:, j], hr.gather_noise(n, j, seed)), "not the kernel's hash"
  assert not np.array_equal(w[:, 2], w[:, 5])
  again = general_ritz(handle, q, opq, yre, yim, codes=codes, seed=seed)
  assert np.array_equal(again["w"], w)
  other = general_ritz(handle, q, opq, yre, yim, codes=codes, seed=seed + 1)
  assert not np.array_equal(other["w"][:, 2], w[:, 2])
  assert np.array_equal(other["w"][:, 0], w[:, 0])


# ------------------------------------------------------------------------------ C
# What a block Arnoldi solve (gen_topk) leaves in the arena: Q, Q2 = Op Q, T = H of the final
# check, the scalings as the solve used them (sc_stage_arnoldi_state).  M is the matrix handed
# in; Op x = p .* x + cl .* (M (cr .* x)) and its products are evaluated in longdouble from M and
# the RETURNED cl, cr, p.  Bounds (derivations in tests/_krylov_ref.py, ArnoldiInvariants):
#   orthonormality   max |Q^T Q - I| <= 4 gamma_{n+m}
#   operator         |OpQ - Op Q| <= gamma_{n+4} (|p||Q| + |cl| (|M| (|cr||Q|)))
#   projection       |H - Q^T OpQ| <= 2 gamma_{n+m+8} |Q|^T |OpQ| + m orth max|H|
#   Arnoldi property |(I - Q Q^T) Op Q[:, 0:m-8]| <= operator bound + m orth max|H|
#                    + 16 x the same figure of the fp64 reference chain on the same operator
#                    (+ 1e-12 m max|H| after a restart: the kept Ritz vectors are Q Y with Y from
#                    the host solver, held to that bar by test_host_general_eig_vs_numpy)
#   scalings         diag(p) + diag(cl) M diag(cr) is minus the oracle's Laplacian of M
# Every case asserts the route it exists for through sc_diag and info.  An eigengap request
# below n = 513 takes the dense Hessenberg route by default, so the Laplacian cases run at
# n = 520, the smallest comfortable size above it; the cases that go through sc_stage_eig (a
# fixed count keeps the Krylov solver) run at the sizes their branch needs.
import _krylov_ref as kr
import spectral_oracle as so
import spectralcluster_amd as sca

BLOCK_ARNOLDI = 4


def arnoldi_state(handle):
  info = (ctypes.c_int32 * 8)()
  none = [None] * 6
  handle.check(handle.lib.sc_stage_arnoldi_state(handle.raw, info, *none))
  m, n = info[0], info[1]
  q, opq, hm = np.full((n, m), np.nan), np.full((n, m), np.nan), np.full((m, m), np.nan)
  cl, cr, p = (np.full(n, np.nan) for _ in range(3))
  handle.check(handle.lib.sc_stage_arnoldi_state(
      handle.raw, info, *[_lib.as_double_p(a) for a in (q, opq, hm, cl, cr, p)]))
  return dict(m=m, n=n, wide=bool(info[2]), cycles=info[3], passes=info[4], negate=bool(info[5]),
              q=q, opq=opq, h=hm, cl=cl, cr=cr, p=p)


def stage_eig(handle, m, count, descend=1):
  n = m.shape[0]
  m = np.ascontiguousarray(m, dtype=np.float64)
  values, vectors = np.empty(count), np.empty((n, count))
  diag = _lib.ScDiag()
  handle.check(handle.lib.sc_stage_eig(handle.raw, _lib.as_double_p(m), n, count, descend,
                                       _lib.as_double_p(values), _lib.as_double_p(vectors), diag))
  return diag, values


def eig_ncluster(matrix, lap, gap="Ratio", max_clusters=7):
  """sc_set_affinity + sc_eig_ncluster on the default handle: `matrix` as the refined matrix (no
  refinement), Laplacian `lap`."""
  clusterer = sca.SpectralClusterer(
      min_clusters=2, max_clusters=max_clusters,
      refinement_options=sca.RefinementOptions(refinement_sequence=[]),
      laplacian_type=sca.LaplacianType(lap) if lap else None,
      eigengap_type=getattr(sca.EigenGapType, gap))
  clusterer._compute_eigenvectors_ncluster(matrix)
  return clusterer.last_diag


ARNOLDI_CASES = ("cap56", "pitch129", "affinity_none", "random_walk", "graph_cut",
                 "ascending_normalized_diff", "restart", "wide")


@functools.lru_cache(maxsize=None)
def _case_matrix(name):
  if name == "cap56":
    return kr.separated_matrix(65)
  if name == "pitch129":
    return kr.separated_matrix(129)
  if name in ("affinity_none", "wide"):
    return hr.thresholded_affinity(300)
  if name == "restart":
    return kr.nonnormal_cluster(300)
  return hr.thresholded_affinity(520)


def run_arnoldi_case(handle, name):
  m = _case_matrix(name)
  lap = 0
  if name in ("cap56", "pitch129"):
    diag, _ = stage_eig(handle, m, 3)
  elif name == "affinity_none":
    diag, _ = stage_eig(handle, m, 4)
  elif name == "restart":
    diag, _ = stage_eig(handle, m, 12)
  elif name == "wide":
    diag, _ = stage_eig(handle, m, 40)
  else:
    lap = {"random_walk": so.LAPLACIAN_RANDOM_WALK, "graph_cut": so.LAPLACIAN_GRAPH_CUT,
           "ascending_normalized_diff": so.LAPLACIAN_RANDOM_WALK}[name]
    diag = eig_ncluster(m, lap, "NormalizedDiff" if name.startswith("ascending") else "Ratio")
    assert diag.symmetry_state == 3, "not the general path"
  assert diag.eig_path == BLOCK_ARNOLDI, (name, diag.eig_path, diag.eig_fallback)
  return m, lap, diag, arnoldi_state(handle)


@pytest.mark.parametrize("name", ARNOLDI_CASES)
def test_arnoldi_state_invariants(handle, name):
  mat, lap, diag, st = run_arnoldi_case(handle, name)
  n, m = st["n"], st["m"]
  assert n == mat.shape[0] and m % kr.B == 0 and 3 * kr.B <= m <= kr.arnoldi_cap(n, st["wide"])
  assert diag.eig_basis == m
  for key in ("q", "opq", "h", "cl", "cr", "p"):
    assert np.all(np.isfinite(st[key])), key
  # the branch the case exists for
  if name == "cap56":
    assert kr.arnoldi_cap(n) == 56 and not st["wide"]
  if name == "pitch129":
    assert n % 16 == 1 and not st["wide"]
  if name == "wide":
    assert st["wide"] and m > kr.GEN_MAX
  else:
    assert not st["wide"]
  # restarts: none where the spectrum is separated; the thresholded affinities take one to four
  # (a basis of 64 is 8 block steps), the tight non-normal cluster more
  if name in ("cap56", "pitch129"):
    assert st["cycles"] == 0
  if name == "restart":
    assert st["cycles"] >= 2
  if name != "ascending_normalized_diff":
    assert diag.eig_cycles == st["cycles"]
  if name == "ascending_normalized_diff":
    # a far-end solve with the sign turned came first: its passes are in sc_diag, the state is
    # the main solve's
    assert not st["negate"] and diag.eig_matvec_passes > st["passes"]
  else:
    assert diag.eig_matvec_passes == st["passes"] and not st["negate"]
  # the scalings are those of the Laplacian asked for
  if lap == so.LAPLACIAN_RANDOM_WALK:
    assert not np.array_equal(st["cl"], st["cr"]) and np.all(st["cr"] == 1.0)
  if lap:
    dense = np.diag(st["p"]) + st["cl"][:, None] * mat * st["cr"][None, :]
    want = -so.laplacian(mat, lap)
    assert np.abs(dense - want).max() <= 4 * kr.gamma(n) * max(1.0, np.abs(want).max())
  else:
    assert np.all(st["cl"] == 1.0) and np.all(st["cr"] == 1.0) and not st["p"].any()
  op = kr.Operator(mat, c=st["cl"], p=st["p"], s=st["cr"])
  inv = kr.ArnoldiInvariants(op, st["q"], st["opq"], st["h"])
  rq, ropq, rh = kr.ArnoldiChain(op).run(m).state()
  ref = kr.ArnoldiInvariants(op, rq, ropq, rh)
  restarted = st["cycles"] > 0
  ratio = inv.arnoldi_ratio(ref.arnoldi_figure(), restarted)
  print("%s n=%d m=%d wide=%d cycles=%d passes=%d: orth %.2e (bound %.2e, reference chain %.2e)  "
        "operator %.3f  projection %.2e (ratio %.3f)  Arnoldi %.2e (reference chain %.2e, "
        "ratio %.3f)" % (name, n, m, st["wide"], st["cycles"], st["passes"], inv.orth,
                         inv.orth_bound, ref.orth, inv.op_ratio(), float(inv.proj_err.max()),
                         inv.proj_ratio(), inv.arnoldi_figure(), ref.arnoldi_figure(), ratio))
  assert inv.orth <= inv.orth_bound
  assert inv.op_ratio() <= 1.0
  assert inv.proj_ratio() <= 1.0
  assert ratio <= 1.0


def test_arnoldi_state_is_refused_after_any_other_solve(handle):
  info = (ctypes.c_int32 * 8)()
  none = [None] * 6
  lib = handle.lib
  rng = np.random.default_rng(5)
  # the dense general solver (n <= 64)
  stage_eig(handle, rng.random((40, 40)), 3)
  assert lib.sc_stage_arnoldi_state(handle.raw, info, *none) == _lib.SC_ERR_INVALID
  assert "not block Arnoldi" in handle.last_error()
  # a block Arnoldi solve, then the dense Hessenberg route (more than 64 pairs)
  diag, _ = stage_eig(handle, hr.thresholded_affinity(129), 4)
  assert diag.eig_path == BLOCK_ARNOLDI
  assert lib.sc_stage_arnoldi_state(handle.raw, info, *none) == _lib.SC_OK and info[1] == 129
  diag, _ = stage_eig(handle, hr.thresholded_affinity(129), 70)
  assert diag.eig_path == 7
  assert lib.sc_stage_arnoldi_state(handle.raw, info, *none) == _lib.SC_ERR_INVALID
  # ... and a symmetric solve
  stage_eig(handle, hr.thresholded_affinity(129), 4)
  g = rng.standard_normal((200, 200))
  values, vectors = np.empty(3), np.empty((200, 3))
  sym = np.ascontiguousarray(g + g.T)
  handle.check(lib.sc_stage_sym_eig(handle.raw, _lib.as_double_p(sym), 200, 3, 1,
                                    _lib.as_double_p(values), _lib.as_double_p(vectors), None))
  assert lib.sc_stage_arnoldi_state(handle.raw, info, *none) == _lib.SC_ERR_INVALID
  assert lib.sc_stage_arnoldi_state(handle.raw, None, *none) == _lib.SC_ERR_INVALID
