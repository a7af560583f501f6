"""References for the dense symmetric route of csrc/eig_dense.hip, in plain NumPy: the orthogonal
factor of the reduction from the reflectors the device keeps (in `longdouble`), the Sturm-count
multisection of k_td_bounds / k_td_bisect restated with IEEE division, and the inputs of the GPU
tests test_gpu_tridiag_kernels.py / test_gpu_dense_eig.py.

Shared by tests/test_tridiag_reference_host.py (CPU: the reflector convention against LAPACK's
dsytrd / dorgtr, the restated multisection against LAPACK's bisection dstebz) and by the GPU
tests, so that what the device kernels are compared with is itself tested.

Storage, as launch_tridiagonalize_blocked leaves it: reflector j, v_j, in ROW j of the destroyed
matrix, columns j+1 .. n-1, with v_j[j+1] = 1 stored; H_j = I - tau_j v_j v_j^T;
Q = H_0 H_1 ... H_{n-2};  T = Q^T M Q has diagonal d and off-diagonal e[0 .. n-2].  That is
LAPACK's dsytrd(uplo='L') with the reflectors transposed into the rows."""

import numpy as np

LD = np.longdouble
EPS = 2.22e-16           # the eps of every bar in the GPU tests
DEVICE_EPS = 2.220446049250313e-16  # the constant in k_td_bounds


# ------------------------------------------------------------------------------ reflectors
def q_from_reflectors(reflectors, tau):
  """Q = H_0 ... H_{n-2}, accumulated in longdouble from the last reflector to the first (only
  the block [j+1:, j+1:] differs from the identity when H_j is applied), returned as float64."""
  n = len(tau)
  r = np.asarray(reflectors)
  q = np.eye(n, dtype=LD)
  for j in range(n - 2, -1, -1):
    if tau[j] == 0.0:
      continue
    v = r[j, j + 1:].astype(LD)
    blk = q[j + 1:, j + 1:]
    blk -= LD(tau[j]) * np.outer(v, v @ blk)
  return q.astype(np.float64)


def apply_q(reflectors, tau, z):
  """Q z for z (n, cols) in longdouble, last reflector first (k_td_backtransform's order)."""
  n = len(tau)
  r = np.asarray(reflectors)
  x = np.array(z, dtype=LD).reshape(n, -1)
  for j in range(n - 2, -1, -1):
    if tau[j] == 0.0:
      continue
    v = r[j, j + 1:].astype(LD)
    x[j + 1:] -= LD(tau[j]) * np.outer(v, v @ x[j + 1:])
  return x


def tridiag(d, e):
  """The dense T of diagonal d (n) and off-diagonal e[0 .. n-2] (a longer e is cut)."""
  d = np.asarray(d, dtype=np.float64)
  n = d.shape[0]
  e = np.asarray(e, dtype=np.float64)[:max(n - 1, 0)]
  return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def gershgorin_norm(d, e):
  """G = max_i (|d_i| + |e_{i-1}| + |e_i|)."""
  d = np.asarray(d, dtype=np.float64)
  n = d.shape[0]
  a = np.zeros(n + 1)
  a[1:n] = np.abs(np.asarray(e, dtype=np.float64)[:n - 1])
  return float(np.max(np.abs(d) + a[:n] + a[1:]))


# ------------------------------------------------------------------------------ multisection
def _sturm_count(d, e2, x, pivmin):
  """td_count for an array of shifts x: eigenvalues of T that are <= x.  1 / q is an IEEE
  division here, a reciprocal with two Newton steps on the device."""
  q = d[0] - x
  q = np.where(np.abs(q) < pivmin, -pivmin, q)
  count = (q <= 0.0).astype(np.int64)
  for i in range(1, d.shape[0]):
    q = (d[i] - x) - e2[i - 1] * (1.0 / q)
    q = np.where(np.abs(q) < pivmin, -pivmin, q)
    count += q <= 0.0
  return count


def sturm_multisection(d, e):
  """k_td_bounds + k_td_bisect: every eigenvalue of tridiag(d, e), DESCENDING.  The same
  Gershgorin bracket, pivmin and slack, the same four cut points per round (1/4, 3/8, the
  midpoint as bisection computes it, 3/4), 48 rounds, the same bracket updates."""
  d = np.asarray(d, dtype=np.float64)
  n = d.shape[0]
  e = np.asarray(e, dtype=np.float64)[:n - 1]
  with np.errstate(all="ignore"):
    a = np.zeros(n + 1)
    a[1:n] = np.abs(e)
    glo = np.min(d - a[:n] - a[1:])
    ghi = np.max(d + a[:n] + a[1:])
    e2 = e * e
    emax = np.max(e2) if n > 1 else 0.0
    tnorm = max(abs(glo), abs(ghi))
    pivmin = 1e-280 * max(1.0, emax)
    slack = 2.1 * tnorm * DEVICE_EPS * n + 2.1 * pivmin
    lo = np.full(n, glo - slack)
    hi = np.full(n, ghi + slack)
    kk = np.arange(n)
    for _ in range(48):
      w = hi - lo
      mid = 0.5 * (lo + hi)
      stuck = ~((mid > lo) & (mid < hi))
      if np.all(stuck):
        break
      xs = np.stack([lo + w * 0.25, mid, lo + w * 0.75, lo + w * 0.375])
      cs = _sturm_count(d, e2, xs, pivmin)
      nlo, nhi = lo.copy(), hi.copy()
      for q in range(4):
        left = cs[q] < kk + 1   # eigenvalue kk lies right of this cut
        nlo = np.where(left & (xs[q] > nlo), xs[q], nlo)
        nhi = np.where(~left & (xs[q] < nhi), xs[q], nhi)
      lo = np.where(stuck, lo, nlo)
      hi = np.where(stuck, hi, nhi)
    return (0.5 * (lo + hi))[::-1].copy()


# ------------------------------------------------------------------------------ matrices (A)
def gaussian_sym(n, seed):
  rng = np.random.default_rng(seed)
  a = rng.standard_normal((n, n))
  return 0.5 * (a + a.T)


def block_sizes(n):
  """Blocks of 70, 80, 90, 60 rows at n = 300, scaled to n (the last takes the remainder)."""
  s = [n * k // 300 for k in (70, 80, 90)]
  return s + [n - sum(s)]


def block_diagonal(n, seed):
  m = np.zeros((n, n))
  r0 = 0
  for i, s in enumerate(block_sizes(n)):
    m[r0:r0 + s, r0:r0 + s] = gaussian_sym(s, seed + i)
    r0 += s
  return m


def toeplitz(n):
  return 2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)


def with_spectrum(lam, seed):
  """Q diag(lam) Q^T for a random orthogonal Q, exactly symmetric."""
  rng = np.random.default_rng(seed)
  n = len(lam)
  q, _ = np.linalg.qr(rng.standard_normal((n, n)))
  m = (q * np.asarray(lam, dtype=np.float64)) @ q.T
  return 0.5 * (m + m.T)


STRUCTURES = ("diagonal", "tridiagonal", "block_diagonal", "rank3", "graded", "zero_border",
              "scaled", "tiny", "huge")
STRUCTURE_SIZES = (161, 300)


def structure(name, n):
  """-> (m, c, p): the input of sc_stage_tridiag (c, p None: Op = m)."""
  rng = np.random.default_rng(1000 + n)
  if name == "diagonal":
    return np.diag(rng.standard_normal(n)), None, None
  if name == "tridiagonal":
    return toeplitz(n), None, None
  if name == "block_diagonal":
    return block_diagonal(n, 7), None, None
  if name == "rank3":
    b = rng.standard_normal((n, 3))
    return b @ b.T, None, None
  if name == "graded":
    return with_spectrum(np.logspace(-12, 0, n), 2), None, None
  if name == "zero_border":
    m = gaussian_sym(n, 3)
    m[:40, :] = 0.0
    m[:, :40] = 0.0
    return m, None, None
  if name == "scaled":
    return gaussian_sym(n, 4), 10.0 ** rng.uniform(-3, 3, n), rng.standard_normal(n)
  if name == "tiny":
    return gaussian_sym(n, 5) * 1e-150, None, None
  if name == "huge":
    return gaussian_sym(n, 6) * 1e150, None, None
  raise KeyError(name)


def materialized(m, c, p):
  """diag(p) + diag(c) m diag(c) with k_td_materialize's roundings: (c_i c_j) first."""
  if c is None and p is None:
    return m
  n = m.shape[0]
  c = np.ones(n) if c is None else c
  p = np.zeros(n) if p is None else p
  op = np.outer(c, c) * m
  op[np.arange(n), np.arange(n)] += p
  return op


# ------------------------------------------------------------------------------ tridiagonals (B)
def wilkinson(n):
  h = (n - 1) // 2
  return np.abs(np.arange(n) - h).astype(np.float64), np.ones(n - 1)


def glued_wilkinson(blocks, glue, size=21):
  d1, e1 = wilkinson(size)
  d = np.tile(d1, blocks)
  e = np.concatenate([np.concatenate([e1, [glue]]) for _ in range(blocks)])[:-1]
  return d, e


def toeplitz_eigenvalues(n):
  return 2 - 2 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1))


RANDOM_SIZES = (1, 2, 3, 8, 9, 10, 15, 16, 17, 129, 1000)


def tridiagonal_cases():
  """name -> (d (n), e (n - 1)): the inputs of sc_stage_tridiag_values."""
  cases = {}
  for n in RANDOM_SIZES:
    rng = np.random.default_rng(n)
    cases["random%d" % n] = (rng.standard_normal(n), rng.standard_normal(n - 1))
  cases["wilkinson21"] = wilkinson(21)
  cases["wilkinson101"] = wilkinson(101)
  cases["glued_1e-14"] = glued_wilkinson(10, 1e-14)
  cases["glued_0"] = glued_wilkinson(10, 0.0)
  cases["toeplitz300"] = (np.full(300, 2.0), np.full(299, -1.0))
  cases["3I"] = (np.full(50, 3.0), np.zeros(49))
  cases["zeros"] = (np.zeros(50), np.zeros(49))
  rng = np.random.default_rng(77)
  g = np.logspace(-12, 0, 100)
  cases["graded"] = (g, 0.3 * np.sqrt(g[:-1] * g[1:]) * rng.choice([-1.0, 1.0], 99))
  cases["tiny_e"] = (rng.standard_normal(100), 1e-170 * rng.standard_normal(99))
  for name, scale in (("scale_1e+100", 1e100), ("scale_1e-100", 1e-100)):
    cases[name] = (scale * rng.standard_normal(100), scale * rng.standard_normal(99))
  cases["negative_definite257"] = (-(2.5 + rng.uniform(0, 1, 257)), rng.uniform(-1, 1, 256))
  k = np.arange(1, 200)
  cases["clement200"] = (np.zeros(200), np.sqrt(k * (200.0 - k)))
  cases["golub_kahan64"] = (np.zeros(64), np.ones(63))
  return cases


# ------------------------------------------------------------------------------ spectra (D)
def four_component_laplacian(n, seed):
  """The normalised Laplacian I - D^-1/2 W D^-1/2 of a graph with four connected components
  (dense positive weights inside a component, none between): a null space of dimension 4."""
  rng = np.random.default_rng(seed)
  w = np.zeros((n, n))
  r0 = 0
  for s in block_sizes(n):
    b = rng.uniform(0.1, 1.0, (s, s))
    w[r0:r0 + s, r0:r0 + s] = 0.5 * (b + b.T)
    r0 += s
  dis = 1.0 / np.sqrt(w.sum(axis=1))
  lap = np.eye(n) - dis[:, None] * w * dis[None, :]
  return 0.5 * (lap + lap.T)


SPECTRA = ("multiplicity20", "multiplicity70", "cluster30_1e-9", "cluster80_1e-4", "bulk_1e-3",
           "rank3_negated", "3I", "diagonal_tenfold", "laplacian4")
SPECTRA_SIZES = (300, 161)
SPECTRA_COUNT = 80


def spectrum_case(name, n):
  """-> (m, descend): the input of sc_stage_sym_eig with 80 vectors."""
  rng = np.random.default_rng(2000 + n)
  rest = lambda k: rng.uniform(-0.5, 0.5, k)
  if name == "multiplicity20":
    return with_spectrum(np.concatenate([np.full(20, 2.0), np.linspace(1.5, 1.0, 60),
                                         rest(n - 80)]), 11), True
  if name == "multiplicity70":
    return with_spectrum(np.concatenate([np.full(70, 2.0), np.linspace(1.5, 1.0, 10),
                                         rest(n - 80)]), 12), True
  if name == "cluster30_1e-9":
    return with_spectrum(np.concatenate([2.0 - 1e-9 * np.arange(30), np.linspace(1.5, 1.0, 50),
                                         rest(n - 80)]), 13), True
  if name == "cluster80_1e-4":
    return with_spectrum(np.concatenate([2.0 - 1e-4 * np.arange(80), rest(n - 80)]), 14), True
  if name == "bulk_1e-3":
    return with_spectrum(1.0 + 1e-3 * rng.uniform(0, 1, n), 15), True
  if name == "rank3_negated":
    b = rng.standard_normal((n, 3))
    return -(b @ b.T), False
  if name == "3I":
    return 3.0 * np.eye(n), True
  if name == "diagonal_tenfold":
    return np.diag(rng.permutation(np.repeat(rng.standard_normal((n + 9) // 10), 10)[:n])), True
  if name == "laplacian4":
    return four_component_laplacian(n, 16), False
  raise KeyError(name)
