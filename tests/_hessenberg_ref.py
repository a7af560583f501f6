"""References for the kernels of the general (non-symmetric) eigen path, in plain NumPy: the
Householder reduction of csrc/hessenberg.hip (LAPACK dgehd2's storage, Q accumulated in
`longdouble` from the packed reflectors, the two figures a reduction is judged by), the
Rayleigh-Ritz kernels of csrc/eig_general.hip (k_gen_ritz, k_gen_residual, k_gen_phase,
k_gen_gather: `longdouble` evaluation, a-priori bounds, NumPy fp64 restatements) and the inputs
of tests/test_gpu_general_kernels.py.

Shared by tests/test_hessenberg_reference_host.py (CPU: the figures against
scipy.linalg.hessenberg, the fp64 restatements inside every bound with room to spare -- so the
bounds are those of an honest fp64 implementation, not fitted to the device), tests/test_host_logic.py
(gehd2 feeds the host half of the dense general route) and the GPU tests.

Storage (dgehd2): step k = 0 .. n-3 applies P_k = I - tau_k v_k v_k^T from both sides, v_k on
rows k+1 .. n-1 with v_k[k+1] = 1 implied; v_k[k+2 ..] is kept below the subdiagonal of column
k.  Q = P_0 P_1 ... P_{n-3} and H = Q^T M Q is upper Hessenberg."""

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
EPS = 2.22e-16           # the eps of every bar in the GPU tests
U = 2.0 ** -53
B = 8                    # kEigBlock: columns of a restart block


def gamma(k):
  """gamma_k = k u / (1 - k u): a length-k fp64 sum of products, in any order, errs by at most
  gamma_k times the same sum of absolute values."""
  return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------ the reduction
def gehd2(a):
  """LAPACK dgehd2 in NumPy, in the storage the device reduction (hessenberg.hip) leaves: the
  Hessenberg matrix on and above the subdiagonal, reflector k (v[k + 1] = 1 implied) below the
  subdiagonal of column k, tau."""
  a = a.copy()
  n = a.shape[0]
  tau = np.zeros(max(n - 2, 1))
  for k in range(n - 2):
    x = a[k + 1:, k].copy()
    alpha, xnorm = x[0], np.linalg.norm(x[1:])
    if xnorm == 0.0:
      continue
    beta = -np.copysign(np.hypot(alpha, xnorm), alpha)
    tau[k] = (beta - alpha) / beta
    v = x / (alpha - beta)
    v[0] = 1.0
    a[:, k + 1:] -= tau[k] * np.outer(a[:, k + 1:] @ v, v)
    a[k + 1:, k + 1:] -= tau[k] * np.outer(v, v @ a[k + 1:, k + 1:])
    a[k + 1, k] = beta
    a[k + 2:, k] = v[1:]
  return np.ascontiguousarray(a), tau


def q_from_packed(packed, tau):
  """Q = P_0 ... P_{n-3}, accumulated in longdouble from the last reflector to the first (only
  the block [k+1:, k+1:] differs from the identity when P_k is applied), returned as float64."""
  r = np.asarray(packed)
  n = r.shape[0]
  q = np.eye(n, dtype=LD)
  for k in range(min(n - 3, len(tau) - 1), -1, -1):
    if tau[k] == 0.0:
      continue
    v = np.concatenate([[1.0], r[k + 2:, k]]).astype(LD)
    blk = q[k + 1:, k + 1:]
    blk -= LD(tau[k]) * np.outer(v, v @ blk)
  return q.astype(np.float64)


def hessenberg_part(packed):
  """The returned matrix with everything below the subdiagonal set to zero."""
  return np.triu(np.asarray(packed), -1)


def power_of_two_below(x):
  """2^e with 2^e <= x < 2^(e+1), x > 0."""
  return float(np.ldexp(1.0, int(np.frexp(x)[1]) - 1))


def reduction_figures(m, q, hm, scale=1.0):
  """(i) max|Q^T Q - I| and (ii) max|Q^T M Q - H scale| / ||M||_2, in fp64 products -- the same
  function for the device's factors and LAPACK's.  M and H are first brought to max|m| in
  [1, 2) by an exact power of two (both figures are invariant; nothing over- or underflows at
  1e+-160)."""
  m = np.asarray(m, dtype=np.float64)
  n = m.shape[0]
  amax = float(np.abs(m).max())
  if amax > 0.0:
    f = power_of_two_below(amax)
    m = m / f
    hm = hm * (scale / f)
  else:
    hm = hm * scale
  orth = float(np.abs(q.T @ q - np.eye(n)).max())
  norm = float(np.linalg.norm(m, 2))
  res = float(np.abs(q.T @ m @ q - hm).max())
  return orth, (res / norm if norm > 0.0 else res)


# ------------------------------------------------------------------------------ matrices
GAUSSIAN_SIZES = (1, 2, 3, 4, 5, 33, 34, 35, 64, 65, 66, 67, 129, 257, 258, 259, 300, 512, 545)
STRUCTURES = ("hessenberg", "triangular", "diagonal", "block_diagonal", "rank_one", "graded_rows",
              "zero_border", "affinity", "random_walk")
STRUCTURE_SIZES = (67, 300)
SCALINGS = ("2^+399", "2^-399", "2^+401", "2^-401", "1e-170", "1e+160")


def gaussian(n, seed=None):
  return np.random.default_rng(5000 + n if seed is None else seed).standard_normal((n, n))


def unit_gaussian(n, seed=None):
  """Gaussian times an exact power of two that brings max|a| into [0.5, 1): what the driver's
  frexp exponent counts from, so that `unit_gaussian * 2^k` has exponent exactly k."""
  g = gaussian(n, seed)
  return g / (2.0 * power_of_two_below(float(np.abs(g).max())))


def block_sizes(n):
  """Blocks of 70, 80, 90, 60 rows at n = 300, scaled to n (the last takes the remainder)."""
  s = [n * k // 300 for k in (70, 80, 90)]
  return s + [n - sum(s)]


def thresholded_affinity(n):
  """so.row_wise_threshold(so.affinity(blobs)): [RowWiseThreshold] alone, the sequence that
  does not end symmetrisable -- non-negative, sparse in magnitude, not symmetric."""
  import spectral_oracle as so
  x = so.blobs(n, 24, 5, seed=n)
  return np.ascontiguousarray(so.row_wise_threshold(
      so.affinity(x), p_percentile=0.9, threshold_type=so.THRESHOLD_PERCENTILE))


def structure(name, n):
  rng = np.random.default_rng(3000 + n)
  if name == "hessenberg":
    return np.triu(rng.standard_normal((n, n)), -1)
  if name == "triangular":
    return np.triu(rng.standard_normal((n, n)))
  if name == "diagonal":
    return np.diag(rng.standard_normal(n))
  if name == "block_diagonal":
    m = np.zeros((n, n))
    r0 = 0
    for s in block_sizes(n):
      m[r0:r0 + s, r0:r0 + s] = rng.standard_normal((s, s))
      r0 += s
    return m
  if name == "rank_one":
    return np.outer(rng.standard_normal(n), rng.standard_normal(n))
  if name == "graded_rows":
    return np.logspace(-12, 0, n)[:, None] * rng.standard_normal((n, n))
  if name == "zero_border":
    m = rng.standard_normal((n, n))
    m[:40, :] = 0.0
    m[:, :40] = 0.0
    return m
  if name == "affinity":
    return thresholded_affinity(n)
  if name == "random_walk":
    import spectral_oracle as so
    return np.ascontiguousarray(so.laplacian(thresholded_affinity(n), so.LAPLACIAN_RANDOM_WALK))
  raise KeyError(name)


def scaled(name, n):
  """-> (matrix, rescaled): is the driver expected to rescale it (max|a| beyond 2^+-400)?"""
  if name.startswith("2^"):
    k = int(name[2:])
    return np.ldexp(unit_gaussian(n), k), abs(k) > 400
  return gaussian(n) * float(name), True


def tiny_column(n):
  """max|a| ~ 1 and a first column whose part below the subdiagonal is ~1e-170: its squares
  underflow to zero, so hess_reflector sees nothing to annihilate there.  (Only the first column
  can stay that small: every later one is mixed with its O(1) rows by the left updates.)"""
  m = gaussian(n, 77)
  m[2:, 0] *= 1e-170
  return m


# ------------------------------------------------------------------------------ Ritz kernels
# k_gen_ritz:  V[i, c] = sum_j Q[i, j] Y[j, c], j ascending, no FMA (real and imaginary part
# separately).  A length-m sum of products: |got - exact| <= gamma_m (|Q| |Y|) per entry.
def ritz_exact(q, yre, yim):
  y = yre.astype(CLD) + 1j * yim.astype(CLD)
  return y if q is None else q.astype(LD) @ y


def ritz_bound(q, yre, yim):
  """Per entry, on the modulus of the complex error."""
  if q is None:
    return np.zeros(yre.shape)  # the identity form copies
  return gamma(q.shape[1]) * (np.abs(q) @ np.hypot(yre, yim))


def ritz_fp64(q, yre, yim):
  """The kernel's own loop in fp64: one product and one addition per term, j ascending."""
  vr = np.zeros((q.shape[0], yre.shape[1]))
  vi = np.zeros_like(vr)
  for j in range(q.shape[1]):
    vr = vr + q[:, j:j + 1] * yre[j:j + 1]
    vi = vi + q[:, j:j + 1] * yim[j:j + 1]
  return vr, vi


# k_gen_residual + k_gen_residual_reduce:  r = OpQ y - theta Q y (complex), resid = ||r||_2.
# Each of the four length-m sums errs by gamma_m of its absolute sum; the complex product
# theta (Q y) keeps the modulus of the error of Q y and adds (sqrt 2 + 1) u |theta| |Q y| for its
# four products and two inner additions, so with
#   delta_i = gamma_{m+4} ((|OpQ| |y|)_i + |theta| (|Q| |y|)_i)
# the computed r_i is within delta_i + u |r_i| of the exact one (the last subtraction).  The
# squares, their fixed-order sum over the n rows and the square root are relative to the
# computed norm: gamma_{n+2} covers them.  Hence
#   | resid - ||r||_2 |  <=  ||delta||_2 + gamma_{n+2} ||r||_2,
# absolute on purpose: the residual of a converged pair is all cancellation.
def residual_exact(q, opq, yre, yim, tre, tim):
  y = yre.astype(CLD) + 1j * yim.astype(CLD)
  theta = tre.astype(CLD) + 1j * tim.astype(CLD)
  r = opq.astype(LD) @ y - (q.astype(LD) @ y) * theta[None, :]
  return np.sqrt(np.sum(r.real ** 2 + r.imag ** 2, axis=0))


def residual_bound(q, opq, yre, yim, tre, tim):
  n, m = q.shape
  ay = np.hypot(yre, yim)
  delta = gamma(m + 4) * (np.abs(opq) @ ay + np.hypot(tre, tim)[None, :] * (np.abs(q) @ ay))
  exact = residual_exact(q, opq, yre, yim, tre, tim).astype(np.float64)
  return np.linalg.norm(delta, axis=0) + gamma(n + 2) * exact


def residual_fp64(q, opq, yre, yim, tre, tim):
  """The kernels' own order in fp64: sums over j ascending, |r|^2 over the 8 rows of a block,
  then block after block."""
  n, m = q.shape
  qr, qi = ritz_fp64(q, yre, yim)
  orr, oi = ritz_fp64(opq, yre, yim)
  rre = orr - (tre[None, :] * qr - tim[None, :] * qi)
  rim = oi - (tre[None, :] * qi + tim[None, :] * qr)
  acc = rre * rre + rim * rim
  total = np.zeros(yre.shape[1])
  for r0 in range(0, n, 8):
    part = np.zeros(yre.shape[1])
    for r in range(r0, min(r0 + 8, n)):
      part = part + acc[r]
    total = total + part
  return np.sqrt(total)


# k_gen_phase:  v <- v conj(v_p) / (|v_p| ||v||_2), p the first index of largest |v_i|^2.
#   ||v||^2: n terms of three roundings each, 256 partial sums of ceil(n / 256) terms and an
#   8-level tree -- relative error gamma_{ceil(n/256)+8+3}, halved by the square root (+1 u), the
#   reciprocal +1 u;  a = vr inv, b = vi inv: 1 u;  the unit factor (cr, ci) = conj(v_p) / |v_p|:
#   |v_p| 2.5 u, the divisions 1 u;  the complex product (sqrt 2 + 1) u as above.
# On the modulus of every entry's complex error, relative to the entry:
def phase_terms(n):
  return 0.5 * (-(-n // 256) + 11) + 9.0


def phase_bound(n, exact):
  return phase_terms(n) * U / (1.0 - phase_terms(n) * U) * np.abs(exact)


def phase_pivot(vre, vim):
  """First index of largest |v_i|^2 per column, with the squares in longdouble."""
  mag = vre.astype(LD) ** 2 + vim.astype(LD) ** 2
  return np.argmax(mag, axis=0)


def phase_pivot_gap(vre, vim):
  """Per column: (largest |v|^2 - largest |v|^2 among the entries that are not bit-equal in
  magnitude to the pivot) / largest.  Exact ties are resolved by index, near ties by rounding:
  the tests keep this at 1e-6 or more."""
  mag = vre.astype(LD) ** 2 + vim.astype(LD) ** 2
  top = mag.max(axis=0)
  rest = np.where(mag == top[None, :], -np.inf, mag).max(axis=0)
  return np.where(top > 0, (top - rest) / np.where(top > 0, top, 1), 1.0).astype(np.float64)


def phase_exact(vre, vim):
  v = vre.astype(CLD) + 1j * vim.astype(CLD)
  p = phase_pivot(vre, vim)
  vp = v[p, np.arange(v.shape[1])]
  norm = np.sqrt(np.sum(v.real ** 2 + v.imag ** 2, axis=0))
  return v * (np.conj(vp) / (np.abs(vp) * norm))[None, :]


def phase_fp64(vre, vim):
  """The kernel in fp64: strided partial sums, tree, the same scalar steps."""
  n, cols = vre.shape
  out_r, out_i = np.empty_like(vre), np.empty_like(vim)
  for c in range(cols):
    vr, vi = vre[:, c], vim[:, c]
    mag = vr * vr + vi * vi
    part = np.zeros(256)
    for r0 in range(0, n, 256):
      seg = mag[r0:r0 + 256]
      part[:len(seg)] = part[:len(seg)] + seg
    o = 128
    while o > 0:
      part[:o] = part[:o] + part[o:2 * o]
      o //= 2
    k = int(np.argmax(mag))
    inv = 1.0 / np.sqrt(part[0])
    pm = np.sqrt(vr[k] * vr[k] + vi[k] * vi[k])
    cr, ci = vr[k] / pm, -vi[k] / pm
    a, b = vr * inv, vi * inv
    out_r[:, c] = a * cr - b * ci
    out_i[:, c] = a * ci + b * cr
  return out_r, out_i


# k_gen_gather's noise column j of a block with `seed`: element e = row * 8 + j
def gather_noise(n, j, seed):
  with np.errstate(over="ignore"):
    e = np.arange(n, dtype=np.uint64) * np.uint64(B) + np.uint64(j)
    x = np.uint64(seed) ^ (np.uint64(0x9E3779B97F4A7C15) * (e + np.uint64(1)))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x = x ^ (x >> np.uint64(31))
  return (x >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0


# ------------------------------------------------------------------------------ Ritz inputs
RITZ_M = (8, 24, 64, 128)
RITZ_COLS = (1, 31, 32, 33, 64)
RITZ_N = (65, 129, 263)
RITZ_KINDS = ("gaussian", "converged", "decades")


def ritz_shapes():
  return [(n, m, cols) for m in RITZ_M for cols in RITZ_COLS if cols <= m for n in RITZ_N]


def ritz_case(kind, n, m, cols):
  """-> q, opq (n, m), yre, yim (m, cols), theta_re, theta_im (cols).
  gaussian   Q orthonormal (Gaussian where m > n), OpQ = Op Q for a Gaussian Op, (theta, Y) the `cols` eigenpairs of
             Q^T Op Q of largest real part (np.linalg.eig: complex pairs occur)
  converged  Q and H of small integers, OpQ := Q H exactly, (theta, Y) eigenpairs of H: every
             residual is rounding of the pair itself, ~1e-13
  decades    all six arrays dense, magnitudes 10^U(-3, 3) with random signs"""
  rng = np.random.default_rng(100000 * RITZ_KINDS.index(kind) + 1000 * m + 10 * cols + n)
  if kind == "decades":
    d = lambda *s: rng.choice([-1.0, 1.0], s) * 10.0 ** rng.uniform(-3.0, 3.0, s)
    return d(n, m), d(n, m), d(m, cols), d(m, cols), d(cols), d(cols)
  if kind == "gaussian":
    q = rng.standard_normal((n, m))
    q = np.linalg.qr(q)[0] if m <= n else q / np.sqrt(n)  # (m > n: no solve, still the kernels)
    opq = rng.standard_normal((n, n)) @ q
    hm = q.T @ opq
  else:
    q = rng.integers(-3, 4, (n, m)).astype(np.float64)
    hm = rng.integers(-4, 5, (m, m)).astype(np.float64)
    opq = q @ hm  # exact: integers below 2^53
  w, y = np.linalg.eig(hm)
  order = np.argsort(-w.real, kind="stable")[:cols]
  w, y = w[order], y[:, order]
  c = np.ascontiguousarray
  return c(q), c(opq), c(y.real), c(y.imag), c(w.real), c(w.imag)


def tie_column(n, first, second, seed):
  """A complex column of length n whose largest magnitude, 1/sqrt(2) = |+-0.5 +- 0.5i|, is taken
  at exactly `first` and `second` (different sign patterns); every other entry has modulus at
  most 0.5.  Exactly representable squares: no rounding can break or make the tie."""
  rng = np.random.default_rng(seed)
  vr = rng.uniform(-0.35, 0.35, n)
  vi = rng.uniform(-0.35, 0.35, n)
  vr[first], vi[first] = -0.5, 0.5
  vr[second], vi[second] = 0.5, 0.5
  return vr, vi
