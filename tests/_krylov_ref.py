"""The block Lanczos chain of csrc/eig.hip restated in NumPy fp64, the a-priori bounds its
kernels are held to, and `longdouble` evaluators of the quantities the bounds are about; and the
same for the block Arnoldi chain of the general path (ArnoldiChain, ArnoldiInvariants: separate
left and right scalings, a full non-symmetric H, the same CGS-2 + CholQR-2 steps and start block
generator; used by test_gpu_general_kernels.py).

Shared by tests/test_krylov_reference_host.py (CPU: the restated chain itself stays within
every bound with a factor 8 to spare, so the bounds are honest) and by the GPU tests
test_gpu_block_operator.py / test_gpu_krylov_invariants.py (the device kernels against the same
bounds; the reference chain's own figures are the additive terms the bounds cannot derive).

The chain, from the comments of eig.hip (k_lz_rows) and eig_driver.hip (sym_topk):

  start block   W = hash_uniform(seed) | Gram | CholQR | CholQR, store Q[:, 0:8]
                (links pre 0 > 4, 4 > 3, 3 > store)
  block step    W = Op Q[:, m-8:m]  (Vs = c .* V is rounded once, as the store link leaves it)
    link 0 > 1  sums of Q[:, 0:m]^T W
    link 1 > 2  H1 = Q^T W: T[0:m, m-8:m] = H1 (mirrored);  W -= Q H1            (CGS 1)
    link 2 > 3  H2 = Q^T W: T += H2;  G' = W^T W - H2^T H2 (Pythagoras), kept as the residual
                Gram;  W = (W - Q H2) chol(G')^-1                               (CGS 2 + CholQR)
    link 3 > st H3 = Q^T W, G'' = W^T W - H3^T H3;  W = (W - Q H3) chol(G'')^-1, stored as
                Q[:, m:m+8]                                         (re-projection + CholQR)
  thick restart (basis at its cap): Q <- [Q[:, 0:m] Y[:, 0:keep] | Q[:, m:m+8]], T <- diag(theta)

Sums over rows run sequentially over blocks of 64 rows, the K sum of the operator over chunks
of 32 columns (not NumPy's pairwise order over the whole length): the figures below are those of
an honest fp64 implementation in a bad order, not of a lucky one."""

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
B = 8                    # vectors per block (kEigBlock)
BASIS_CAP = 128          # kEigBasisCap
SEED = 0x5EED5EED        # sym_topk's start block


def gamma(k):
  """gamma_k = k u / (1 - k u): a length-k fp64 sum of products, in any order, with or without
  FMA, errs by at most gamma_k times the same sum of absolute values."""
  return k * U / (1.0 - k * U)


def basis_cap(n):
  """sym_topk: LDS Jacobi limit, and basis + next block must fit in R^n."""
  return min(BASIS_CAP, ((n - B) // B) * B)


# ------------------------------------------------------------------------------ start block
def _splitmix64(x):
  x = x + np.uint64(0x9E3779B97F4A7C15)
  x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
  x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
  return x ^ (x >> np.uint64(31))


def start_block(n, seed=SEED):
  """k_lz_rows with init_random: W[r, j] = hash_uniform(seed, r * 8 + j), exact in fp64."""
  with np.errstate(over="ignore"):
    idx = np.arange(n * B, dtype=np.uint64)
    h = _splitmix64(np.uint64(seed) ^ _splitmix64(idx))
  return ((h >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0).reshape(n, B)


# ------------------------------------------------------------------------------ the operator
def _chunked_product(a, x, chunk):
  """sum over k-chunks of a[:, chunk] @ x[chunk], accumulated chunk after chunk."""
  acc = np.zeros((a.shape[0], x.shape[1]), dtype=np.result_type(a, x))
  for k0 in range(0, a.shape[1], chunk):
    acc = acc + a[:, k0:k0 + chunk] @ x[k0:k0 + chunk]
  return acc


class Operator:
  """W = p .* V + c .* (M (s .* V))  or, with `two`, p .* V + c .* (M (M (s .* V))).
  c, p, s: n-vectors or None (1 / 0 / same as c).  M need not be symmetric."""

  def __init__(self, m, c=None, p=None, s=None, two=False):
    self.m = np.ascontiguousarray(m, dtype=np.float64)
    self.n = self.m.shape[0]
    self.c = None if c is None else np.asarray(c, dtype=np.float64)
    self.p = None if p is None else np.asarray(p, dtype=np.float64)
    self.s = self.c if s is None else np.asarray(s, dtype=np.float64)
    self.two = bool(two)
    self._m_ld = None
    self._m_abs = None

  def _vec(self, v, fill, dtype):
    return (np.full(self.n, fill, dtype=dtype) if v is None else v.astype(dtype))[:, None]

  def apply(self, v):
    """fp64, K summed in chunks of 32 columns; Vs rounded once."""
    y = self._vec(self.s, 1.0, np.float64) * v
    for _ in range(2 if self.two else 1):
      y = _chunked_product(self.m, y, 32)
    w = self._vec(self.c, 1.0, np.float64) * y
    return w if self.p is None else w + self.p[:, None] * v

  def apply_ld(self, v):
    """The same in longdouble from the fp64 inputs (nothing rounded to fp64 on the way)."""
    if self._m_ld is None:
      self._m_ld = self.m.astype(LD)
    y = self._vec(self.s, 1.0, LD) * v.astype(LD)
    for _ in range(2 if self.two else 1):
      y = self._m_ld @ y
    return self._vec(self.p, 0.0, LD) * v.astype(LD) + self._vec(self.c, 1.0, LD) * y

  def apply_abs(self, v):
    """|p| .* |V| + |c| .* (|M| (|s| .* |V|))  (twice |M| for the two-product form)."""
    if self._m_abs is None:
      self._m_abs = np.abs(self.m)
    y = np.abs(self._vec(self.s, 1.0, np.float64) * v)
    for _ in range(2 if self.two else 1):
      y = self._m_abs @ y
    return np.abs(self._vec(self.p, 0.0, np.float64) * v) + np.abs(self._vec(self.c, 1.0, np.float64)) * y

  def terms(self):
    """Length of the accumulated sums + the roundings of the scalings: gamma's index."""
    return 2 * self.n + 6 if self.two else self.n + 4

  def bound(self, v):
    """Elementwise bound on |W - W_exact| for a correctly rounded kernel in any summation order."""
    return gamma(self.terms()) * self.apply_abs(v)


# ------------------------------------------------------------------------------ the chain
def _rows_product(x, y, chunk=64):
  """x^T y, summed over blocks of 64 rows one after the other."""
  acc = np.zeros((x.shape[1], y.shape[1]))
  for r0 in range(0, x.shape[0], chunk):
    acc = acc + x[r0:r0 + chunk].T @ y[r0:r0 + chunk]
  return acc


def _chol_inverse(g):
  """Rc = chol(G)^-1 (upper): the block times Rc has Gram I."""
  r = np.linalg.cholesky(g).T
  return np.linalg.solve(r, np.eye(B))


class Chain:
  """State of the restated chain: q (n, m + 8) basis with the next block, t (m, m)."""

  def __init__(self, op, seed=SEED):
    self.op = op
    self.n = op.n
    self.cap = basis_cap(self.n)
    ldq = BASIS_CAP + B
    self.q = np.zeros((self.n, ldq))
    self.t = np.zeros((ldq, ldq))
    self.g = np.zeros((B, B))
    self.m = 0
    self.cycles = 0
    w = start_block(self.n, seed)
    w = w @ _chol_inverse(_rows_product(w, w))
    w = w @ _chol_inverse(_rows_product(w, w))
    self.q[:, 0:B] = w

  def step(self):
    m = self.m + B                       # basis including the block the operator is applied to
    q = self.q[:, :m]
    w = self.op.apply(self.q[:, m - B:m])
    h1 = _rows_product(q, w)
    w = w - q @ h1
    h2 = _rows_product(q, w)
    t = h1 + h2
    self.g = _rows_product(w, w) - h2.T @ h2
    w = (w - q @ h2) @ _chol_inverse(self.g)
    h3 = _rows_product(q, w)
    w = (w - q @ h3) @ _chol_inverse(_rows_product(w, w) - h3.T @ h3)
    # T[0:m, m-8:m] and its mirror; the diagonal block from its upper triangle (lz_rows_body
    # writes entries i <= j and mirrors them)
    d = t[m - B:m]
    t[m - B:m] = np.triu(d) + np.triu(d, 1).T
    self.t[:m, m - B:m] = t
    self.t[m - B:m, :m] = t.T
    self.q[:, m:m + B] = w
    self.m = m

  def ritz(self):
    """Rayleigh-Ritz on T[0:m, 0:m]: theta descending, Y, the residual estimates of the driver
    (sqrt(y_last^T G y_last), host_rayleigh_ritz)."""
    m = self.m
    theta, y = np.linalg.eigh(self.t[:m, :m])
    theta, y = theta[::-1], y[:, ::-1]
    yl = y[m - B:m]
    resid = np.sqrt(np.maximum(np.einsum("pi,pq,qi->i", yl, self.g, yl), 0.0))
    return theta, y, resid

  def restart(self, keep):
    m = self.m
    theta, y, _ = self.ritz()
    q2 = np.zeros_like(self.q)
    q2[:, :keep] = self.q[:, :m] @ y[:, :keep]
    q2[:, keep:keep + B] = self.q[:, m:m + B]
    self.q = q2
    self.t[:] = 0.0
    self.t[np.arange(keep), np.arange(keep)] = theta[:keep]
    self.m = keep
    self.cycles += 1

  def run(self, m_final, cycles=0, keep=None):
    """Advance to a basis of m_final vectors in restart cycle `cycles` (restarts happen where
    the driver's do: when the next block would exceed the cap)."""
    while not (self.cycles == cycles and self.m == m_final):
      if self.m + B > self.cap:
        assert self.cycles < cycles and keep is not None, "m_final unreachable"
        self.restart(keep)
      self.step()
    return self

  def basis(self):
    return self.q[:, :self.m].copy(), self.t[:self.m, :self.m].copy()


def restart_keep(count, cap):
  """sym_topk's `keep` for a request of `count` pairs once the basis holds them."""
  keep = -(-(count + B) // B) * B
  return max(B, min(keep, cap - 2 * B))


# ------------------------------------------------------------------------------ invariants
class Invariants:
  """The measured quantities (longdouble) and their derived bounds for a basis Q (n, m) with
  projected matrix T (m, m) of the operator `op`."""

  def __init__(self, op, q, t):
    n, m = q.shape
    self.n, self.m = n, m
    ql = q.astype(LD)
    gram = ql.T @ ql
    self.orth = float(np.max(np.abs(gram - np.eye(m, dtype=LD))))
    self.orth_bound = 4.0 * gamma(n + m)
    opq = op.apply_ld(q)
    proj = ql.T @ opq
    tmax = float(np.max(np.abs(t)))
    self.slack = m * self.orth * tmax       # (I - Q^T Q) leaking into either check
    self.proj_err = np.abs(t.astype(LD) - proj).astype(np.float64)
    aq = np.abs(q)
    self.proj_bound = 2.0 * gamma(n + m + 8) * (aq.T @ op.apply_abs(aq)) + self.slack
    self.symmetric = bool(np.array_equal(t, t.T))
    # Krylov property: Op Q[:, 0:m-8] lies in span Q
    k = m - B
    self.krylov_err = np.abs(opq[:, :k] - ql @ proj[:, :k]).astype(np.float64)
    self.krylov_bound = op.bound(q[:, :k]) + self.slack   # + 16 x the reference's figure

  def proj_ratio(self, extra=0.0):
    return float(np.max(self.proj_err / np.maximum(self.proj_bound, extra)))

  def krylov_ratio(self, ref_figure, restarted=False):
    bound = self.krylov_bound + 16.0 * ref_figure
    if restarted:
      bound = np.maximum(self.krylov_bound, 16.0 * ref_figure)
    return float(np.max(self.krylov_err / bound))

  def figures(self):
    return {"orth": self.orth, "proj": float(np.max(self.proj_err)),
            "krylov": float(np.max(self.krylov_err))}


# ------------------------------------------------------------------------------ block Arnoldi
# The general path's chain (eig_driver.hip, gen_topk), a non-symmetric variant of the one above:
# the operator has separate left and right scalings, Op x = p .* x + cl .* (M (cr .* x))
# (Operator(m, c=cl, p=p, s=cr)); a block is orthogonalised by the host-driven links
# (orthonormalize: CGS twice, CholQR twice) and NOT recorded in T; the products Op Q are kept
# (Q2) and the projected matrix is formed explicitly and in full, H = Q^T (Op Q), at a check.
#   start block   W = hash_uniform(ARNOLDI_SEED) | CholQR | CholQR -> Q[:, 0:8]
#   block step    W = Op Q[:, m-8:m] (kept as OpQ[:, m-8:m]) | CGS | CGS | CholQR | CholQR
ARNOLDI_SEED = 0x9E3779B97F4A7C15
GEN_MAX = 64             # kGenMax: basis cap of the narrow form


def arnoldi_cap(n, wide=False):
  return min(BASIS_CAP if wide else GEN_MAX, ((n - B) // B) * B)


class ArnoldiChain:
  """State of the restated chain without restarts: q, opq (n, m), m a multiple of 8."""

  def __init__(self, op, seed=ARNOLDI_SEED):
    self.op = op
    self.n = op.n
    self.q = np.zeros((self.n, BASIS_CAP + B))
    self.opq = np.zeros((self.n, BASIS_CAP + B))
    self.m = 0
    self.seed = seed

  def step(self):
    m = self.m
    w = start_block(self.n, self.seed) if m == 0 else self.opq[:, m - B:m].copy()
    q = self.q[:, :m]
    if m > 0:
      for _ in range(2):
        w = w - q @ _rows_product(q, w)
    w = w @ _chol_inverse(_rows_product(w, w))
    w = w @ _chol_inverse(_rows_product(w, w))
    self.q[:, m:m + B] = w
    self.opq[:, m:m + B] = self.op.apply(w)
    self.m = m + B

  def run(self, m_final):
    while self.m < m_final:
      self.step()
    return self

  def state(self):
    """q, opq (n, m) and H = Q^T (Op Q), column block after column block."""
    m = self.m
    q, opq = self.q[:, :m].copy(), self.opq[:, :m].copy()
    return q, opq, _rows_product(q, opq)


class ArnoldiInvariants:
  """The measured quantities (longdouble) and their derived bounds for a basis Q (n, m), the
  stored products OpQ (n, m) and the projected matrix H (m, m) of the operator `op`:
    orthonormality   max |Q^T Q - I| <= 4 gamma_{n+m}                         (the Lanczos bar)
    operator         |OpQ - Op Q| <= gamma_{n+4} (|p||Q| + |cl| (|M| (|cr||Q|)))
    projection       |H - Q^T OpQ| <= 2 gamma_{n+m+8} |Q|^T |OpQ| + m orth max|H|
    Arnoldi property |(I - Q Q^T) Op Q[:, 0:m-8]| <= operator bound + m orth max|H|
                     (+ 16 x the reference chain's figure, + 1e-12 m max|H| after a restart:
                     arnoldi_ratio)"""

  def __init__(self, op, q, opq, h):
    n, m = q.shape
    self.n, self.m = n, m
    ql = q.astype(LD)
    self.orth = float(np.max(np.abs(ql.T @ ql - np.eye(m, dtype=LD))))
    self.orth_bound = 4.0 * gamma(n + m)
    exact = op.apply_ld(q)
    self.op_err = np.abs(opq.astype(LD) - exact).astype(np.float64)
    self.op_bound = op.bound(q)
    self.hmax = float(np.max(np.abs(h)))
    self.slack = m * self.orth * self.hmax
    self.proj_err = np.abs(h.astype(LD) - ql.T @ opq.astype(LD)).astype(np.float64)
    self.proj_bound = 2.0 * gamma(n + m + 8) * (np.abs(q).T @ np.abs(opq)) + self.slack
    k = m - B
    proj = ql.T @ exact
    self.arnoldi_err = np.abs(exact[:, :k] - ql @ proj[:, :k]).astype(np.float64)
    self.arnoldi_bound = self.op_bound[:, :k] + self.slack

  def op_ratio(self):
    return float(np.max(self.op_err / self.op_bound))

  def proj_ratio(self):
    return float(np.max(self.proj_err / self.proj_bound))

  def arnoldi_figure(self):
    return float(np.max(self.arnoldi_err)) if self.arnoldi_err.size else 0.0

  def arnoldi_ratio(self, ref_figure=0.0, restarted=False):
    if not self.arnoldi_err.size:
      return 0.0
    bound = self.arnoldi_bound + 16.0 * ref_figure
    if restarted:  # the kept Ritz vectors Q Y: Y from the host solver, held to 1e-12 m ||H||
      bound = bound + 1e-12 * self.m * self.hmax
    return float(np.max(self.arnoldi_err / bound))


def general_scaling_vectors(deg, laplacian_type):
  """k_scaling_general (eig_general.hip): cl, cr, p of Op = M (None / Affinity), -(D - M)
  (Unnormalized), -D'^-1 (D - M) (RandomWalk), -D'^-1/2 (D - M) D'^-1/2 (GraphCut)."""
  one, zero = np.ones_like(deg), np.zeros_like(deg)
  if laplacian_type in (0, 1):
    return one, one, zero
  if laplacian_type == 2:
    return one, one, -deg
  if laplacian_type == 3:
    g = 1.0 / (deg + 1e-10)
    return g, one, -(g * deg)
  if laplacian_type == 4:
    h = 1.0 / (np.sqrt(deg) + 1e-10)
    return h, h, -((h * deg) * h)
  raise ValueError("laplacian_type")


def separated_matrix(n):
  """Three eigenvalues near 5, 4, 3 over a non-symmetric bulk of radius 0.03: a block Krylov
  space of a few blocks holds them to 1e-10 -- a solve without a restart."""
  rng = np.random.default_rng(6000 + n)
  m = 0.03 * rng.standard_normal((n, n)) / np.sqrt(n)
  m[np.arange(3), np.arange(3)] += np.array([5.0, 4.0, 3.0])
  return m


def nonnormal_cluster(n, seed=0):
  """A non-normal matrix with a tight leading cluster: eigenvalues 2 - 1e-2 k (k < 12) over a
  bulk in the unit disc (2 x 2 rotation blocks: complex pairs), in a basis of condition ~30."""
  rng = np.random.default_rng(7000 + n + seed)
  d = np.zeros((n, n))
  k = 12
  d[np.arange(k), np.arange(k)] = 2.0 - 1e-2 * np.arange(k)
  for i in range(k, n - 1, 2):
    r, phi = rng.uniform(0.2, 0.95), rng.uniform(0.1, np.pi - 0.1)
    d[i:i + 2, i:i + 2] = r * np.array([[np.cos(phi), -np.sin(phi)], [np.sin(phi), np.cos(phi)]])
  if (n - k) % 2:
    d[n - 1, n - 1] = -0.5
  x, _ = np.linalg.qr(rng.standard_normal((n, n)))
  s = x * np.logspace(0, 1.5, n)[rng.permutation(n)]
  return np.ascontiguousarray(s @ d @ np.linalg.inv(s))


# ------------------------------------------------------------------------------ scaling vectors
def scaling_vectors(rowsum, laplacian_type):
  """scaling_vectors_body (rowops.hip) without RowWiseNormalize, in the dtype of rowsum:
  Op = diag(p) + diag(c) S diag(c) is S (None / Affinity), -(D - S) (Unnormalized) or
  -D^-1/2 (D - S) D^-1/2 with the reference's eps (GraphCut, laplacian.py:56-57)."""
  deg = rowsum
  one = deg.dtype.type(1.0)
  eps = deg.dtype.type(1e-10)
  if laplacian_type == 4:
    h = one / (np.sqrt(deg) + eps)
    return h, -((h * deg) * h)
  if laplacian_type == 2:
    return np.ones_like(deg), -deg
  if laplacian_type in (0, 1):
    return np.ones_like(deg), np.zeros_like(deg)
  raise ValueError("laplacian_type")


# ------------------------------------------------------------------------------ inputs
OPERATOR_SIZES = (129, 255, 256, 257, 383, 512, 640, 1153)
TWO_PRODUCT_SIZES = (257, 640, 1153)
GROUP_SIZES = (129, 0, 1153, 257, 512, 0, 383, 0, 256, 255, 0, 640, 0, 129, 0, 257)  # kGroupMax


def probe_matrix(n):
  """M[i, j] = M[j, i] = (4096 min(i, j) + max(i, j) + 1) 2^-24: exact, unique per pair."""
  i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
  return (4096.0 * np.minimum(i, j) + np.maximum(i, j) + 1.0) * 2.0 ** -24


def probe_columns(n):
  """Columns the position probes select: the fixed ones, every 8 q + 2 g (+1) slot of one
  interior 32-column chunk and of the last, ragged chunk."""
  cols = [0, 1, 7, 8, 31, 32, 33, 127, 128, 129, n - 2, n - 1]
  cols += list(range(64, 96))
  cols += list(range(32 * ((n - 1) // 32), n))
  seen, out = set(), []
  for k in cols:
    if 0 <= k < n and k not in seen:
      seen.add(k)
      out.append(k)
  return out


def dense_case(n, seed, symmetric=True, with_c=True, with_p=True, own_s=False):
  """(M, c, p, s, V) of the dense-block checks: entries N(0,1) 10^U(-6,0)."""
  rng = np.random.default_rng(1000 * n + seed)
  m = rng.standard_normal((n, n)) * 10.0 ** rng.uniform(-6.0, 0.0, (n, n))
  if symmetric:
    m = np.triu(m) + np.triu(m, 1).T
  c = rng.uniform(0.5, 2.0, n) if with_c else None
  p = rng.standard_normal(n) if with_p else None
  s = rng.uniform(0.5, 2.0, n) if own_s else None
  v = rng.standard_normal((n, B))
  return m, c, p, s, v


def refined_affinity(n, seed=None):
  """A symmetric non-negative refined affinity from the oracle: cosine affinity of blobs,
  CropDiagonal, GaussianBlur, RowWiseThreshold, Symmetrize (the ICASSP2018 sequence up to
  Diffuse -- the matrix the matrix-free operator applies twice)."""
  import spectral_oracle as so
  x = so.blobs(n, 32, 4, seed=n if seed is None else seed)
  cfg = so.icassp2018_config()
  cfg.sequence = so.ICASSP2018_SEQUENCE[:4]
  return np.ascontiguousarray(so.refine(so.affinity(x), cfg))


def spectrum_matrix(n, spec, seed):
  """Symmetric matrix with the given spectrum in a random orthogonal basis."""
  rng = np.random.default_rng(seed)
  q, _ = np.linalg.qr(rng.standard_normal((n, n)))
  m = (q * spec) @ q.T
  return 0.5 * (m + m.T)


# ------------------------------------------------------------------------------ Krylov cases
def _top_and_bulk(n, k, top, low, seed):
  """k values from `top` down to `low` over a bulk uniform in [0, 1): the closer `low` is to
  the bulk, the more basis vectors the solver needs."""
  rng = np.random.default_rng(seed)
  return np.concatenate([np.linspace(top, low, k), rng.random(n - k)])


def krylov_case(name):
  """Inputs of the Krylov invariant cases.  Returns a dict:
       kind      "stage" (sc_stage_sym_eig on `matrix`, `count` largest pairs) or "affinity"
                 (given affinity `matrix`, refinement `sequence`, GraphCut Laplacian)
       operator  f(c, p) -> Operator the solver works on (c, p: None = computed here in fp64)
       ref       (m, cycles) the reference chain is run to on the CPU (about where the solver
                 stops; the GPU tests rerun it to the device's own m)
  The spectra of K1 / K5a / K5b were chosen with the restated chain and the driver's check
  schedule: residuals 5x above the tolerance at the check before the asserted basis size and
  10x or more below it at the size itself."""
  if name == "K1":      # n = 129: cap 120, the second 128-row workgroup of a link holds one row
    n, count = 129, 5
    m = spectrum_matrix(n, _top_and_bulk(n, count, 6.0, 4.0, n), n)
    return dict(kind="stage", n=n, matrix=m, count=count, ref=(96, 0),
                operator=lambda c=None, p=None: Operator(m))
  if name == "K2":      # the spectrum of test_gpu_stages.py::test_sym_eig_lanczos_path
    n, count = 777, 21
    rng = np.random.default_rng(n)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    spec = np.concatenate([np.linspace(50, 30, count), rng.random(n - count)])
    m = (q * spec) @ q.T
    m = 0.5 * (m + m.T)
    return dict(kind="stage", n=n, matrix=m, count=count, ref=(64, 0),
                operator=lambda c=None, p=None: Operator(m))
  if name in ("K5a", "K5b"):   # n = 400, cap 128: links of 64 rows from a basis of 112 on
    n, count = 400, 12
    top, low = (4.0, 2.8) if name == "K5a" else (2.0, 1.4)
    m = spectrum_matrix(n, _top_and_bulk(n, count, top, low, n), n)
    return dict(kind="stage", n=n, matrix=m, count=count,
                ref=(128, 0) if name == "K5a" else (128, 1),
                operator=lambda c=None, p=None: Operator(m))
  import spectral_oracle as so
  if name == "K3":      # a given affinity, no refinement, GraphCut: non-trivial c and p
    n = 1000                # (a refined affinity: the cosine affinity of d = 32 embeddings has
    a = refined_affinity(n)  #  rank 33, its Krylov blocks go rank deficient after four steps)

    def op3(c=None, p=None):
      if c is None:
        c, p = scaling_vectors(_chunked_product(a, np.ones((n, 1)), 32)[:, 0], 4)
      return Operator(a, c, p)
    return dict(kind="affinity", n=n, matrix=a, sequence=(), two=False, max_clusters=7,
                ref=(48, 0), operator=op3)
  if name == "K4":      # Diffuse matrix-free: the operator applies the affinity twice.  (The
    n = 640             # route is not taken for a Diffuse that reads the resident affinity
    a = refined_affinity(n)  # itself: Symmetrize, the identity on this input, goes first.)

    def op4(c=None, p=None):
      if c is None:
        one = _chunked_product(a, np.ones((n, 1)), 32)
        c, p = scaling_vectors(_chunked_product(a, one, 32)[:, 0], 4)
      return Operator(a, c, p, two=True)
    return dict(kind="affinity", n=n, matrix=a, sequence=("Symmetrize", "Diffuse"), two=True, max_clusters=7,
                ref=(48, 0), operator=op4)
  raise KeyError(name)


KRYLOV_CASES = ("K1", "K2", "K3", "K4", "K5a", "K5b")
