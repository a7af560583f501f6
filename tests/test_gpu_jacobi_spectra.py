"""GPU: the one-workgroup Jacobi eigensolver (jacobi_body of eig.hip: every symmetric problem of
n <= 128) on spectra that are NOT well separated: near-scalar matrices, exact multiplicities,
degenerate diagonals with weak coupling, tight clusters, what degenerate embeddings produce, and
matrices scaled to both ends of the fp64 range.

On such inputs a rotation between two (nearly) equal diagonal entries is about 45 degrees however
small the off-diagonal entry is, so a sweep of "small" off-diagonal entries does not leave a
diagonal matrix behind; a stop rule that looks at the entries alone returns after one sweep with
the off-diagonals it was given.  Every case is held to the bars test_sym_eig_dense_path sets for
this kernel on Gaussian input:

  eigenvalues   within 1e-12 max|w| of np.linalg.eigvalsh of the same fp64 matrix,
  residual      max|M V - V w| < 1e-11 max|w|,
  vectors       max|V^T V - I| <= 1e-12,

for descend in (True, False) -- the ascending order runs on a negated copy --, and with
max|w| = 0 everything is exactly 0.  LAPACK holds 1e-14 max|w| on all of these inputs, so the bars
leave it a factor of 100.  Vectors inside an eigenspace are not defined one by one: they are
checked through the residual and orthonormality only.

Sizes: 2 / 3 (smallest even / odd, odd n pads to n + 1), 16 and 33 (two pair rows per wave:
n / 2 <= 32), 64 / 65 (the last size of that form and the first of the other), 96 / 97 (vector
accumulator in LDS / in global memory), 127 / 128 (the full 4 x 16-wave unroll at 128).
"""

import numpy as np
import pytest

import spectral_oracle as so
import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from test_gpu_hard_spectra import _matrix_with_spectrum

pytestmark = pytest.mark.gpu

JACOBI = 1  # SC_EIG_PATH_DENSE_JACOBI
ALL_SIZES = [2, 3, 16, 33, 64, 65, 96, 97, 127, 128]


def eigenpairs(handle, m, descend):
  """sc_stage_sym_eig for all n pairs of m; (values, vectors, diag)"""
  n = m.shape[0]
  m = np.ascontiguousarray(m, dtype=np.float64)
  values = np.empty(n)
  vectors = np.empty((n, n))
  diag = _lib.ScDiag()
  handle.check(handle.lib.sc_stage_sym_eig(
      handle.raw, _lib.as_double_p(m), n, n, int(descend), _lib.as_double_p(values),
      _lib.as_double_p(vectors), diag))
  return values, vectors, diag


def check(handle, m, name):
  n = m.shape[0]
  assert np.array_equal(m, m.T), name
  want = np.linalg.eigvalsh(m)
  scale = np.abs(want).max()
  for descend in (True, False):
    w, v, diag = eigenpairs(handle, m, descend)
    assert diag.eig_path == JACOBI, (name, descend, diag.eig_path)
    ref = want[::-1] if descend else want
    err = np.abs(w - ref).max()
    res = np.abs(m @ v - v * w).max()
    orth = np.abs(v.T @ v - np.eye(n)).max()
    rel = scale if scale > 0 else 1.0
    print("%s descend=%d: eigenvalue error %.3g  residual %.3g  (of max|w| = %.3g)  "
          "|V^T V - I| %.3g" % (name, descend, err / rel, res / rel, scale, orth))
    where = (name, descend)
    assert err <= 1e-12 * scale, where + ("eigenvalues", err / rel)
    if scale > 0:
      assert res < 1e-11 * scale, where + ("residual", res / rel)
    else:
      assert res == 0.0, where + ("residual", res)
    assert orth <= 1e-12, where + ("orthonormality", orth)


def gaussian_sym(n, seed):
  a = np.random.default_rng(seed).standard_normal((n, n))
  return a + a.T


# ---------------------------------------------------------------- c I + eps P
@pytest.mark.parametrize("n", ALL_SIZES)
@pytest.mark.parametrize("eps", [1e-6, 1e-9, 1e-10, 1e-12, 1e-14])
@pytest.mark.parametrize("c", [1.0, -2.5])
def test_near_scalar(handle, c, eps, n):
  """c < 0 also puts the negated copy of descend=False on a positive diagonal and the plain one
  on a negative diagonal"""
  m = c * np.eye(n) + eps * gaussian_sym(n, n)
  check(handle, m, "near_scalar c=%g eps=%g n=%d" % (c, eps, n))


# ---------------------------------------------------------------- exact multiplicities
def multiplicity_spectrum(kind, n):
  if kind == "two_values":  # multiplicity ceil(n / 2) and floor(n / 2)
    return np.array([2.0] * ((n + 1) // 2) + [1.0] * (n // 2))
  if kind == "eight_over_bulk":
    bulk = np.sort(np.random.default_rng(n).uniform(0.0, 1.0, n - 8))[::-1]
    return np.concatenate([[3.0] * 8, bulk])
  if kind == "all_but_one":  # multiplicity n - 1 and one outlier
    return np.array([5.0] + [1.0] * (n - 1))
  raise ValueError(kind)


MULTIPLICITY_CASES = (
    [("two_values", n) for n in ALL_SIZES] + [("all_but_one", n) for n in ALL_SIZES] +
    [("eight_over_bulk", n) for n in ALL_SIZES if n >= 16])


@pytest.mark.parametrize("kind,n", MULTIPLICITY_CASES)
def test_exact_multiplicities(handle, kind, n):
  m = _matrix_with_spectrum(multiplicity_spectrum(kind, n), seed=1000 + n)
  check(handle, m, "%s n=%d" % (kind, n))


# ---------------------------------------------------------------- degenerate diagonal
@pytest.mark.parametrize("n", [16, 33, 64, 97, 128])
def test_degenerate_diagonal_weak_coupling(handle, n):
  """diag(3 x 8, 2 x 4, bulk) + 1e-10 P: a restarted Rayleigh-Ritz matrix with locked copies of
  a multiple eigenvalue looks like this"""
  bulk = np.sort(np.random.default_rng(n).uniform(0.0, 1.0, n - 12))[::-1]
  m = np.diag(np.concatenate([[3.0] * 8, [2.0] * 4, bulk])) + 1e-10 * gaussian_sym(n, 2000 + n)
  check(handle, m, "degenerate_diagonal n=%d" % n)


# ---------------------------------------------------------------- tight cluster
@pytest.mark.parametrize("n", [64, 97, 128])
def test_tight_cluster(handle, n):
  """nine values within 1e-8 relative of 3.0, then 1.2 and 0.7, then a bulk below 5e-3: the case
  test_gpu_hard_spectra.py has at n = 650, at the sizes of this kernel"""
  head = list(3.0 * (1.0 + 1e-8 * np.arange(9)[::-1] / 9.0)) + [1.2, 0.7]
  bulk = np.sort(np.random.default_rng(n).uniform(0.0, 5e-3, n - len(head)))[::-1]
  m = _matrix_with_spectrum(np.concatenate([head, bulk]), seed=3000 + n)
  check(handle, m, "tight_cluster n=%d" % n)


# ---------------------------------------------------------------- degenerate embeddings
def block_of_similar_rows(b, seed):
  u = np.random.default_rng(seed).uniform(0.6, 1.0, (b, b))
  u = 0.5 * (u + u.T)
  np.fill_diagonal(u, 1.0)
  return u


def embedding_matrix(kind, n):
  rng = np.random.default_rng(4000 + n)
  if kind == "all_ones":  # identical embeddings
    return np.ones((n, n))
  if kind == "half_ones_half_identity":
    return 0.5 * np.ones((n, n)) + 0.5 * np.eye(n)
  if kind == "disconnected_identical_blocks":  # kron(I_4, B)
    return np.kron(np.eye(4), block_of_similar_rows(n // 4, 4000 + n))
  if kind == "rows_repeated_three_times":  # cosine affinity, rank <= 6
    x = np.repeat(rng.standard_normal(((n + 2) // 3, 5)), 3, axis=0)[:n]
    a = so.affinity(x)
    return 0.5 * (a + a.T)
  if kind == "zero":
    return np.zeros((n, n))
  if kind == "hollow":  # zero diagonal: the kernel's scale (max |diagonal|) is 0
    m = gaussian_sym(n, 4000 + n)
    np.fill_diagonal(m, 0.0)
    return m
  if kind == "diagonal_repeated":
    return np.diag(rng.permutation(np.resize([4.0, 4.0, 4.0, -1.5, -1.5, 0.25, 0.0, 0.0], n)))
  if kind == "graded_12_decades":
    return _matrix_with_spectrum(np.logspace(-12, 0, n), seed=4000 + n)
  raise ValueError(kind)


EMBEDDING_CASES = (
    [(kind, n) for kind in ("all_ones", "half_ones_half_identity", "rows_repeated_three_times",
                            "zero", "hollow", "diagonal_repeated", "graded_12_decades")
     for n in (33, 97, 128)] +
    [("disconnected_identical_blocks", n) for n in (64, 96, 128)])


@pytest.mark.parametrize("kind,n", EMBEDDING_CASES)
def test_what_degenerate_embeddings_produce(handle, kind, n):
  check(handle, embedding_matrix(kind, n), "%s n=%d" % (kind, n))


# ---------------------------------------------------------------- scaling
@pytest.mark.parametrize("n", [33, 96, 127])
def test_scaled_down_to_1e_minus_150(handle, n):
  check(handle, gaussian_sym(n, 5000 + n) * 1e-150, "scaled 1e-150 n=%d" % n)


@pytest.mark.parametrize("n", [33, 96, 127])
def test_scaled_up_to_1e_plus_150(handle, n):
  check(handle, gaussian_sym(n, 5000 + n) * 1e+150, "scaled 1e+150 n=%d" % n)


# ---------------------------------------------------------------- mode 1: c_i c_j A_ij + delta_ij p_i
def duplicate_row_affinity(n):
  """two groups of exactly identical embeddings: a rank-2 affinity of two constant blocks"""
  x = np.vstack([np.tile([[1.0, 0.2, 0.0]], (6 * n // 10, 1)),
                 np.tile([[0.0, 0.3, 1.0]], (n - 6 * n // 10, 1))])
  a = so.affinity(x)
  return 0.5 * (a + a.T)


OPERATOR_INPUTS = {
    "kron4_n96": lambda: np.kron(np.eye(4), block_of_similar_rows(24, 96)),
    "kron5_n125": lambda: np.kron(np.eye(5), block_of_similar_rows(25, 125)),
    "duplicate_rows_n100": lambda: duplicate_row_affinity(100),
}
OPERATOR_LAPLACIANS = [(so.LAPLACIAN_NONE, None),
                       (so.LAPLACIAN_UNNORMALIZED, sca.LaplacianType.Unnormalized),
                       (so.LAPLACIAN_GRAPH_CUT, sca.LaplacianType.GraphCut)]


@pytest.mark.parametrize("lap_code,lap", OPERATOR_LAPLACIANS, ids=["none", "unnormalized", "graphcut"])
@pytest.mark.parametrize("name", sorted(OPERATOR_INPUTS))
def test_scaled_operator_of_the_pipeline(name, lap_code, lap):
  """The kernel's mode 1 with the Laplacian's scaling vectors, through
  _compute_eigenvectors_ncluster on an unrefined affinity: every eigenvalue against eigvalsh of
  the oracle's Laplacian, absolute to max|w| (the k-fold zero eigenvalue of k disconnected
  components has no relative accuracy), and the oracle's eigengap decision."""
  a = OPERATOR_INPUTS[name]()
  n = a.shape[0]
  descend = lap is None
  ref = np.linalg.eigvalsh(so.laplacian(a, lap_code) if not descend else a)
  ref = ref[::-1] if descend else ref
  scale = np.abs(ref).max()
  want_k, _ = so.eigengap(ref, 10, 1e-2, so.EIGENGAP_RATIO, descend)
  c = sca.SpectralClusterer(
      min_clusters=2, max_clusters=10, laplacian_type=lap,
      refinement_options=sca.RefinementOptions(refinement_sequence=[]))
  vectors, k, _ = c._compute_eigenvectors_ncluster(a)
  assert c.last_diag.eig_path == JACOBI
  w = c.consumed_eigenvalues()
  assert 11 <= w.shape[0] <= n and vectors.shape[0] == n
  err = np.abs(w - ref[:w.shape[0]]).max()
  print("%s lap=%d: %d eigenvalues, error %.3g of max|w| = %.3g" % (
      name, lap_code, w.shape[0], err / scale, scale))
  assert err <= 1e-12 * scale, (name, lap_code, err / scale)
  assert k == c.last_diag.n_clusters_raw == want_k
