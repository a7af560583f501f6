"""GPU: what a real block Lanczos solve leaves behind -- the basis Q, the projected matrix T, the
scaling vectors -- held to rounding-level invariants instead of to a converged spectrum
(`sc_stage_krylov_state`).  A Krylov iteration forgives a basis orthonormal only to 1e-9, a
stale Cholesky factor or links that sum one partial too few: it merely converges a little later.
These checks do not.  (One thing they cannot see, and nothing at rounding level can: T without
the CGS-2 term H2.  H2 = Q^T (W - Q H1) IS the rounding error of the first projection; on the
restated chain T = H1 alone satisfies T = Q^T Op Q to 9.3e-16 against 1.6e-15 with the term.)
The bounds (u = 2^-53, gamma_k = k u / (1 - k u); derivations in tests/_krylov_ref.py,
all reference quantities in longdouble, Op built on the host from the input and the RETURNED c, p):

  orthonormality   max |Q^T Q - I| <= 4 gamma_{n+m}
  projection       |T - Q^T Op Q|_ij <= 2 gamma_{n+m+8} (|Q|^T |Op| |Q|)_ij + m orth max|T|
  symmetry         T == T^T exactly
  Krylov property  |(I - Q Q^T) Op Q[:, 0:m-8]|_ij <= operator bound_ij + m orth max|T|
                   + 16 x the same figure of the fp64 reference chain on the same operator
  scaling vectors  diag(p) + diag(c) S diag(c) is minus the oracle's GraphCut Laplacian of S,
                   entry by entry to gamma_n (gamma_2n where S = A A is applied as two products:
                   its degrees are two nested sums of length n)

After a thick restart each tolerance is the larger of the bound and 16 x the reference chain's
figure carried through the same restart (the products Q Y of the kept Ritz vectors add terms the
bounds do not derive).  Every case asserts the route it exists for."""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _krylov_ref as kr
import spectral_oracle as so
import spectralcluster_amd as sca
from spectralcluster_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPH_CUT = 4


def krylov_state(handle):
  info = (ctypes.c_int32 * 8)()
  handle.check(handle.lib.sc_stage_krylov_state(handle.raw, info, None, None, None, None, None))
  m, n = info[0], info[1]
  q, t, g = np.empty((n, m)), np.empty((m, m)), np.empty((kr.B, kr.B))
  c, p = np.empty(n), np.empty(n)
  handle.check(handle.lib.sc_stage_krylov_state(
      handle.raw, info, _lib.as_double_p(q), _lib.as_double_p(t), _lib.as_double_p(g),
      _lib.as_double_p(c), _lib.as_double_p(p)))
  return dict(m=m, n=n, two=bool(info[2]), ahead=info[3], cycles=info[4], q=q, t=t, g=g, c=c, p=p)


def solve(handle, case):
  """The case's solve on the default handle; returns its sc_diag."""
  if case["kind"] == "stage":
    n, count = case["n"], case["count"]
    values, vectors = np.empty(count), np.empty((n, count))
    diag = _lib.ScDiag()
    m = np.ascontiguousarray(case["matrix"])
    handle.check(handle.lib.sc_stage_sym_eig(handle.raw, _lib.as_double_p(m), n, count, 1,
                                             _lib.as_double_p(values), _lib.as_double_p(vectors),
                                             diag))
    return diag
  seq = [getattr(sca.RefinementName, s) for s in case["sequence"]]
  clusterer = sca.SpectralClusterer(
      min_clusters=2, max_clusters=case["max_clusters"],
      refinement_options=sca.RefinementOptions(refinement_sequence=seq),
      laplacian_type=sca.LaplacianType.GraphCut)
  clusterer.diffuse_mode = 2 if case["two"] else 1
  clusterer._compute_eigenvectors_ncluster(case["matrix"])
  return clusterer.last_diag


def check_scaling(case, st):
  """c, p reproduce Op = -L_GraphCut(S) (laplacian.py:56-57, scaling_vectors_body)."""
  a = case["matrix"]
  n, two = case["n"], case["two"]
  al = a.astype(kr.LD)
  one = np.ones(n, dtype=kr.LD)
  deg = al @ (al @ one) if two else al @ one
  sdiag = np.einsum("ij,ij->i", al, al) if two else np.diag(al)
  cref, pref = kr.scaling_vectors(deg, GRAPH_CUT)
  g = kr.gamma(2 * n if two else n)
  c, p = st["c"].astype(kr.LD), st["p"].astype(kr.LD)
  # off-diagonal entries c_i c_j S_ij: S_ij is common to both sides
  off = float(np.max(np.abs(np.outer(c, c) - np.outer(cref, cref)) / np.outer(cref, cref)))
  dia = float(np.max(np.abs((p + c * c * sdiag) - (pref + cref * cref * sdiag)) /
                     (np.abs(pref) + cref * cref * sdiag)))
  # ... and against the oracle's own (fp64) Laplacian, which carries as much rounding again
  s = so.diffuse(a) if two else a
  op = np.diag(st["p"]) + np.outer(st["c"], st["c"]) * s
  mag = np.diag(np.abs(st["p"])) + np.outer(st["c"], st["c"]) * np.abs(s)
  diff = np.abs(op + so.laplacian(s, so.LAPLACIAN_GRAPH_CUT))
  assert np.all(diff[mag == 0.0] == 0.0)
  ora = float(np.max(diff[mag > 0.0] / mag[mag > 0.0]))
  print("  scaling: entries off-diagonal %.2e diagonal %.2e (bound %.2e); against the oracle's "
        "Laplacian %.2e (bound %.2e)" % (off, dia, g, ora, 2 * g))
  assert off <= g and dia <= g and ora <= 2 * g
  assert np.all(st["c"] > 0) and np.all(st["p"] < 0)


def run_case(name, handle=None):
  """Solve, fetch the state, check every invariant; prints one table row.  Returns (diag, state)."""
  handle = handle or _lib.default_handle()
  case = kr.krylov_case(name)
  diag = solve(handle, case)
  assert diag.eig_path == 2, "not block Lanczos: eig_path %d" % diag.eig_path
  st = krylov_state(handle)
  n, m = st["n"], st["m"]
  assert n == case["n"] and m == diag.eig_basis and st["cycles"] == diag.eig_cycles
  assert st["two"] == bool(case.get("two", False))
  if case["kind"] == "affinity":
    check_scaling(case, st)
    op = case["operator"](st["c"], st["p"])
  else:
    assert np.all(st["c"] == 1.0) and np.all(st["p"] == 0.0)
    op = case["operator"]()
  inv = kr.Invariants(op, st["q"], st["t"])
  keep = kr.restart_keep(case.get("count", 8), kr.basis_cap(n))
  ref = kr.Invariants(op, *kr.Chain(op).run(m, st["cycles"], keep).basis())
  rf = ref.figures()
  restarted = st["cycles"] > 0
  orth_tol = max(inv.orth_bound, 16.0 * rf["orth"]) if restarted else inv.orth_bound
  proj_ratio = inv.proj_ratio(16.0 * rf["proj"] if restarted else 0.0)
  kry_ratio = inv.krylov_ratio(rf["krylov"])
  fg = inv.figures()
  print("%s n=%d m=%d cycles=%d run-ahead=%d host_chain=%d | orth %.2e bound %.2e ref %.2e | "
        "proj %.2e err/bound %.3f ref %.2e | krylov %.2e err/bound %.3f ref %.2e" % (
            name, n, m, st["cycles"], st["ahead"], diag.eig_host_chain, fg["orth"], orth_tol,
            rf["orth"], fg["proj"], proj_ratio, rf["proj"], fg["krylov"], kry_ratio, rf["krylov"]))
  assert inv.symmetric, "T is not exactly symmetric"
  assert inv.orth <= orth_tol
  assert proj_ratio <= 1.0
  assert kry_ratio <= 1.0
  return diag, st


def test_k1_two_workgroups_second_with_one_row(handle):
  diag, _ = run_case("K1", handle)
  assert diag.eig_basis >= 64


def test_k2_n777(handle):
  run_case("K2", handle)


def test_k3_given_affinity_graph_cut(handle):
  diag, st = run_case("K3", handle)
  assert np.ptp(st["c"]) > 0 and np.ptp(st["p"]) > 0   # non-trivial scaling


def test_k4_two_product_operator(handle):
  diag, st = run_case("K4", handle)
  assert diag.diffuse_path == 2 and st["two"]


def test_k5_basis_of_112_and_more(handle):
  diag, _ = run_case("K5a", handle)
  assert diag.eig_basis >= 112     # the links ran in their 64-row form


def test_k5_thick_restart(handle):
  diag, _ = run_case("K5b", handle)
  assert diag.eig_cycles >= 1 and diag.eig_basis >= 112


def test_state_is_refused_without_a_lanczos_solve(handle):
  m = kr.spectrum_matrix(64, np.linspace(1.0, 2.0, 64), 64)   # n <= 128: dense Jacobi
  vals = np.empty(3)
  handle.check(handle.lib.sc_stage_sym_eig(handle.raw, _lib.as_double_p(m), 64, 3, 1,
                                           _lib.as_double_p(vals), None, None))
  info = (ctypes.c_int32 * 8)()
  rc = handle.lib.sc_stage_krylov_state(handle.raw, info, None, None, None, None, None)
  assert rc == _lib.SC_ERR_INVALID and "block Lanczos" in handle.last_error()
  fresh = _lib.Handle(handle.device)
  assert fresh.lib.sc_stage_krylov_state(fresh.raw, info, None, None, None, None,
                                         None) == _lib.SC_ERR_INVALID
  fresh.close()


# K6: the same solves in a fresh interpreter each (the switches are read once per process)
@pytest.mark.parametrize("name,switch", [("K2", "SC_MATVEC_SYM_MIN_N=129"),
                                         ("K3", "SC_MATVEC_SYM_MIN_N=129"),
                                         ("K2", "SC_EIG_HOST_CHAIN=1"),
                                         ("K3", "SC_EIG_HOST_CHAIN=1")])
def test_k6_alternate_routes(name, switch):
  code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
          "import test_gpu_krylov_invariants as t\n"
          "diag, st = t.run_case(%r)\n"
          "print('HOST_CHAIN', diag.eig_host_chain)\n"
          "print('KRYLOV_CASE_OK')\n") % (os.path.join(ROOT, "tests"), ROOT,
                                          os.path.join(ROOT, "oracle"), name)
  env = dict(os.environ)
  key, _, value = switch.partition("=")
  env[key] = value
  r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                     env=env)
  print(r.stdout)
  assert r.returncode == 0 and "KRYLOV_CASE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
  if key == "SC_EIG_HOST_CHAIN":
    assert "HOST_CHAIN 1" in r.stdout
