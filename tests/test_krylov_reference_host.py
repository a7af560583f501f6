"""CPU: the block Lanczos chain restated in NumPy fp64 (tests/_krylov_ref.py) stays within every
bound the GPU tests hold the device kernels to, with a factor 8 to spare, on every input those
tests use.  This is what keeps the bounds honest: a bound that an fp64 implementation in a bad
summation order cannot meet comfortably would be a wrong bound, not a strict one."""

import numpy as np
import pytest

import _krylov_ref as kr

SPARE = 8.0


def _operator_ratio(op, v):
  w = op.apply(v)
  assert np.all(np.isfinite(w))
  err = np.abs(w.astype(kr.LD) - op.apply_ld(v)).astype(np.float64)
  bound = op.bound(v)
  assert np.all(bound > 0.0)
  return float(np.max(err / bound))


def test_gamma_and_start_block():
  assert kr.gamma(1) == pytest.approx(2.0 ** -53, rel=1e-15)
  assert kr.gamma(1000) > 1000 * 2.0 ** -53
  w = kr.start_block(129)
  assert w.shape == (129, 8) and np.all(w >= -1.0) and np.all(w < 1.0)
  # multiples of 2^-52 by construction, and not a degenerate stream
  assert np.array_equal(w * 2.0 ** 52, np.rint(w * 2.0 ** 52))
  assert np.unique(w).size == w.size and abs(w.mean()) < 0.1
  assert kr.basis_cap(129) == 120 and kr.basis_cap(400) == 128 and kr.basis_cap(136) == 128


@pytest.mark.parametrize("n", kr.OPERATOR_SIZES)
def test_position_probe_is_exact_in_fp64(n):
  m = kr.probe_matrix(n)
  assert np.array_equal(m, m.T)
  assert np.unique(m[np.triu_indices(n)]).size == n * (n + 1) // 2
  cols = kr.probe_columns(n)
  assert {0, 1, 7, 8, 31, 32, 33, 127, 128, n - 2, n - 1} <= set(cols)
  assert set(range(64, 96)) <= set(cols) and set(range(32 * ((n - 1) // 32), n)) <= set(cols)
  op = kr.Operator(m)
  v = np.zeros((n, kr.B))
  v[cols[:kr.B], np.arange(kr.B)] = 1.0
  assert np.array_equal(op.apply(v), m[:, cols[:kr.B]])


@pytest.mark.parametrize("n", kr.OPERATOR_SIZES)
def test_reference_operator_within_bound(n):
  ratios = {}
  m, c, p, s, v = kr.dense_case(n, 0)
  ratios["sym"] = _operator_ratio(kr.Operator(m, c, p), v)
  m, c, p, s, v = kr.dense_case(n, 1, symmetric=False, own_s=True)
  ratios["general"] = _operator_ratio(kr.Operator(m, c, p, s), v)
  m, c, p, s, v = kr.dense_case(n, 2, with_c=False, with_p=False)
  ratios["null"] = _operator_ratio(kr.Operator(m), v)
  if n in kr.TWO_PRODUCT_SIZES:
    a = kr.refined_affinity(n)
    assert np.array_equal(a, a.T) and a.min() >= 0.0
    _, c, p, _, v = kr.dense_case(n, 3)
    ratios["two"] = _operator_ratio(kr.Operator(a, c, p, two=True), v)
  print("n=%d error/bound of the fp64 reference:" % n,
        " ".join("%s %.3f" % kv for kv in ratios.items()))
  assert max(ratios.values()) * SPARE <= 1.0, ratios


@pytest.mark.parametrize("name", kr.KRYLOV_CASES)
def test_reference_chain_within_bounds(name):
  case = kr.krylov_case(name)
  op = case["operator"]()
  m_ref, cycles = case["ref"]
  keep = kr.restart_keep(case.get("count", 8), kr.basis_cap(case["n"]))
  chain = kr.Chain(op).run(m_ref, cycles, keep)
  q, t = chain.basis()
  inv = kr.Invariants(op, q, t)
  kry = float(np.max(inv.krylov_err / inv.krylov_bound))
  print("%s n=%d m=%d cycles=%d: orth %.2e (bound %.2e)  proj %.2e (ratio %.3f)  "
        "krylov %.2e (ratio %.3f)" % (name, case["n"], m_ref, cycles, inv.orth, inv.orth_bound,
                                      float(inv.proj_err.max()), inv.proj_ratio(),
                                      float(inv.krylov_err.max()), kry))
  assert inv.symmetric
  assert inv.orth * SPARE <= inv.orth_bound
  if cycles == 0:
    assert inv.proj_ratio() * SPARE <= 1.0
    assert kry * SPARE <= 1.0
  else:
    # after a thick restart T[0:keep, 0:keep] = diag(theta) and the kept vectors are products
    # Q Y: their rounding is not in the derived bounds (the GPU tests take 16 x these figures
    # where they exceed the bound); here they must stay at rounding level
    scale = float(np.max(np.abs(t)))
    assert float(inv.proj_err.max()) <= 64 * kr.gamma(inv.n + inv.m) * scale
    assert float(inv.krylov_err.max()) <= 64 * kr.gamma(inv.n + inv.m) * scale


# ------------------------------------------------------------------------------ block Arnoldi
def _arnoldi_operator(name):
  """The operators of the GPU cases (test_gpu_general_kernels.py, section C), scalings in fp64
  from the row sums as k_scaling_general forms them."""
  import _hessenberg_ref as hr
  n, lap = {"cap56": (65, 0), "pitch129": (129, 0), "affinity_none": (300, 0),
            "random_walk": (520, 3), "graph_cut": (520, 4), "unnormalized": (520, 2),
            "restart": (300, 0)}[name]
  m = (kr.nonnormal_cluster(n) if name == "restart" else
       kr.separated_matrix(n) if name in ("cap56", "pitch129") else hr.thresholded_affinity(n))
  cl, cr, p = kr.general_scaling_vectors(m.sum(axis=1), lap)
  return kr.Operator(m, c=cl, p=p, s=cr), lap


@pytest.mark.parametrize("name", ["cap56", "pitch129", "affinity_none", "random_walk", "graph_cut",
                                  "unnormalized", "restart"])
def test_reference_arnoldi_chain_within_bounds(name):
  import spectral_oracle as so
  op, lap = _arnoldi_operator(name)
  n = op.n
  if lap:  # the scalings are those of the oracle's Laplacian
    dense = np.diag(op.p) + op.c[:, None] * op.m * op.s[None, :]
    want = -so.laplacian(op.m, lap)
    assert np.abs(dense - want).max() <= 4 * kr.gamma(n) * max(1.0, np.abs(want).max())
    assert (lap == 3) == (not np.array_equal(op.c, op.s))
  for m in (24, kr.arnoldi_cap(n)):
    q, opq, h = kr.ArnoldiChain(op).run(m).state()
    inv = kr.ArnoldiInvariants(op, q, opq, h)
    print("%s n=%d m=%d: orth %.2e (bound %.2e)  operator %.3f  projection %.3f  Arnoldi %.2e "
          "(ratio %.3f)" % (name, n, m, inv.orth, inv.orth_bound, inv.op_ratio(), inv.proj_ratio(),
                            inv.arnoldi_figure(), inv.arnoldi_ratio()))
    assert not np.array_equal(h, h.T)          # a full, non-symmetric H
    assert inv.orth * SPARE <= inv.orth_bound
    assert inv.op_ratio() * SPARE <= 1.0
    assert inv.proj_ratio() * SPARE <= 1.0
    assert inv.arnoldi_ratio() * SPARE <= 1.0
  # the wide form's basis
  if name == "affinity_none":
    assert kr.arnoldi_cap(n, wide=True) == 128 and kr.arnoldi_cap(65) == 56
    q, opq, h = kr.ArnoldiChain(op).run(128).state()
    inv = kr.ArnoldiInvariants(op, q, opq, h)
    assert inv.orth * SPARE <= inv.orth_bound and inv.arnoldi_ratio() * SPARE <= 1.0
