"""CPU: the references of the general path's kernel tests (tests/_hessenberg_ref.py), so that
what the device kernels are compared with is itself pinned.

  * the reflector convention: q_from_packed on LAPACK's dgehrd output reproduces dorghr, and
    Q^T M Q is the Hessenberg matrix dgehrd returned;
  * the NumPy dgehd2 (gehd2) that feeds the host half's tests holds the figures the device is
    held to: max(8 x scipy.linalg.hessenberg's, n eps);
  * the a-priori bounds of the Rayleigh-Ritz kernels: fp64 restatements of k_gen_ritz,
    k_gen_residual (+ reduce) and k_gen_phase in the kernels' own summation order stay inside
    every bound on every input of the GPU test -- the residual bound with a factor 8 to spare,
    the per-entry bounds with a factor 2 (the test says why 8 is out of reach for a sum of eight
    products) -- so the bounds are those of an honest fp64 implementation and not fitted to
    the device;
  * the generated inputs are what their names say; the three test entries are declared,
    prototyped, exported and reject a NULL handle."""

import os
import re

import numpy as np
import pytest
import scipy.linalg
from scipy.linalg import lapack

import _hessenberg_ref as hr
from spectralcluster_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sc_stage_hessenberg", "sc_stage_general_ritz", "sc_stage_arnoldi_state")


def test_stage_entries_are_declared_prototyped_and_exported():
  header = open(os.path.join(ROOT, "include", "spectralcluster_amd.h")).read()
  lib = _lib.load()
  for name in ENTRIES:
    assert re.search(r"^int\s+%s\s*\(" % name, header, flags=re.M), name
    assert name in _lib.PROTOTYPES and hasattr(lib, name), name
  assert re.search(r"^#define SC_ABI_VERSION 11$", header, flags=re.M)
  assert lib.sc_abi_version() == _lib.SC_ABI_VERSION == 11
  none = [None] * 20
  assert lib.sc_stage_hessenberg(None, None, 0, None, None, None) == _lib.SC_ERR_INVALID
  assert lib.sc_stage_general_ritz(None, None, None, 0, 0, *none[:4], 0, *none[:6], None, 0,
                                   None) == _lib.SC_ERR_INVALID
  assert lib.sc_stage_arnoldi_state(None, *none[:7]) == _lib.SC_ERR_INVALID


@pytest.mark.parametrize("n", [3, 4, 34, 131])
def test_reflector_convention_reproduces_dorghr(n):
  m = hr.gaussian(n)
  packed, tau, info = lapack.dgehrd(m)
  assert info == 0
  want, info = lapack.dorghr(packed, tau)
  assert info == 0
  q = hr.q_from_packed(packed, np.concatenate([tau, [0.0]]))
  assert np.max(np.abs(q - want)) <= n * hr.EPS
  orth, res = hr.reduction_figures(m, q, hr.hessenberg_part(packed))
  assert orth <= n * hr.EPS and res <= 4 * n * hr.EPS


@pytest.mark.parametrize("n", [1, 2, 3, 5, 35, 67, 129, 258])
def test_numpy_gehd2_holds_the_device_bars(n):
  m = hr.gaussian(n)
  packed, tau = hr.gehd2(m)
  q = hr.q_from_packed(packed, tau)
  orth, res = hr.reduction_figures(m, q, hr.hessenberg_part(packed))
  hl, ql = scipy.linalg.hessenberg(m, calc_q=True)
  orth_l, res_l = hr.reduction_figures(m, ql, hl)
  assert orth <= max(8 * orth_l, n * hr.EPS), (orth, orth_l)
  assert res <= max(8 * res_l, n * hr.EPS), (res, res_l)
  assert np.all((tau == 0.0) | ((tau >= 1.0) & (tau <= 2.0)))
  assert np.all(np.abs(np.tril(packed, -2)) <= 1.0)


def test_figures_are_scale_invariant_and_see_a_wrong_factor():
  n = 40
  m = hr.gaussian(n)
  hl, ql = scipy.linalg.hessenberg(m, calc_q=True)
  base = hr.reduction_figures(m, ql, hl)
  for k in (-500, 500):
    f = float(np.ldexp(1.0, k))
    assert hr.reduction_figures(m * f, ql, hl, f) == base          # H kept in scaled units
  assert hr.reduction_figures(m, ql, hl, 2.0)[1] > 0.1              # a wrong `scale` shows
  hl[7, 3] = 1e-9                                                  # so does an entry of H
  assert hr.reduction_figures(m, ql, hl)[1] > 1e-11


def test_inputs_are_what_their_names_say():
  for n in hr.STRUCTURE_SIZES:
    assert not np.tril(hr.structure("hessenberg", n), -2).any()
    assert not np.tril(hr.structure("triangular", n), -1).any()
    assert np.linalg.matrix_rank(hr.structure("rank_one", n)) == 1
    g = np.abs(hr.structure("graded_rows", n)).max(axis=1)
    assert 1e10 < g[-1] / g[0] < 1e14
    z = hr.structure("zero_border", n)
    assert not z[:40].any() and not z[:, :40].any() and z[40:, 40:].all()
    a = hr.structure("affinity", n)
    assert a.min() >= 0.0 and not np.array_equal(a, a.T)
    lap = hr.structure("random_walk", n)
    assert np.abs(lap.sum(axis=1)).max() < 1e-8 and not np.array_equal(lap, lap.T)
    bd = hr.structure("block_diagonal", n)
    e = np.cumsum(hr.block_sizes(n))[0]
    assert not bd[e:, :e].any() and not bd[:e, e:].any() and bd[:e, :e].all()
  u = hr.unit_gaussian(67)
  assert 0.5 <= np.abs(u).max() < 1.0
  for name in hr.SCALINGS:
    m, rescaled = hr.scaled(name, 67)
    e = int(np.frexp(np.abs(m).max())[1])
    assert np.all(np.isfinite(m)) and (abs(e) > 400) == rescaled, name
  t = hr.tiny_column(67)
  assert np.all(t[2:, 0] ** 2 == 0.0) and t[2:, 0].all() and 1 < np.abs(t).max() < 8


@pytest.mark.parametrize("kind", hr.RITZ_KINDS)
def test_ritz_restatements_sit_inside_their_bounds(kind):
  worst = {"ritz": 0.0, "resid": 0.0, "phase": 0.0}
  for n, m, cols in hr.ritz_shapes():
    if n == 129 and m not in (8, 128):
      continue  # (the CPU sweep: every m and cols, two of the three n)
    q, opq, yre, yim, tre, tim = hr.ritz_case(kind, n, m, cols)
    vr, vi = hr.ritz_fp64(q, yre, yim)
    exact = hr.ritz_exact(q, yre, yim)
    err = np.abs((vr.astype(hr.LD) + 1j * vi.astype(hr.LD)) - exact).astype(np.float64)
    bound = hr.ritz_bound(q, yre, yim)
    assert np.all(bound > 0)
    worst["ritz"] = max(worst["ritz"], float((err / bound).max()))
    got = hr.residual_fp64(q, opq, yre, yim, tre, tim)
    want = hr.residual_exact(q, opq, yre, yim, tre, tim).astype(np.float64)
    rb = hr.residual_bound(q, opq, yre, yim, tre, tim)
    worst["resid"] = max(worst["resid"], float((np.abs(got - want) / rb).max()))
    if kind == "converged":  # all cancellation: ~1e-13 against |OpQ||y| of order 1e3
      assert want.max() < 1e-9 * np.abs(opq).max()
    pr, pi = hr.phase_fp64(vr, vi)
    pe = hr.phase_exact(vr, vi)
    perr = np.abs((pr.astype(hr.LD) + 1j * pi.astype(hr.LD)) - pe).astype(np.float64)
    pb = hr.phase_bound(n, pe).astype(np.float64)
    ok = pb > 0
    worst["phase"] = max(worst["phase"], float((perr[ok] / pb[ok]).max()))
    assert not perr[~ok].any()
  print(kind, worst)
  # The residual bound has its factor 8 to spare (measured: 0.018 at most).  The Ritz-vector and
  # phase bounds cannot: they count every rounding once and worst case, and an entry that is one
  # dominant product already errs by u / 2 for the product and u / 2 for each of the m - 1
  # additions that carry it -- half of gamma_m, m = 8 (measured: 0.48 on the six-decade data,
  # 0.22 on the Gaussian; 0.04 - 0.17 at m >= 64).  The phase bound is fifteen roundings of which
  # a result meets five (0.35 at most).  They are held inside the bound with a factor 2.
  assert worst["resid"] * 8 <= 1.0, worst
  assert worst["ritz"] * 2 <= 1.0, worst
  assert worst["phase"] * 2 <= 1.0, worst


def test_residual_reference_sees_theta_im_and_the_pivot_rule_sees_order():
  q, opq, yre, yim, tre, tim = hr.ritz_case("gaussian", 65, 24, 1)
  tim = tim + 0.5
  full = hr.residual_exact(q, opq, yre, yim, tre, tim).astype(np.float64)
  no_im = hr.residual_exact(q, opq, yre, yim, tre, 0 * tim).astype(np.float64)
  assert np.all(np.abs(full - no_im) > 1e3 * hr.residual_bound(q, opq, yre, yim, tre, tim))
  for first, second in ((5, 300), (255, 256), (300, 261), (0, 332)):
    vr, vi = hr.tie_column(333, first, second, 1)
    assert hr.phase_pivot(vr[:, None], vi[:, None])[0] == min(first, second)
    assert hr.phase_pivot_gap(vr[:, None], vi[:, None])[0] >= 0.5 - 2 * 0.35 ** 2 - 1e-12
    mag = vr * vr + vi * vi
    assert mag[first] == mag[second] == 0.5 and np.sum(mag == 0.5) == 2


def test_gather_noise_is_the_kernels_hash():
  a = hr.gather_noise(100, 3, 0x9E3779B97F4A7C16)
  b = hr.gather_noise(100, 4, 0x9E3779B97F4A7C16)
  assert np.all((a >= -1.0) & (a < 1.0)) and np.unique(a).size == 100
  assert not np.array_equal(a, b)
  assert np.array_equal(a, hr.gather_noise(100, 3, 0x9E3779B97F4A7C16))
