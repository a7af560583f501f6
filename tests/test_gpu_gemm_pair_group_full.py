"""GPU: the grouped two-operand fp64 product (`launch_gemm_nt_pair_group`) in its full-output form
-- every tile of every member from its own operands, what the dense last stage of a grouped
ConstraintPropagation chain needs for X = T Q^T -- through `sc_stage_gemm_pair_group`.

The operands hold small integers, so every partial sum is an exact double whatever the order of
the K sum: the reference is the int64 product and every comparison is an equality.  The entry
point's device memory is NaN-filled before the operands go in: an element of the result that no
tile wrote, or a read outside an operand, shows as a NaN."""

import ctypes

import numpy as np
import pytest

from spectralcluster_amd import _lib

pytestmark = pytest.mark.gpu

EPI_NONE, EPI_ADD = 0, 2
# an idle member in the middle; 129 / 257: one row past a tile edge, 128: exactly one tile,
# 17: less than a tile, 300 / 191: ragged last tiles of a 3 x 3 and a 2 x 2 grid
MIXED = (129, 0, 300, 17, 257, 128, 191)
SIXTEEN = (1, 2, 17, 64, 65, 127, 128, 129, 130, 200, 255, 256, 257, 33, 300, 96)


def matrix_ld(n):
  ld = (n + 15) // 16 * 16
  return ld + 16 if ld % 512 == 0 else ld


def integers(n, seed, low=-3, high=4):
  return np.random.default_rng(seed).integers(low, high, size=(n, n)).astype(np.int64)


def run_group(ns, a_mats, b_mats, addends, epilogue, full):
  """outs[z]: the (n, ld) result buffer of member z, prefilled with -7 on the host (an idle
  member's stays that way)."""
  count = len(ns)
  dp = ctypes.POINTER(ctypes.c_double)
  as_f = [np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in a_mats]
  bs_f = [np.ascontiguousarray(b, dtype=np.float64) if b is not None else None for b in b_mats]
  ad_f = [np.ascontiguousarray(c, dtype=np.float64) if c is not None else None for c in addends]
  outs = [np.full((n, matrix_ld(n)) if n else (3, 3), -7.0) for n in ns]
  pointers = lambda ms: (dp * count)(*[_lib.as_double_p(m) if m is not None and m.size else None
                                      for m in ms])
  handle = _lib.default_handle()
  handle.check(handle.lib.sc_stage_gemm_pair_group(
      handle.raw, count, (ctypes.c_int32 * count)(*ns), pointers(as_f), pointers(bs_f),
      pointers(ad_f) if epilogue == EPI_ADD else None, pointers(outs), epilogue, int(full)))
  return outs


def check_against_int64(ns, outs, a_mats, b_mats, addends, epilogue):
  for z, n in enumerate(ns):
    if n == 0:
      assert np.all(outs[z] == -7.0), "idle member %d was written" % z
      continue
    b = a_mats[z] if b_mats[z] is None else b_mats[z]
    want = a_mats[z] @ b.T
    if epilogue == EPI_ADD:
      want = want + addends[z]
    assert np.max(np.abs(want)) < 2 ** 50
    inside = outs[z][:, :n]  # (the padding columns of the row pitch need not hold anything)
    assert not np.isnan(inside).any(), "member %d (n=%d): an element was not written" % (z, n)
    assert np.array_equal(inside, want.astype(np.float64)), "member %d (n=%d)" % (z, n)


@pytest.mark.parametrize("epilogue", [EPI_NONE, EPI_ADD], ids=["none", "add"])
@pytest.mark.parametrize("ns", [MIXED, SIXTEEN], ids=["mixed", "sixteen"])
def test_full_output_product_is_exact_for_operands_that_are_not_symmetric(ns, epilogue):
  a_mats = [integers(n, 10 + z) if n else None for z, n in enumerate(ns)]
  b_mats = [integers(n, 50 + z) if n else None for z, n in enumerate(ns)]
  addends = [integers(n, 90 + z, -1000, 1000) if n else None for z, n in enumerate(ns)]
  for z, n in enumerate(ns):
    if n >= 17:  # neither operand nor the product is symmetric: a mirror write would show
      assert not np.array_equal(a_mats[z], a_mats[z].T)
      assert not np.array_equal(a_mats[z] @ b_mats[z].T, (a_mats[z] @ b_mats[z].T).T)
  outs = run_group(ns, a_mats, b_mats, addends, epilogue, full=True)
  check_against_int64(ns, outs, a_mats, b_mats, addends, epilogue)


def test_full_output_product_with_b_left_out_is_a_a_transposed():
  ns = (130, 0, 17)
  a_mats = [integers(n, 7 + z) if n else None for z, n in enumerate(ns)]
  outs = run_group(ns, a_mats, [None] * 3, [None] * 3, EPI_NONE, full=True)
  check_against_int64(ns, outs, a_mats, [None] * 3, [None] * 3, EPI_NONE)


@pytest.mark.parametrize("epilogue", [EPI_NONE, EPI_ADD], ids=["none", "add"])
def test_symmetric_form_is_what_it_was_on_commuting_symmetric_operands(epilogue):
  """A = S and B = S S commute and are symmetric, like the factors of the Neumann chain: the
  symmetric form (upper-triangle tiles, mirrors written transposed) gives the exact product too,
  and the full-output form the same bits."""
  ns = MIXED
  a_mats, b_mats, addends = [], [], []
  for z, n in enumerate(ns):
    if n == 0:
      a_mats.append(None), b_mats.append(None), addends.append(None)
      continue
    s = np.triu(integers(n, 200 + z, -1, 2))
    s = s + np.triu(s, 1).T
    c = np.triu(integers(n, 300 + z, -1000, 1000))
    a_mats.append(s), b_mats.append(s @ s), addends.append(c + np.triu(c, 1).T)
  sym = run_group(ns, a_mats, b_mats, addends, epilogue, full=False)
  check_against_int64(ns, sym, a_mats, b_mats, addends, epilogue)
  full = run_group(ns, a_mats, b_mats, addends, epilogue, full=True)
  for z, n in enumerate(ns):
    assert np.array_equal(sym[z][:, :n], full[z][:, :n])


def test_entry_point_errors():
  handle = _lib.default_handle()
  lib = handle.lib
  a = np.eye(4)
  out = np.zeros((4, 16))
  dp = ctypes.POINTER(ctypes.c_double)
  one = lambda m: (dp * 1)(_lib.as_double_p(m))
  ns = (ctypes.c_int32 * 1)(4)
  assert lib.sc_stage_gemm_pair_group(handle.raw, 0, ns, one(a), None, None, one(out), 0,
                                      1) == _lib.SC_ERR_INVALID
  assert lib.sc_stage_gemm_pair_group(handle.raw, 17, ns, one(a), None, None, one(out), 0,
                                      1) == _lib.SC_ERR_INVALID
  assert lib.sc_stage_gemm_pair_group(handle.raw, 1, ns, one(a), None, None, one(out), 1,
                                      1) == _lib.SC_ERR_INVALID  # (the affinity epilogue)
  assert lib.sc_stage_gemm_pair_group(handle.raw, 1, ns, one(a), None, None, one(out), EPI_ADD,
                                      1) == _lib.SC_ERR_INVALID  # (no addends)
  assert lib.sc_stage_gemm_pair_group(handle.raw, 1, (ctypes.c_int32 * 1)(-1), one(a), None,
                                      None, one(out), 0, 1) == _lib.SC_ERR_INVALID
