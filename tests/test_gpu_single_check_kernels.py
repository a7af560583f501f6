"""GPU: the single-cluster test of a batch (spectralcluster_amd/csrc/single_check.hip) through
`sc_batch_single_check` -- the short form (n <= 128, one workgroup per matrix, the whole decision in
one launch) and the chain form (128 < n < 4096, grouped launches, parameters updated on the device)
-- against the single call's `sc_affinity_stats` / `sc_affinity_gmm_bic` on the same matrix and
against the host restatement (tests/_single_check_ref.py).

Inputs: sizes either side of kDenseMax = 128 and of a wavefront of rows, the smallest legal n for
offset 1, and sizes whose 2-component EM outlasts one look at the slots; three classes per size
(one noisy speaker, one tight speaker, three speakers).  Bars: minima bit-equal; mean and std
rtol 1e-12 (the bar of the golden statistics test); BICs rtol 1e-9 (the project's bar for bic1
against sklearn, five orders below the smallest relative gap between the two BICs of a case);
Lloyd and EM step counts equal to the host restatement's.  Every matrix is checked alone and
inside one mixed call of all of them."""

import ctypes

import numpy as np
import pytest

import _single_check_ref as ref_lib

from spectralcluster_amd import _lib

pytestmark = pytest.mark.gpu

V = {name: i for i, name in enumerate(_lib.SINGLE_CHECK_VALUES)}


def batch_check(mats, condition, offset, threshold=0.0):
  """One sc_batch_single_check call; outputs NaN / -1 filled before it."""
  count = len(mats)
  values = np.full((count, 8), np.nan)
  single = np.full(count, -1, dtype=np.int32)
  handle = _lib.default_handle()
  ap = (ctypes.POINTER(ctypes.c_double) * count)(*[_lib.as_double_p(a) for a in mats])
  ns = (ctypes.c_int * count)(*[a.shape[0] for a in mats])
  check = _lib.ScSingleCheck(condition, offset, threshold)
  rc = handle.lib.sc_batch_single_check(
      handle.raw, ap, ns, count, ctypes.byref(check), _lib.as_double_p(values),
      single.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
  return rc, values, single, handle


def single_call(a, offset):
  """sc_affinity_stats and sc_affinity_gmm_bic on `a`: (stats[4], bic[2])."""
  handle = _lib.default_handle()
  handle.check(handle.lib.sc_set_affinity(handle.raw, _lib.as_double_p(a), a.shape[0]))
  stats, bic = np.empty(4), np.empty(2)
  handle.check(handle.lib.sc_affinity_stats(handle.raw, _lib.as_double_p(stats)))
  handle.check(handle.lib.sc_affinity_gmm_bic(handle.raw, offset, _lib.as_double_p(bic[0:1]),
                                              _lib.as_double_p(bic[1:2])))
  return stats, bic


@pytest.fixture(scope="module", params=[1, 2])
def run(request):
  """Per offset: the cases, each matrix's record from a call of its own and from ONE mixed call
  of all of them (AffinityGmmBic), and the single call's values."""
  offset = request.param
  cases = ref_lib.cases(offset)
  mats = [ref_lib.case_affinity(n, cls) for n, cls in cases]
  rc, mixed, mixed_single, handle = batch_check(mats, 1, offset)
  handle.check(rc)
  alone, alone_single = [], []
  for a in mats:
    rc, values, single, handle = batch_check([a], 1, offset)
    handle.check(rc)
    alone.append(values[0])
    alone_single.append(single[0])
  out = {"offset": offset, "cases": cases, "mats": mats, "mixed": mixed,
         "mixed_single": mixed_single, "alone": np.stack(alone),
         "alone_single": np.array(alone_single),
         "single_call": [single_call(a, offset) for a in mats]}
  for key in ("mixed", "alone"):
    out[key].setflags(write=False)
  return out


def test_records_vs_single_call_and_restatement(run):
  for i, (n, cls) in enumerate(run["cases"]):
    ref = ref_lib.case_reference(n, cls, run["offset"])
    ref_lib.assert_margins(ref, (n, cls))
    stats, bic = run["single_call"][i]
    for where in ("alone", "mixed"):
      got = run[where][i]
      print(run["offset"], n, cls, where, list(got), list(stats), list(bic))
      assert not np.isnan(got).any()
      assert got[V["min"]] == stats[0] and got[V["neighbor_min"]] == stats[1]
      np.testing.assert_allclose(got[[V["mean"], V["std"]]], stats[2:], rtol=1e-12)
      np.testing.assert_allclose(got[[V["bic1"], V["bic2"]]], bic, rtol=1e-9)
      assert got[V["lloyd_steps"]] == ref["lloyd_steps"], (n, cls, where)
      assert got[V["em_steps"]] == ref["em_steps"], (n, cls, where)
      # (and the restatement itself: the same arithmetic in NumPy's summation order)
      np.testing.assert_allclose(got[[V["bic1"], V["bic2"]]], [ref["bic1"], ref["bic2"]],
                                 rtol=1e-9)


def test_alone_is_mixed_bit_for_bit_and_calls_repeat(run):
  assert run["alone"].tobytes() == run["mixed"].tobytes()
  assert np.array_equal(run["alone_single"], run["mixed_single"])
  rc, again, again_single, handle = batch_check(run["mats"], 1, run["offset"])
  handle.check(rc)
  assert again.tobytes() == run["mixed"].tobytes()
  assert np.array_equal(again_single, run["mixed_single"])


def test_verdicts_of_all_four_conditions(run):
  for condition in (1, 2, 3, 4):
    threshold = ref_lib.THRESHOLDS.get(condition, 0.0)
    rc, values, single, handle = batch_check(run["mats"], condition, run["offset"], threshold)
    handle.check(rc)
    assert not np.isnan(values).any() and set(single.tolist()) <= {0, 1}
    # (the statistics do not depend on the condition; the mixture runs for AffinityGmmBic alone)
    assert values[:, :4].tobytes() == run["mixed"][:, :4].tobytes()
    if condition != 1:
      assert not values[:, 4:].any()
    for i, (n, cls) in enumerate(run["cases"]):
      ref = ref_lib.case_reference(n, cls, run["offset"])
      assert bool(single[i]) == ref_lib.verdict(ref, condition), (n, cls, condition)
      rc, one_values, one, handle = batch_check([run["mats"][i]], condition, run["offset"],
                                                threshold)
      handle.check(rc)
      assert one[0] == single[i] and one_values.tobytes() == values[i:i + 1].tobytes()


def test_offset_beyond_the_matrix_fails_before_launch():
  mats = [ref_lib.case_affinity(64, "a"), ref_lib.case_affinity(3, "a")]
  rc, values, single, handle = batch_check(mats, 1, 2)   # n = 3: offset 2 >= n - 1
  assert rc == _lib.SC_ERR_INVALID
  with pytest.raises(ValueError, match=ref_lib.OFFSET_MESSAGE) as err:
    handle.check(rc)
  assert "(utterance 1)" in str(err.value)
  assert np.isnan(values).all() and (single == -1).all()
  # the other three conditions do not read the offset
  rc, values, single, handle = batch_check(mats, 2, 2, 0.75)
  handle.check(rc)
  assert not np.isnan(values).any() and single.tolist() == [1, 1]
