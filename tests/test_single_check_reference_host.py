"""The host restatement of the single-cluster decision (tests/_single_check_ref.py) against
sklearn's GaussianMixture on the inputs of the single-check tests, to the bars of
test_gpu_fallback.test_gmm_bic_vs_sklearn; and the margins that keep those inputs away from a
tie.  No GPU."""

import numpy as np
import pytest

import _single_check_ref as ref_lib


@pytest.mark.parametrize("n", ref_lib.SHORT_SIZES + ref_lib.CHAIN_SIZES)
def test_reference_vs_sklearn(n):
  from sklearn.mixture import GaussianMixture
  for cls in ref_lib.CLASSES:
    ref = ref_lib.case_reference(n, cls, 1)
    vals = ref_lib.entries(ref_lib.case_affinity(n, cls), 1)[:, None]
    want1 = GaussianMixture(n_components=1).fit(vals).bic(vals)
    want2 = GaussianMixture(n_components=2, random_state=0).fit(vals).bic(vals)
    print(n, cls, ref["bic1"], want1, ref["bic2"], want2)
    np.testing.assert_allclose(ref["bic1"], want1, rtol=1e-9)
    np.testing.assert_allclose(ref["bic2"], want2, rtol=1e-3)  # EM stops at tol=1e-3 per sample


@pytest.mark.parametrize("offset", [1, 2])
def test_inputs_are_not_near_ties(offset):
  """|bic1 - bic2| >= 1 and every EM stop decision at least 1e-6 from its threshold; the three
  classes are what their names say under all four conditions, the statistics at least 0.15
  (minima, thresholds 0.75) and 0.07 (std, threshold 0.1) away from their thresholds."""
  cases = ref_lib.cases(offset)
  assert len(cases) == (24 if offset == 1 else 21)  # (n = 3 has no entries at offset 2)
  for n, cls in cases:
    ref = ref_lib.case_reference(n, cls, offset)
    print(offset, n, cls, ref)
    ref_lib.assert_margins(ref, (n, cls, offset))
    if n >= 64:
      assert ref_lib.verdict(ref, 1) == (cls == "b"), (n, cls)
    if cls in "ab":
      assert ref["min"] >= 0.9 and ref["neighbor_min"] >= 0.9 and ref["std"] <= 0.03
    else:
      assert ref["min"] <= 0.55 and ref["neighbor_min"] <= 0.55 and ref["std"] >= 0.19
    for condition in (2, 3, 4):
      assert ref_lib.verdict(ref, condition) == (cls in "ab"), (n, cls, condition)


def test_step_counts_of_the_restatement():
  """Class (b) stops its EM at the second pass, class (a) needs more than one chunk of passes."""
  for n in ref_lib.CHAIN_SIZES:
    assert ref_lib.case_reference(n, "b", 1)["em_steps"] == 2
    a = ref_lib.case_reference(n, "a", 1)
    assert 4 <= a["em_steps"] <= 6 and 12 <= a["lloyd_steps"] <= 30
