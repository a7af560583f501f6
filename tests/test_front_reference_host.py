"""The CPU reference chain of the fused front (`tests/_front_ref.py`) against the oracle's
`refine` and the goldens of the real reference, bit for bit.  tests/test_gpu_front.py compares
the device's front with this chain; these tests are what keeps the chain itself honest.  No GPU.
"""

import dataclasses

import numpy as np
import pytest

import spectral_oracle as so
from conftest import golden

import _front_ref as fr

PRESETS = {
    "icassp2018": so.icassp2018_config(),
    "icassp2018_sigma2_p30": so.icassp2018_config(gaussian_blur_sigma=2, p_percentile=0.3),
    "icassp2018_preserve_diagonal": so.icassp2018_config(preserve_diagonal=True),
    "icassp2018_average_binarize": so.icassp2018_config(
        symmetrize_type=so.SYMMETRIZE_AVERAGE, binarize=True),
    "turntodiarize": so.turntodiarize_config(constraint_name=so.CONSTRAINT_NONE),
    "turntodiarize_p40": so.turntodiarize_config(constraint_name=so.CONSTRAINT_NONE,
                                                 p_percentile=0.4),
}


def before_diffuse(cfg):
  seq = list(cfg.sequence)
  if so.OP_DIFFUSE in seq:
    seq = seq[:seq.index(so.OP_DIFFUSE)]
  return dataclasses.replace(cfg, sequence=tuple(seq))


@pytest.mark.parametrize("name", sorted(PRESETS))
@pytest.mark.parametrize("n,d", [(40, 8), (131, 16), (300, 32)])
def test_chain_is_the_oracles_refine(name, n, d):
  cfg = PRESETS[name]
  a0 = so.affinity(so.blobs(n, d, 3, seed=n))
  ref = fr.front(a0, cfg)
  # the matrices: the oracle's refine, stopped before Diffuse / after it / at the end
  assert np.array_equal(ref.a, so.refine(a0, before_diffuse(cfg)))
  assert np.array_equal(ref.a, ref.a.T)
  if so.OP_DIFFUSE in cfg.sequence:
    upto = tuple(cfg.sequence[:list(cfg.sequence).index(so.OP_DIFFUSE) + 1])
    assert np.array_equal(ref.s, so.refine(a0, dataclasses.replace(cfg, sequence=upto)))
  else:
    assert ref.s is None
  assert np.array_equal(fr.refined_from(ref), so.refine(a0, cfg))
  # the vectors: applying them reproduces the oracle's own operations
  m = a0
  if so.OP_CROP_DIAGONAL in cfg.sequence:
    cropped = a0.copy()
    np.fill_diagonal(cropped, ref.cropval)
    assert np.array_equal(cropped, so.crop_diagonal(a0))
    m = so.gaussian_blur(cropped, cfg.gaussian_blur_sigma)
    assert np.array_equal(ref.blurred, m)
  thresholded = so.row_wise_threshold(m, cfg.p_percentile, cfg.soft_multiplier,
                                      cfg.threshold_type, cfg.binarize, cfg.preserve_diagonal)
  assert np.array_equal(fr.apply_cut(m, ref.cut, cfg), thresholded)
  assert np.array_equal(so.symmetrize(thresholded, cfg.symmetrize_type), ref.a)
  last = ref.a if ref.s is None else ref.s
  assert np.array_equal(ref.rowmax, last.max(axis=1))
  assert np.array_equal(ref.rowsum, last.sum(axis=1))
  assert ref.folded_rownorm == (cfg.sequence[-1] == so.OP_ROW_WISE_NORMALIZE)


def test_pieces_against_the_reference_goldens():
  """ops_n40.npz holds the REAL reference's output of every single operation on one input."""
  g = golden("ops_n40.npz")
  m = g["input"]
  cropped = m.copy()
  np.fill_diagonal(cropped, fr.crop_value(m))
  assert np.array_equal(cropped, g["crop"])
  for tname, tt in (("rowmax", so.THRESHOLD_ROW_MAX), ("pct", so.THRESHOLD_PERCENTILE)):
    for bz in (0, 1):
      for pd in (0, 1):
        cfg = so.OracleConfig(p_percentile=0.8, soft_multiplier=0.01, threshold_type=tt,
                              binarize=bool(bz), preserve_diagonal=bool(pd))
        want = g["thr_%s_b%d_d%d" % (tname, bz, pd)]
        assert np.array_equal(fr.apply_cut(m, fr.cut_vector(m, cfg), cfg), want)
  # the whole chain on the golden input: every matrix it passes is the reference's
  for sigma, key in ((1, "blur_s1"), (2, "blur_s2")):
    cfg = dataclasses.replace(so.icassp2018_config(gaussian_blur_sigma=sigma),
                              sequence=(so.OP_GAUSSIAN_BLUR,))
    assert np.array_equal(fr.front(m, cfg).blurred, g[key])
  for st, key in ((so.SYMMETRIZE_MAX, "sym_max"), (so.SYMMETRIZE_AVERAGE, "sym_avg")):
    cfg = so.OracleConfig(sequence=(so.OP_SYMMETRIZE,), symmetrize_type=st)
    assert np.array_equal(fr.front(m, cfg).a, g[key])
  ref = fr.front(g["sym_max"], so.OracleConfig(sequence=(so.OP_DIFFUSE,
                                                         so.OP_ROW_WISE_NORMALIZE)))
  np.testing.assert_allclose(ref.s, so.diffuse(g["sym_max"]), rtol=0, atol=0)
  assert ref.folded_rownorm


@pytest.mark.parametrize("lap", [so.LAPLACIAN_NONE, so.LAPLACIAN_UNNORMALIZED,
                                 so.LAPLACIAN_RANDOM_WALK, so.LAPLACIAN_GRAPH_CUT])
@pytest.mark.parametrize("folded", [False, True])
def test_scaling_vectors_give_the_reference_laplacian(lap, folded):
  """diag(p) + diag(c) S diag(c) with the chain's c, p is the Laplacian of the refined matrix
  up to the similarity transform the solver undoes with t: checked through the golden
  Laplacians' definition (laplacian.py:41-58) on a refined affinity."""
  cfg = so.icassp2018_config()
  if not folded:
    cfg = dataclasses.replace(cfg, sequence=tuple(cfg.sequence[:-1]))
  ref = fr.front(so.affinity(so.blobs(60, 8, 3, seed=60)), cfg)
  c, p, t = fr.scaling_vectors(ref.rowmax, ref.rowsum, lap, ref.folded_rownorm)
  op = np.diag(p) + c[:, None] * ref.s * c[None, :]
  w = fr.refined_from(ref)                      # what the reference hands its Laplacian
  want = so.laplacian(w, lap) if lap != so.LAPLACIAN_NONE else w
  if lap != so.LAPLACIAN_NONE:
    want = -want                                # the solver takes the largest of -L
  # Op = D^-1 (want) D with D = diag(t / c-free factor): similar matrices share their spectrum
  got = np.sort(np.linalg.eigvals(op).real)
  ref_w = np.sort(np.linalg.eigvals(want).real)
  np.testing.assert_allclose(got, ref_w, rtol=0, atol=1e-9 * max(1.0, np.abs(ref_w).max()))
  assert np.all(np.isfinite(t))
