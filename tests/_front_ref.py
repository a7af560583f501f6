"""CPU reference chain of the fused refinement front (tests/test_gpu_front.py).

Everything between the affinity and the eigensolver, computed in NumPy from an affinity the
caller supplies -- the tests pass the affinity the DEVICE returned, so that no comparison depends
on GEMM rounding -- with the intermediate vectors the fused kernels keep on the device: the
CropDiagonal value, the cut vector of RowWiseThreshold, the refined matrix before Diffuse,
S = A A^T with its row statistics, and the scaling vectors of the operator the eigensolver works
on.  The matrices come from the oracle's own operations (`spectral_oracle`); the vectors are
recomputed here and `tests/test_front_reference_host.py` pins both against `so.refine` and the
goldens of the real reference, bit for bit.
"""

import dataclasses
import typing

import numpy as np

import spectral_oracle as so

EPS = 1e-10  # laplacian.py:6


@dataclasses.dataclass
class FrontRef:
  cropval: typing.Optional[np.ndarray]   # None: no CropDiagonal in the sequence
  blurred: typing.Optional[np.ndarray]   # None: no GaussianBlur
  cut: typing.Optional[np.ndarray]       # None: no RowWiseThreshold
  a: np.ndarray                          # the refined matrix before Diffuse
  s: typing.Optional[np.ndarray]         # Diffuse(a); None: no Diffuse in the sequence
  rowmax: np.ndarray                     # row statistics of the last matrix (s, else a)
  rowsum: np.ndarray
  folded_rownorm: bool                   # the sequence ends in RowWiseNormalize


def crop_value(a0: np.ndarray) -> np.ndarray:
  """max(0, max over j != i of a0[i, j]) (refinement.py:148-150: the diagonal is zeroed, then
  set to the row maximum)."""
  m = np.array(a0, dtype=np.float64, copy=True)
  np.fill_diagonal(m, -np.inf)
  return np.maximum(0.0, m.max(axis=1))


def cut_vector(m: np.ndarray, cfg: so.OracleConfig) -> np.ndarray:
  """The row cut of RowWiseThreshold as the configuration computes it (refinement.py:185-197)."""
  m = np.array(m, dtype=np.float64, copy=True)
  if cfg.preserve_diagonal:
    np.fill_diagonal(m, 0.0)
  if cfg.threshold_type == so.THRESHOLD_ROW_MAX:
    return m.max(axis=1) * cfg.p_percentile
  if cfg.threshold_type == so.THRESHOLD_PERCENTILE:
    return np.percentile(m, cfg.p_percentile * 100, axis=1)
  raise ValueError("Unsupported thresholding_type")


def apply_cut(m: np.ndarray, cut: np.ndarray, cfg: so.OracleConfig) -> np.ndarray:
  """RowWiseThreshold given its cut vector (refinement.py:198-210); the host test holds it to
  `so.row_wise_threshold`."""
  out = np.array(m, dtype=np.float64, copy=True)
  if cfg.preserve_diagonal:
    np.fill_diagonal(out, 0.0)
  small = out < cut[:, None]
  keep = np.ones_like(out) if cfg.binarize else out
  out = np.where(small, out * cfg.soft_multiplier, keep)
  if cfg.preserve_diagonal:
    np.fill_diagonal(out, 1.0)
  return out


def front(a0: np.ndarray, cfg: so.OracleConfig) -> FrontRef:
  """The sequence of `cfg` on `a0`, op by op with the oracle's operations, keeping what the
  fused front keeps.  Sequences: any order of CropDiagonal, GaussianBlur, RowWiseThreshold,
  Symmetrize, then optionally Diffuse and a final RowWiseNormalize."""
  m = np.array(a0, dtype=np.float64, copy=True)
  cropval = blurred = cut = s = None
  folded = False
  seq = list(cfg.sequence)
  for i, op in enumerate(seq):
    if s is not None and op != so.OP_ROW_WISE_NORMALIZE:
      raise ValueError("nothing but RowWiseNormalize may follow Diffuse here")
    if op == so.OP_CROP_DIAGONAL:
      cropval = crop_value(m)
      m = so.crop_diagonal(m)
    elif op == so.OP_GAUSSIAN_BLUR:
      m = blurred = so.gaussian_blur(m, cfg.gaussian_blur_sigma)
    elif op == so.OP_ROW_WISE_THRESHOLD:
      cut = cut_vector(m, cfg)
      m = so.row_wise_threshold(m, cfg.p_percentile, cfg.soft_multiplier, cfg.threshold_type,
                                cfg.binarize, cfg.preserve_diagonal)
    elif op == so.OP_SYMMETRIZE:
      m = so.symmetrize(m, cfg.symmetrize_type)
    elif op == so.OP_DIFFUSE:
      s = so.diffuse(m)
    elif op == so.OP_ROW_WISE_NORMALIZE:
      if i != len(seq) - 1:
        raise ValueError("RowWiseNormalize must be last")
      folded = True
    else:
      raise ValueError("Unknown refinement operation: {}".format(op))
  last = m if s is None else s
  return FrontRef(cropval, blurred, cut, m, s, last.max(axis=1), last.sum(axis=1), folded)


def scaling_vectors(rowmax: np.ndarray, rowsum: np.ndarray, laplacian_type: int,
                    folded_rownorm: bool):
  """c, p, t of Op = diag(p) + diag(c) S diag(c) (csrc/rowops.hip, above scaling_vectors_body),
  each operation rounded once in float64, in the kernel's order."""
  rowmax = np.asarray(rowmax, dtype=np.float64)
  rowsum = np.asarray(rowsum, dtype=np.float64)
  a = 1.0 / rowmax if folded_rownorm else np.ones_like(rowmax)
  sa = np.sqrt(a)
  deg = rowsum / rowmax if folded_rownorm else rowsum.copy()
  c, p, t = sa.copy(), np.zeros_like(sa), sa.copy()
  if laplacian_type == so.LAPLACIAN_UNNORMALIZED:
    p = -deg
  elif laplacian_type == so.LAPLACIAN_RANDOM_WALK:
    g = 1.0 / (deg + EPS)
    c = np.sqrt(g * a)
    p = -(g * deg)
    t = c.copy()
  elif laplacian_type == so.LAPLACIAN_GRAPH_CUT:
    h = 1.0 / (np.sqrt(deg) + EPS)
    c = h * sa
    p = -((h * deg) * h)
  return c, p, t


def refined_from(ref: FrontRef) -> np.ndarray:
  """What `so.refine` returns for the whole sequence, from the pieces."""
  last = ref.a if ref.s is None else ref.s
  return last / ref.rowmax[:, None] if ref.folded_rownorm else last
