"""Pairwise-constraint operators (mirror of reference `spectralcluster/constraint.py`).

`AffinityIntegration` and `ConstraintPropagation` run on the device through
`sc_stage_constraint`; inside `SpectralClusterer.predict` the constraint matrix stays
resident and the same kernels run in the pipeline (`sc_set_constraint`).  Wherever a
constraint matrix is accepted, a `ConstraintMatrix` instance is accepted too: its n - 1 band
values travel instead of the (n, n) array of `compute_diagonals()`
(`sc_set_constraint_band` / `sc_stage_constraint_band`).  A `PairwiseConstraints` instance -- a
list of must-link / cannot-link pairs -- is accepted as well: its K directed entries travel
(`sc_set_constraint_pairs` / `sc_stage_constraint_pairs`), 16 bytes each, and no (n, n) array is
built on either side.  A `DenseConstraints` instance wraps a dense (n, n) matrix that is read where
it is -- host or device memory, float64 / float32 / float16 / bfloat16, any strides -- and widened
exactly on the device (`sc_set_constraint_array` / `sc_stage_constraint_array`); in a batch it
travels inside the library call.  An ndarray always takes the dense route through the host
(widened to float64 there, `sc_set_constraint`), and a `DenseConstraints` the dense arithmetic,
whatever either holds: no band or sparse structure is looked for.  The E2CP
inverse `(I - alpha * A_norm)^-1` is evaluated as a Neumann product of fp64 MFMA GEMMs
(see `csrc/constraint_api.hip: constraint_propagation`), which needs |alpha| < 1 and a
non-negative affinity; anything else raises `UnsupportedOnDeviceError`.
"""

from __future__ import annotations

import abc
import ctypes
import dataclasses
import enum
import typing

import numpy as np

from spectralcluster_amd import _dlpack
from spectralcluster_amd import _lib

EPS = 1e-10


class ConstraintName(enum.Enum):
  """Constrained-clustering methods (reference constraint.py:10-16)."""
  AffinityIntegration = 1
  ConstraintPropagation = 2


class IntegrationType(enum.Enum):
  """How AffinityIntegration merges the two matrices (reference constraint.py:19-22)."""
  Max = 1
  Average = 2


def _device_adjust(affinity: np.ndarray, constraint_matrix, name: ConstraintName,
                   integration_type: typing.Optional[IntegrationType],
                   alpha: float) -> np.ndarray:
  src = np.ascontiguousarray(affinity, dtype=np.float64)
  banded = isinstance(constraint_matrix, ConstraintMatrix)
  paired = isinstance(constraint_matrix, PairwiseConstraints)
  dense = isinstance(constraint_matrix, DenseConstraints)
  if not paired and not dense:
    con = constraint_matrix.band() if banded else np.ascontiguousarray(
        constraint_matrix, dtype=np.float64)
  cfg = _lib.ScConfig()
  _lib.load().sc_config_default(cfg)
  cfg.constraint_name = name.value
  cfg.constraint_before_refinement = 1
  cfg.integration_type = integration_type.value if integration_type is not None else 0
  cfg.constraint_alpha = float(alpha)
  out = np.empty_like(src)
  handle = _lib.default_handle()
  if dense:
    with _lib.use_device(handle.device):
      with constraint_matrix.describe(lambda: handle) as source:
        handle.check(handle.lib.sc_stage_constraint_array(
            handle.raw, cfg, _lib.as_double_p(src), ctypes.byref(source.array), src.shape[0],
            _lib.as_double_p(out)), TypeError)
    return out
  if paired:
    rows, cols, vals = constraint_matrix.entries()
    handle.check(handle.lib.sc_stage_constraint_pairs(
        handle.raw, cfg, _lib.as_double_p(src), _lib.as_int32_p(rows), _lib.as_int32_p(cols),
        _lib.as_double_p(vals), len(vals), src.shape[0], _lib.as_double_p(out)))
    return out
  stage = handle.lib.sc_stage_constraint_band if banded else handle.lib.sc_stage_constraint
  handle.check(stage(
      handle.raw, cfg, _lib.as_double_p(src), _lib.as_double_p(con), src.shape[0],
      _lib.as_double_p(out)))
  return out


class ConstraintOperation(metaclass=abc.ABCMeta):
  """Base class of the two operators (reference constraint.py:51-92)."""

  def check_input(self, affinity: np.ndarray, constraint_matrix):
    """Same checks and messages as reference constraint.py:54-76.  A `ConstraintMatrix`
    stands for the (n, n) matrix of its `compute_diagonals()`, n = its number of scores; a
    `PairwiseConstraints` for the (n, n) matrix of its `to_dense()`; a `DenseConstraints` is
    the (n, n) matrix it holds."""
    if isinstance(constraint_matrix, (ConstraintMatrix, PairwiseConstraints, DenseConstraints)):
      n = (len(constraint_matrix.speaker_turn_scores)
           if isinstance(constraint_matrix, ConstraintMatrix) else constraint_matrix.n)
      constraint_matrix = np.lib.stride_tricks.as_strided(np.zeros(1, dtype=bool), (n, n), (0, 0))
    for what, m in (("affinity", affinity), ("constraint matrix", constraint_matrix)):
      if len(m.shape) != 2:
        raise ValueError("%s must be 2-dimensional" % what)
      if m.shape[0] != m.shape[1]:
        raise ValueError("%s must be a square matrix" % what)
    if affinity.shape != constraint_matrix.shape:
      raise ValueError("affinity and constraint matrix must have the same shape")

  @abc.abstractmethod
  def adjust_affinity(self, affinity: np.ndarray,
                      constraint_matrix: np.ndarray) -> np.ndarray:
    """Returns the adjusted (n, n) affinity."""


class AffinityIntegration(ConstraintOperation):
  """max(A, Q) or (A + Q) / 2 (reference constraint.py:95-118)."""

  def __init__(self, integration_type: IntegrationType = IntegrationType.Max):
    self.integration_type = integration_type

  def adjust_affinity(self, affinity, constraint_matrix):
    self.check_input(affinity, constraint_matrix)
    if not isinstance(self.integration_type, IntegrationType):
      raise ValueError("Unsupported integration type: {}".format(self.integration_type))
    return _device_adjust(affinity, constraint_matrix, ConstraintName.AffinityIntegration,
                          self.integration_type, 0.0)


class ConstraintPropagation(ConstraintOperation):
  """Exhaustive and efficient constraint propagation, E2CP (Lu & Ip, ECCV 2010;
  reference constraint.py:121-164): F = (1-a)^2 (I - a A_norm)^-1 Q (I - a A_norm)^-1,
  then A <- 1 - (1 - F)(1 - A) where F > 0 and (1 + F) A elsewhere."""

  def __init__(self, alpha: float = 0.6):
    self.alpha = alpha

  def adjust_affinity(self, affinity, constraint_matrix):
    self.check_input(affinity, constraint_matrix)
    return _device_adjust(affinity, constraint_matrix, ConstraintName.ConstraintPropagation,
                          None, self.alpha)


@dataclasses.dataclass
class ConstraintOptions:
  """Option bag handed to SpectralClusterer (reference constraint.py:25-48)."""
  constraint_name: ConstraintName
  # True: adjust the raw affinity (suggested for ConstraintPropagation);
  # False: adjust the refined matrix (suggested for AffinityIntegration).
  apply_before_refinement: bool
  integration_type: typing.Optional[IntegrationType] = None
  constraint_propagation_alpha: float = 0.6

  def __post_init__(self):
    if self.constraint_name == ConstraintName.AffinityIntegration:
      self.constraint_operator = AffinityIntegration(self.integration_type)
    elif self.constraint_name == ConstraintName.ConstraintPropagation:
      self.constraint_operator = ConstraintPropagation(self.constraint_propagation_alpha)

  def to_config(self, cfg: _lib.ScConfig) -> None:
    """Fill the constraint fields of an `sc_config`."""
    if not isinstance(self.constraint_name, ConstraintName):
      raise TypeError("constraint_name must be a ConstraintName")
    cfg.constraint_name = self.constraint_name.value
    cfg.constraint_before_refinement = int(bool(self.apply_before_refinement))
    if self.constraint_name == ConstraintName.AffinityIntegration:
      # read the live operator, like the reference does at call time
      kind = self.constraint_operator.integration_type
      if not isinstance(kind, IntegrationType):
        raise ValueError("Unsupported integration type: {}".format(kind))
      cfg.integration_type = kind.value
    else:
      cfg.constraint_alpha = float(self.constraint_operator.alpha)


class ConstraintMatrix:
  """Constraint matrix from speaker-turn confidences (reference constraint.py:167-207):
  adjacent segments without a turn must link (+1); a turn whose score exceeds
  `threshold` makes them cannot-link (-1).  Host-side: O(n) scalar work."""

  def __init__(self, speaker_turn_scores: typing.Sequence[float], threshold: float = 1):
    if any(score < 0 for score in speaker_turn_scores):
      raise ValueError("Speaker turn score must be larger or equal to 0.")
    self.speaker_turn_scores = speaker_turn_scores
    self.threshold = threshold

  def band(self) -> np.ndarray:
    """The n - 1 values `compute_diagonals()` puts on the first super- and sub-diagonal:
    band[i] = Q[i, i + 1] = Q[i + 1, i] (float64, shape (max(n - 1, 0),)).  What the device
    needs of the matrix; pass the `ConstraintMatrix` itself wherever a constraint matrix is
    accepted and only these travel."""
    nxt = np.asarray(self.speaker_turn_scores, dtype=np.float64)[1:]
    return np.where(nxt == 0, 1.0, np.where(nxt > self.threshold, -1.0, 0.0))

  def compute_diagonals(self) -> np.ndarray:
    scores = np.asarray(self.speaker_turn_scores, dtype=np.float64)
    n = len(scores)
    out = np.zeros((n, n))
    if n < 2:
      return out
    nxt = scores[1:]  # nxt[i]: turn score between segment i and i + 1
    band = np.where(nxt == 0, 1.0, np.where(nxt > self.threshold, -1.0, 0.0))
    idx = np.arange(n - 1)
    out[idx, idx + 1] = band
    out[idx + 1, idx] = band
    return out


class PairwiseConstraints:
  """Constraint matrix given as a list of pairs: Q[i, j] = Q[j, i] = v for every listed pair
  {i, j}, 0 elsewhere (the input E2CP is about: a handful of must-link / cannot-link pairs).

  `must_link` / `cannot_link`: sequences of (i, j), values +1 / -1 (the convention of
  `ConstraintMatrix.compute_diagonals`).  `pairs` (m, 2) with `values` (m,): arbitrary finite
  weights.  i == j is allowed and gives one entry on the diagonal.  Pass the object wherever a
  constraint matrix is accepted and only its entries travel to the device."""

  def __init__(self, n: int, must_link: typing.Sequence = (), cannot_link: typing.Sequence = (),
               pairs=None, values=None):
    self.n = int(n)
    if self.n < 0:
      raise ValueError("n must not be negative")
    if (pairs is None) != (values is None):
      raise ValueError("pairs and values must be given together")
    ij = [np.asarray(must_link, dtype=np.int64).reshape(-1, 2),
          np.asarray(cannot_link, dtype=np.int64).reshape(-1, 2)]
    v = [np.ones(len(ij[0])), -np.ones(len(ij[1]))]
    if pairs is not None:
      pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
      values = np.asarray(values, dtype=np.float64).reshape(-1)
      if len(pairs) != len(values):
        raise ValueError("pairs and values must have the same length")
      ij.append(pairs)
      v.append(values)
    self._pairs = np.concatenate(ij)
    self._values = np.concatenate(v).astype(np.float64)
    if np.any(self._pairs < 0) or np.any(self._pairs >= self.n):
      raise ValueError("pair index outside [0, n)")
    if not np.all(np.isfinite(self._values)):
      raise ValueError("constraint values must be finite")
    key = self._pairs.min(axis=1) * max(self.n, 1) + self._pairs.max(axis=1)
    if len(np.unique(key)) != len(key):
      raise ValueError("a pair is listed twice")

  @classmethod
  def from_dense(cls, q) -> "PairwiseConstraints":
    """The non-zeros of a symmetric (n, n) matrix."""
    q = np.asarray(q, dtype=np.float64)
    if q.ndim != 2 or q.shape[0] != q.shape[1]:
      raise ValueError("constraint matrix must be a square matrix")
    if not np.array_equal(q, q.T):
      raise ValueError("constraint matrix must be symmetric")
    i, j = np.nonzero(np.triu(q))
    return cls(q.shape[0], pairs=np.stack([i, j], axis=1), values=q[i, j])

  def to_dense(self) -> np.ndarray:
    """The (n, n) float64 matrix the pairs stand for."""
    out = np.zeros((self.n, self.n))
    out[self._pairs[:, 0], self._pairs[:, 1]] = self._values
    out[self._pairs[:, 1], self._pairs[:, 0]] = self._values
    return out

  def entries(self) -> typing.Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(rows int32, cols int32, vals float64): the directed entries Q[rows[e], cols[e]] =
    vals[e], in the order the pairs were given -- (i, j) then (j, i), adjacent; a diagonal pair
    gives one entry.  What `sc_set_constraint_pairs` takes."""
    i, j = self._pairs[:, 0], self._pairs[:, 1]
    rows = np.stack([i, j], axis=1).reshape(-1)
    cols = np.stack([j, i], axis=1).reshape(-1)
    keep = np.stack([np.ones(len(i), dtype=bool), i != j], axis=1).reshape(-1)
    return (np.ascontiguousarray(rows[keep], dtype=np.int32),
            np.ascontiguousarray(cols[keep], dtype=np.int32),
            np.ascontiguousarray(np.repeat(self._values, 2)[keep], dtype=np.float64))

  def __array__(self, dtype=None, copy=None):
    out = self.to_dense()
    return out if dtype is None else out.astype(dtype, copy=False)


def check_square_input(matrix, what: str) -> int:
  """The TypeError / ValueError for an object that is no (n, n) matrix -- no `shape`, not 2-D,
  not square -- before any device is touched.  Returns n."""
  shape = np.shape(matrix) if isinstance(matrix, np.ndarray) else getattr(matrix, "shape", None)
  if shape is None:
    raise TypeError("%s must be a numpy array or support __dlpack__" % what)
  shape = tuple(int(s) for s in shape)
  if len(shape) != 2:
    raise ValueError("%s must be 2-dimensional, got shape %s" % (what, shape))
  if shape[0] != shape[1]:
    raise ValueError("%s must be a square matrix, got shape %s" % (what, shape))
  return shape[0]


class DenseConstraints:
  """A dense (n, n) constraint matrix taken where it is: a model's pairwise same-speaker /
  different-speaker scores, learned must-link weights -- a NumPy array or an object with
  `__dlpack__` (a PyTorch tensor on the clusterer's GPU), float64 / float32 / float16 / bfloat16,
  contiguous or a strided view (a `.T`, every other column of a wider array).

  The object is stored as it is: nothing is copied or converted here, and the device widens the
  values exactly when a call reads them, deciding in the same kernel pass whether the matrix is
  symmetric.  A device tensor needs no synchronisation by the caller and may be overwritten or
  freed when the call that read it has returned.  Pass the wrapper wherever a constraint matrix is
  accepted; inside `predict_batch` / `predict_affinity_batch` it travels in the library call,
  where a raw ndarray sends the batch through per-utterance calls.

  No structure is detected: a `DenseConstraints` always takes the dense arithmetic (two n^3
  products in ConstraintPropagation), also when the matrix it holds is a band or a handful of
  pairs -- `ConstraintMatrix` and `PairwiseConstraints` are the forms for those.

  TypeError / ValueError as `predict_affinity` raises them for its matrix, here at construction:
  an object without a shape, not 2-D, not square; a dtype that is none of the four (nothing is
  promoted here); a negative stride.  An ndarray is checked in full.  A DLPack object is checked
  through its `dtype` attribute and its `stride()` / `strides`, which PyTorch, CuPy and JAX arrays
  have, without asking for a capsule; one that has neither is checked when a call describes it,
  with the same errors."""

  _DTYPE_NAMES = ("float64", "float32", "float16", "bfloat16")

  def __init__(self, matrix):
    what = "constraint matrix"
    self.n = check_square_input(matrix, what)
    if isinstance(matrix, np.ndarray):
      if matrix.dtype not in (np.dtype(np.float64), np.dtype(np.float32), np.dtype(np.float16)):
        raise TypeError(_dlpack.dtype_message(what, "got %s" % matrix.dtype))
      strides = matrix.strides
    elif not (hasattr(matrix, "__dlpack__") and hasattr(matrix, "__dlpack_device__")):
      raise TypeError("%s must be a numpy array or support __dlpack__" % what)
    else:
      dtype = getattr(matrix, "dtype", None)
      # ("torch.float32", "float32", dtype('float32'), "<class 'jax.numpy.float32'>")
      if dtype is not None and not any(
          str(getattr(dtype, "name", dtype)).split(".")[-1].rstrip("'>") == name
          for name in self._DTYPE_NAMES):
        raise TypeError(_dlpack.dtype_message(what, "got %s" % dtype))
      strides = getattr(matrix, "stride", None)
      strides = strides() if callable(strides) else getattr(matrix, "strides", None)
    if strides is not None and any(int(s) < 0 for s in strides):
      raise ValueError(_dlpack.negative_strides_message("constraint matrices"))
    self.matrix = matrix

  @property
  def shape(self) -> typing.Tuple[int, int]:
    return (self.n, self.n)

  def describe(self, get_handle):
    """The `_dlpack.Source` of the matrix as it lies (release() it after the library call)."""
    return _dlpack.describe(self.matrix, get_handle, strided=True)
