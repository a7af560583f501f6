"""`utils.get_cluster_centroids` restated in NumPy with the order of the adds written out: row c
of the result is the sum from 0.0 of the float64 rows with label c, in ascending row index, divided
by their number.  Rows with a negative label belong to no cluster, a label in range(k) that no row
carries gives a row of NaN (0 / 0), k = max(labels) + 1 (0 when every label is negative).  The
result is float64; `centroid_bits` narrows it through `_narrow_ref` to the bits an output of
another dtype holds."""

import numpy as np

import _narrow_ref as nr


def centroids(x: np.ndarray, labels: np.ndarray) -> np.ndarray:
  x = np.asarray(x, dtype=np.float64)
  labels = np.asarray(labels).astype(np.int64)
  assert x.ndim == 2 and labels.shape == (x.shape[0],)
  k = max(int(labels.max()) + 1, 0) if labels.size else 0
  sums = np.zeros((k, x.shape[1]), dtype=np.float64)
  counts = np.zeros(k, dtype=np.float64)
  for i in range(x.shape[0]):  # ascending i: the order is the contract
    c = int(labels[i])
    if c >= 0:
      sums[c] = sums[c] + x[i]
      counts[c] += 1.0
  with np.errstate(invalid="ignore", divide="ignore"):
    return sums / counts[:, None]


def centroid_bits(x: np.ndarray, labels: np.ndarray, dtype: str) -> np.ndarray:
  return nr.narrow_bits(centroids(x, labels), dtype)


def wide_range_input(rng: np.random.Generator, n: int, d: int) -> np.ndarray:
  """Every column spans three decades (and both signs): another order of the adds rounds
  differently."""
  return rng.standard_normal((n, d)) * 10.0 ** rng.uniform(0.0, 3.0, size=(n, d))
