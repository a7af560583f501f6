"""A NumPy restatement of the naive online clusterer (reference naive_clusterer.py) in float64
with np.dot / np.linalg.norm, for the tests of the batched form, with the MARGIN of a walk: how
far the nearest decision was from going the other way.  A comparison of labels against this
reference is decisive only when the margin is well above the rounding of a cosine (a few 1e-16
times the row length): the tests ask for more than 1e-9."""

import numpy as np
import spectral_oracle as so

GRID_D = (3, 64, 255, 256, 257, 600)
GRID_N = (1, 2, 65, 300)
# (threshold, adaptation_threshold, blobs): (0.2, 0.2) walks a single blob
GRID_PAIRS = ((0.5, None, 4), (0.7, 0.9, 4), (0.2, 0.2, 1))


def naive_walk(x, threshold, adaptation_threshold=None):
  """(labels, counts, centroids, margin) of NaiveClusterer(threshold, adaptation).predict(x)
  from the empty state.  margin: the smallest of |cos - threshold| and |cos - adaptation| over
  every cosine, and of the gap between the two largest cosines of a row (inf when none)."""
  x = np.asarray(x, dtype=np.float64)
  adaptation = threshold if adaptation_threshold is None else adaptation_threshold
  centroids, counts = [], []
  labels = np.zeros(x.shape[0], dtype=np.int64)
  margin = np.inf
  for i, e in enumerate(x):
    if not centroids:
      centroids.append(e.copy())
      counts.append(1)
      continue
    sims = np.array([np.dot(c, e) / (np.linalg.norm(c) * np.linalg.norm(e)) for c in centroids])
    margin = min(margin, np.abs(sims - threshold).min(), np.abs(sims - adaptation).min())
    if sims.size > 1:
      top = np.sort(sims)
      margin = min(margin, top[-1] - top[-2])
    best = int(np.argmax(sims))
    if sims[best] < threshold:
      centroids.append(e.copy())
      counts.append(1)
      labels[i] = len(centroids) - 1
      continue
    if sims[best] > adaptation:
      centroids[best] = (centroids[best] * counts[best] + e) / (counts[best] + 1)
      counts[best] += 1
    labels[i] = best
  return labels, np.array(counts, dtype=np.int32), np.array(centroids), margin


def verdict(labels):
  """(single, stopped_at) of the verdict form: the first row labelled 1, or n."""
  later = np.flatnonzero(np.asarray(labels) == 1)
  return later.size == 0, int(later[0]) if later.size else len(labels)


def grid():
  """The cases of the kernel tests: (x, threshold, adaptation_threshold) over GRID_D x GRID_N x
  GRID_PAIRS, so.blobs(n, d, k, 7000 + 10 d + j, noise=0.6)."""
  cases = []
  for d in GRID_D:
    for n in GRID_N:
      for j, (threshold, adaptation, k) in enumerate(GRID_PAIRS):
        cases.append((so.blobs(n, d, k, 7000 + 10 * d + j, noise=0.6), threshold, adaptation))
  return cases
