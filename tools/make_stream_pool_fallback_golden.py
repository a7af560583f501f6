#!/usr/bin/env python3
"""Writes tests/golden/stream_pool_fallback.npz: the rows and sklearn's own labels for the sizes
at which the pooled fallback clusterer is tested (tests/test_gpu_stream_pool_early.py).

  rows_<n>          (n, 16) float64: conversation(8000 + n, n, noise=0.25), the generator of
                    tests/test_gpu_stream_pool.py
  labels_<n>_t05    AgglomerativeClustering(n_clusters=None, metric="cosine", linkage="average",
  labels_<n>_t19      distance_threshold=0.5 | 1.9).fit_predict(rows_<n>); 1.9 merges everything
  min_gap_<n>       smallest difference between two distinct pair distances (scipy pdist)
  height_gap_<n>    smallest difference between two distinct merge heights (scipy linkage)
  margin_<n>        smallest |merge height - 0.5|
The nearest-neighbour chain breaks ties on exact values and the cut compares heights with the
threshold, so these inputs are only a yardstick while the three values are far above the 1e-15
a reordered K = 16 sum moves; the test asserts >= 1e-9 from the file.

Needs scikit-learn and scipy (written with 1.7.2 and 1.15.3); nothing else in the repository
does.  Run from the repository root: python tools/make_stream_pool_fallback_golden.py
"""

import os

import numpy as np
from scipy.cluster.hierarchy import linkage
from scipy.spatial.distance import pdist
from sklearn.cluster import AgglomerativeClustering

SIZES = (2, 3, 5, 33, 63, 64, 65, 96, 127, 128, 129)
D = 16
THRESHOLDS = (("t05", 0.5), ("t19", 1.9))


def conversation(seed, count, d=16, speakers=4, noise=0.02, run=5):
  rng = np.random.default_rng(seed)
  centres = np.linalg.qr(rng.standard_normal((d, speakers)))[0].T
  who = np.repeat(rng.integers(0, speakers, (count + run - 1) // run), run)[:count]
  return centres[who] + noise * rng.standard_normal((count, d))


def smallest_gap(values: np.ndarray) -> float:
  values = np.unique(values)
  return float(np.diff(values).min()) if values.size > 1 else float("inf")


def main():
  out = {}
  for n in SIZES:
    x = conversation(8000 + n, n, d=D, noise=0.25)
    out["rows_%d" % n] = x
    counts = []
    for tag, t in THRESHOLDS:
      labels = AgglomerativeClustering(n_clusters=None, metric="cosine", linkage="average",
                                       distance_threshold=t).fit_predict(x)
      out["labels_%d_%s" % (n, tag)] = labels.astype(np.int64)
      counts.append(int(labels.max()) + 1)
    dist = pdist(x, metric="cosine")
    heights = linkage(dist, method="average")[:, 2]
    out["min_gap_%d" % n] = np.array(smallest_gap(dist))
    out["height_gap_%d" % n] = np.array(smallest_gap(heights))
    out["margin_%d" % n] = np.array(np.abs(heights - 0.5).min())
    print("n = %3d: %2d / %d clusters, pair-distance gap %.2e, height gap %.2e, margin to 0.5 "
          "%.2e" % (n, counts[0], counts[1], out["min_gap_%d" % n], out["height_gap_%d" % n],
                    out["margin_%d" % n]))
  path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests",
                      "golden", "stream_pool_fallback.npz")
  np.savez_compressed(path, **out)
  print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
  main()
