#!/usr/bin/env python3
"""Writes tests/golden/stream_pool_ahc.npz: the rows and sklearn's own labels for the sizes
at which the pooled pre-clusterer is tested (tests/test_gpu_stream_pool.py).

  rows_<n>     (n, 16) float64, seeded standard-normal rows
  labels_<n>   AgglomerativeClustering(n_clusters=24, metric="cosine",
               linkage="complete").fit_predict(rows_<n>)
  min_gap_<n>  smallest difference between two distinct pair distances (scipy pdist): the
               nearest-neighbour chain breaks ties on exact values, so these inputs are only
               useful while that gap is far above the 1e-15 a reordered K = 16 sum moves

Needs scikit-learn and scipy (written with 1.7.2 and 1.15.3); nothing else in the repository
does.  Run from the repository root: python tools/make_stream_pool_golden.py
"""

import os

import numpy as np
from scipy.spatial.distance import pdist
from sklearn.cluster import AgglomerativeClustering

SIZES = (25, 63, 64, 65, 129, 1025)
D = 16
N_CLUSTERS = 24


def rows_for(n: int) -> np.ndarray:
  return np.random.default_rng(7000 + n).standard_normal((n, D))


def main():
  out = {}
  for n in SIZES:
    x = rows_for(n)
    labels = AgglomerativeClustering(n_clusters=N_CLUSTERS, metric="cosine",
                                     linkage="complete").fit_predict(x)
    dist = np.unique(pdist(x, metric="cosine"))
    out["rows_%d" % n] = x
    out["labels_%d" % n] = labels.astype(np.int64)
    out["min_gap_%d" % n] = np.array(np.diff(dist).min())
    print("n = %4d: %d clusters, smallest gap between pair distances %.2e"
          % (n, labels.max() + 1, out["min_gap_%d" % n]))
  path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests",
                      "golden", "stream_pool_ahc.npz")
  np.savez_compressed(path, **out)
  print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
  main()
