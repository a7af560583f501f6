"""Generate tests/golden/kmeans_dim.npz by running the REAL reference's k-means module on
embeddings whose width differs from the cluster count.

CPU only; needs the reference package on sys.path (as oracle/make_golden.py does):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_kmeans_dim_golden.py --reference DIR

where DIR holds the reference's `spectralcluster` package.

Inputs (all stored in the file):
  a  1000 x 6, k = 4: the reference test's 400/300/200/100 layout + seeded noise
     (tests/custom_distance_kmeans_test.py:46-72 of the reference)
  b  500 x 12, k = 5
  c  300 x 3, k = 6 (dim < k)
  d  1000 x 144, k = 8, float32-exact values (128 < dim: numpy's pairwise row mean in the
     correlation metric), cast to float64 before the reference sees it
Records:
  labels_<tag>_<metric>          run_kmeans(e, k, metric, 300)
  ck_<tag>_<metric>_labels/_cent CustomKMeans(k, init copy, custom_dist=metric).predict(e) with
                                 the stored init_<tag>; the centroids the reference leaves in
                                 the array; ck_<tag>_cosine_tol02_* at tol = 0.2
  none_<i>_*                     CustomKMeans(centroids=None) after np.random.seed(seed): the
                                 exception name ("" when it returns), the labels when it
                                 returns, the next np.random.rand()
"""

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.dont_write_bytecode = True

DEVICE_METRICS = ("cosine", "euclidean", "sqeuclidean", "cityblock", "chebyshev",
                  "correlation", "braycurtis", "canberra")
RUN_METRICS = DEVICE_METRICS + ("minkowski",)
WIDE_METRICS = ("cosine", "euclidean", "correlation")
K = {"a": 4, "b": 5, "c": 6, "d": 8}
NONE_SEEDS = (0, 1, 2)


def inputs():
  """The four inputs and the initial centroids of the CustomKMeans cases."""
  e = {}
  layout = np.array([[1.0, 0.0, 0.0, 0.0, 0.0, 0.0]] * 400 +
                    [[0.0, 1.0, 0.0, 0.0, 0.0, 0.0]] * 300 +
                    [[0.0, 0.0, 2.0, 0.0, 0.0, 0.0]] * 200 +
                    [[0.0, 0.0, 0.0, 1.0, 0.0, 0.0]] * 100)
  e["a"] = layout + (np.random.RandomState(7).rand(1000, 6) * 2 - 1) * 0.1
  rng = np.random.default_rng(21)
  cent = rng.standard_normal((5, 12))
  e["b"] = cent[rng.integers(0, 5, 500)] + 0.4 * rng.standard_normal((500, 12))
  rng = np.random.default_rng(22)
  cent = rng.standard_normal((6, 3)) * 2.0
  e["c"] = cent[rng.integers(0, 6, 300)] + 0.5 * rng.standard_normal((300, 3))
  rng = np.random.default_rng(23)
  cent = rng.standard_normal((8, 144))
  d = cent[rng.integers(0, 8, 1000)] * 0.6 + 0.35 * rng.standard_normal((1000, 144))
  e["d"] = d.astype(np.float32)
  init = {}
  for tag, seed in (("a", 31), ("b", 32)):
    r = np.random.default_rng(seed)
    rows = r.choice(e[tag].shape[0], size=K[tag], replace=False)
    init[tag] = e[tag][rows] + 0.05 * r.standard_normal((K[tag], e[tag].shape[1]))
  return e, init


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reference", required=True,
                  help="directory that holds the reference's spectralcluster package")
  args = ap.parse_args()
  sys.path.insert(0, args.reference)
  from spectralcluster import custom_distance_kmeans as ref  # pylint: disable=import-outside-toplevel

  e, init = inputs()
  out = {"e_" + t: v for t, v in e.items()}
  out.update({"init_" + t: v for t, v in init.items()})
  for tag in "abcd":
    x = e[tag].astype(np.float64)
    for metric in (WIDE_METRICS if tag == "d" else RUN_METRICS):
      out["labels_%s_%s" % (tag, metric)] = ref.run_kmeans(x, K[tag], metric, 300).astype(
          np.int16)
  for tag in "ab":
    for metric in RUN_METRICS:
      c = init[tag].copy()
      lab = ref.CustomKMeans(n_clusters=K[tag], centroids=c, custom_dist=metric).predict(e[tag])
      out["ck_%s_%s_labels" % (tag, metric)] = lab.astype(np.int16)
      out["ck_%s_%s_cent" % (tag, metric)] = c
    c = init[tag].copy()
    lab = ref.CustomKMeans(n_clusters=K[tag], centroids=c, tol=0.2).predict(e[tag])
    out["ck_%s_cosine_tol02_labels" % tag] = lab.astype(np.int16)
    out["ck_%s_cosine_tol02_cent" % tag] = c
  # centroids=None: random rows; the reference's first update raises UnboundLocalError
  # (n_centroids is bound only on the given-centroids branch) ...
  cases = [(e["a"], 4, "cosine", s) for s in NONE_SEEDS]
  # ... and returns when the rule stops the loop after the first pass: n == k distinct rows,
  # euclidean, every row its own centroid (mean distance 0)
  out["e_r"] = np.random.default_rng(24).standard_normal((5, 3))
  cases.append((out["e_r"], 5, "euclidean", 3))
  for i, (x, k, metric, seed) in enumerate(cases):
    np.random.seed(seed)
    exc, lab = "", np.zeros(0, dtype=np.int16)
    try:
      lab = ref.CustomKMeans(n_clusters=k, custom_dist=metric).predict(x).astype(np.int16)
    except Exception as err:  # pylint: disable=broad-except
      exc = type(err).__name__
    out["none_%d_exc" % i] = np.array(exc)
    out["none_%d_labels" % i] = lab
    out["none_%d_next_rand" % i] = np.array(np.random.rand())
    out["none_%d_case" % i] = np.array("%s,%d,%s,%d" % ("r" if x is out["e_r"] else "a", k,
                                                         metric, seed))
  path = os.path.join(ROOT, "tests", "golden", "kmeans_dim.npz")
  np.savez_compressed(path, **out)
  print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
  main()
