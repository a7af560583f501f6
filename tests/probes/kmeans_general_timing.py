"""ms per call of the general k-means form (run_kmeans with dim != n_clusters ->
sc_stage_kmeans_general), upload of the (n, dim) input included, for the sizes DESIGN.md 3.7
quotes.  Run from the repo root on a GPU box:

    python tests/probes/kmeans_general_timing.py [--reps R] [--out FILE] [--only N,DIM,K,METRIC]

One JSON line per (n, dim, k, metric): median / min ms over R timed calls after two warm-up
calls, the distance passes the loop ran, and whether the labels equal the oracle's
(spectral_oracle.run_kmeans_metric, i.e. sklearn seeds + scipy cdist)."""

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import spectral_oracle as so  # noqa: E402
from spectralcluster_amd import _lib  # noqa: E402
from spectralcluster_amd import custom_distance_kmeans as ckm  # noqa: E402

SIZES = ((1000, 6, 4), (8192, 256, 20), (20000, 64, 10))


def passes(e, k, metric):
  h = _lib.default_handle()
  n, dim = e.shape
  lab = np.empty(n, dtype=np.int64)
  it = ctypes.c_int(0)
  h.check(h.lib.sc_stage_kmeans_general(h.raw, _lib.as_double_p(e), n, dim, k, 300,
                                        _lib.kmeans_metric_code(metric), 0.001, None,
                                        _lib.as_int64_p(lab), None, ctypes.byref(it)))
  return it.value


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=20)
  ap.add_argument("--out", default=None)
  ap.add_argument("--only", default=None, help="one case, e.g. 8192,256,20,cosine")
  args = ap.parse_args()
  lines = []
  cases = [(n, dim, k, m) for n, dim, k in SIZES for m in ("cosine", "euclidean")]
  if args.only:
    n, dim, k, m = args.only.split(",")
    cases = [(int(n), int(dim), int(k), m)]
  for n, dim, k, metric in cases:
    e = so.blobs(n, dim, k, seed=n + dim, noise=0.5)
    if True:
      for _ in range(2):
        got = ckm.run_kmeans(e, k, metric, 300)
      ts = []
      for _ in range(args.reps):
        t0 = time.perf_counter()
        ckm.run_kmeans(e, k, metric, 300)
        ts.append((time.perf_counter() - t0) * 1e3)
      rec = {"n": n, "dim": dim, "k": k, "metric": metric,
             "ms_median": round(float(np.median(ts)), 3), "ms_min": round(min(ts), 3),
             "reps": args.reps, "passes": passes(e, k, metric),
             "input_mb": round(n * dim * 8 / 1e6, 2),
             "labels_equal_oracle": bool(np.array_equal(got, so.run_kmeans_metric(e, k, 300,
                                                                                  metric)))}
      print(json.dumps(rec), flush=True)
      lines.append(json.dumps(rec))
  if args.out:
    with open(args.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
