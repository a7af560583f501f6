"""What the banded constraint saves: host-clock ms per call of the Turn-to-Diarize preset with
the constraint given (a) as the dense ndarray of `compute_diagonals()` -- built INSIDE the timed
call, because that is what a caller pays -- and (b) as the `ConstraintMatrix` itself (its band
travels).  The same two for `ConstraintPropagation.adjust_affinity` alone.  Run from the repo
root on a GPU box:

    python tests/probes/constraint_band_timing.py [--sizes 1200,4096,8192] [--pairs 20]
        [--out FILE] [--legs predict,adjust]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- \\
        python tests/probes/constraint_band_timing.py --band-only 4096
    python tools/rocprof_summary.py DIR/.../run_results.db

Both shapes are warmed first; then (a) and (b) alternate in one process, `--pairs` times.  One
JSON line per (n, leg): median, quartiles, min and max of each form, "spread" = the
interquartile range, and `band_below_dense_by_more_than_spread`.  Every call ends in a download
(labels / the adjusted matrix), so the host clock sees the whole call.  `--band-only N`: three
band calls of each leg at one size and nothing else (the process to put under rocprofv3)."""

import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import spectral_oracle as so  # noqa: E402
import spectralcluster_amd as sca  # noqa: E402
from spectralcluster_amd import constraint as con  # noqa: E402

ALPHA = 0.4  # the preset's constraint_propagation_alpha


def stats(ts):
  ts = np.asarray(ts)
  q25, q50, q75 = np.percentile(ts, [25, 50, 75])
  return {"median_ms": round(float(q50), 3), "q25_ms": round(float(q25), 3),
          "q75_ms": round(float(q75), 3), "min_ms": round(float(ts.min()), 3),
          "max_ms": round(float(ts.max()), 3), "spread_ms": round(float(q75 - q25), 3)}


def timed(fn):
  t0 = time.perf_counter()
  out = fn()
  return (time.perf_counter() - t0) * 1e3, out


def legs_for(n):
  x, _, scores = so.turn_blobs(n, 32, 4, seed=n, noise=0.6)
  scores = list(scores)
  a = so.affinity(x)
  op = con.ConstraintPropagation(ALPHA)

  def preset():
    # a fresh copy per call: AutoTune leaves its last p_percentile in the clusterer
    return copy.deepcopy(sca.configs.turntodiarize_clusterer)

  return {
      "predict": (
          lambda: preset().predict(x, sca.ConstraintMatrix(scores, 1).compute_diagonals()),
          lambda: preset().predict(x, sca.ConstraintMatrix(scores, 1))),
      "adjust": (
          lambda: op.adjust_affinity(a, sca.ConstraintMatrix(scores, 1).compute_diagonals()),
          lambda: op.adjust_affinity(a, sca.ConstraintMatrix(scores, 1))),
  }, scores


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--sizes", default="1200,4096,8192")
  ap.add_argument("--pairs", type=int, default=20)
  ap.add_argument("--legs", default="predict,adjust")
  ap.add_argument("--out", default=None)
  ap.add_argument("--band-only", type=int, default=0)
  args = ap.parse_args()
  if args.band_only:
    legs, _ = legs_for(args.band_only)
    for name in ("adjust", "predict"):
      for _ in range(3):
        legs[name][1]()
    return
  lines = []
  for n in [int(v) for v in args.sizes.split(",")]:
    legs, scores = legs_for(n)
    build_ms = [timed(lambda: sca.ConstraintMatrix(scores, 1).compute_diagonals())[0]
                for _ in range(5)]
    for name in args.legs.split(","):
      dense, band = legs[name]
      for _ in range(2):  # warm both shapes (buffers, code objects, the dense (n, ld) buffer)
        out_dense, out_band = dense(), band()
      td, tb = [], []
      for _ in range(args.pairs):
        td.append(timed(dense)[0])
        tb.append(timed(band)[0])
      sd, sb = stats(td), stats(tb)
      rec = {"n": n, "leg": name, "pairs": args.pairs, "dense": sd, "band": sb,
             "gain_ms": round(sd["median_ms"] - sb["median_ms"], 3),
             "band_below_dense_by_more_than_spread":
                 bool(sd["median_ms"] - sb["median_ms"] > max(sd["spread_ms"], sb["spread_ms"])),
             "band_below_dense_by_more_than_range":
                 bool(sd["median_ms"] - sb["median_ms"] >
                      max(sd["max_ms"] - sd["min_ms"], sb["max_ms"] - sb["min_ms"])),
             "compute_diagonals_ms_median": round(float(np.median(build_ms)), 3),
             "dense_constraint_mb": round(n * n * 8 / 1e6, 1),
             "results_equal": bool(np.array_equal(out_dense, out_band))}
      print(json.dumps(rec), flush=True)
      lines.append(json.dumps(rec))
  if args.out:
    with open(args.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
