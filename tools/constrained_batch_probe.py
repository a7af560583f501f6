#!/usr/bin/env python
"""Throughput of a batch in which every utterance carries speaker-turn constraints.

Two workloads of 512 synthetic conversations (oracle turn_blobs, fixed seeds, d = 256), each
utterance with the `ConstraintMatrix` of its turn scores:
  config5  n uniform in [300, 3000] (SURVEY.md's config 5 sizes: the grouped block Lanczos route)
  short    n uniform in [20, 128] (the short route: one Jacobi workgroup per utterance)
under the Turn-to-Diarize refinement at p_percentile = 0.9 with a GraphCut Laplacian and
ConstraintPropagation (alpha = 0.4) before refinement.  Per workload, after a warm-up batch,
utterances/s of `predict_batch(us, constraint_matrices=cs)` (best of --repeat) and how many
utterances took which route.  A build without the constrained batch runs the same call as its
per-utterance loop (every route 0): run this file from that tree for the yardstick.  One JSON
line per workload on stdout; --out appends them to a file.

  python tools/constrained_batch_probe.py [--count 512] [--repeat 2] [--only config5|short]
                                          [--out FILE] [--tag NAME]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import spectral_oracle as so  # noqa: E402
import spectralcluster_amd as sca  # noqa: E402

WORKLOADS = {"config5": (300, 3000, 512), "short": (20, 128, 2018)}


def conversations(name, count):
  lo, hi, seed = WORKLOADS[name]
  rng = np.random.default_rng(seed)
  ns = rng.integers(lo, hi + 1, 512)[:count]
  ks = rng.integers(2, 7, 512)[:count]
  us, cs = [], []
  for i, (n, k) in enumerate(zip(ns, ks)):
    x, _, scores = so.turn_blobs(int(n), 256, int(k), seed=70000 + i, noise=0.8)
    us.append(x)
    cs.append(sca.ConstraintMatrix(list(scores), 1))
  return us, cs


def clusterer():
  options = sca.RefinementOptions(
      p_percentile=0.9, thresholding_type=sca.ThresholdType.Percentile,
      thresholding_with_binarization=True, thresholding_preserve_diagonal=True,
      symmetrize_type=sca.SymmetrizeType.Average,
      refinement_sequence=sca.TURNTODIARIZE_REFINEMENT_SEQUENCE)
  return sca.SpectralClusterer(
      min_clusters=2, max_clusters=7, refinement_options=options,
      laplacian_type=sca.LaplacianType.GraphCut, row_wise_renorm=True,
      constraint_options=sca.ConstraintOptions(
          constraint_name=sca.ConstraintName.ConstraintPropagation,
          apply_before_refinement=True, constraint_propagation_alpha=0.4))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--count", type=int, default=512)
  ap.add_argument("--repeat", type=int, default=2)
  ap.add_argument("--only", choices=sorted(WORKLOADS), default=None)
  ap.add_argument("--out", default=None)
  ap.add_argument("--tag", default="")
  args = ap.parse_args()
  for name in ([args.only] if args.only else ["config5", "short"]):
    us, cs = conversations(name, args.count)
    c = clusterer()
    c.predict_batch(us, constraint_matrices=cs)  # warm-up: arenas, streams, pinned staging
    best = 0.0
    for _ in range(args.repeat):
      t0 = time.perf_counter()
      c.predict_batch(us, constraint_matrices=cs)
      best = max(best, len(us) / (time.perf_counter() - t0))
    routes = c.last_batch_routes
    rec = {"tag": args.tag, "workload": name, "utterances": len(us),
           "n": list(WORKLOADS[name][:2]), "d": 256, "repeat": args.repeat,
           "utt_per_s": round(best, 1),
           "routes": {str(r): routes.count(r) for r in sorted(set(routes))}}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
      with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
  main()
