#!/usr/bin/env python
"""Throughput of an AutoTune batch: the Turn-to-Diarize preset (AutoTune 0.40-0.95, step 0.05,
one level; Percentile threshold, GraphCut, ConstraintPropagation alpha = 0.4 before refinement),
every utterance with the `ConstraintMatrix` of its speaker-turn scores.

Two compositions of 512 synthetic conversations (oracle turn_blobs, fixed seeds, d = 256):
  short  n uniform in [20, 128]    (route 2: waves of (utterance, p) pairs, dense Jacobi solves)
  long   n uniform in [300, 3000]  (route 1: three lanes, every level a lockstep Lanczos group)
Per composition, after a warm-up on the first 64 utterances, utterances/s of
`predict_batch(us, constraint_matrices=cs, autotune_from_entry_state=True)` (best of --repeat).
A tree without that keyword runs the same request as its per-utterance loop, each utterance on a
fresh copy of the AutoTune object: run this file with --root pointing at that tree for the
yardstick.  One JSON line per composition on stdout; --out appends them to a file.

  python tools/autotune_batch_probe.py [--count 512] [--repeat 1] [--only short|long]
                                       [--root TREE] [--out FILE] [--tag NAME]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

WORKLOADS = {"short": (20, 128, 2018), "long": (300, 3000, 512)}


def conversations(so, sca, name, count):
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


def run_batch(clusterer, us, cs):
  """The one request on either tree -> (best_p per utterance, form)."""
  try:
    clusterer.predict_batch(us, constraint_matrices=cs, autotune_from_entry_state=True)
    return list(clusterer.last_batch_best_p), "predict_batch"
  except TypeError as exc:
    if "autotune_from_entry_state" not in str(exc):
      raise
  entry = clusterer.autotune
  best = []
  try:
    for u, c in zip(us, cs):
      clusterer.autotune = copy.deepcopy(entry)
      clusterer.predict(u, c)
      best.append(clusterer.last_best_p)
  finally:
    clusterer.autotune = entry
  return best, "loop"


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--count", type=int, default=512)
  ap.add_argument("--repeat", type=int, default=1)
  ap.add_argument("--only", choices=sorted(WORKLOADS), default=None)
  ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  ap.add_argument("--out", default=None)
  ap.add_argument("--tag", default="")
  args = ap.parse_args()
  root = os.path.abspath(args.root)
  sys.path.insert(0, root)
  sys.path.insert(0, os.path.join(root, "oracle"))
  import spectral_oracle as so
  import spectralcluster_amd as sca
  for name in ([args.only] if args.only else ["short", "long"]):
    us, cs = conversations(so, sca, name, args.count)
    c = copy.deepcopy(sca.configs.turntodiarize_clusterer)
    run_batch(c, us[:64], cs[:64])  # warm-up: arenas, streams, pinned staging
    best, form, best_p = 0.0, "", []
    for _ in range(args.repeat):
      t0 = time.perf_counter()
      best_p, form = run_batch(c, us, cs)
      best = max(best, len(us) / (time.perf_counter() - t0))
    rec = {"tag": args.tag, "workload": name, "utterances": len(us),
           "n": list(WORKLOADS[name][:2]), "d": 256, "repeat": args.repeat, "form": form,
           "utt_per_s": round(best, 1),
           "routes": ({str(r): c.last_batch_routes.count(r) for r in sorted(set(c.last_batch_routes))}
                      if form == "predict_batch" else {"0": len(us)}),
           # (the same winners on either tree: a checksum of the searches' results)
           "best_p_sum": round(float(np.sum(best_p)), 6)}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
      with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
  main()
