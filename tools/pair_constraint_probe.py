#!/usr/bin/env python
"""Must-link / cannot-link pairs as `PairwiseConstraints` against the same constraints as a dense
(n, n) matrix on the parent commit, in alternating fresh processes.

Legs (Turn-to-Diarize refinement at p_percentile = 0.9, GraphCut Laplacian, ConstraintPropagation
alpha = 0.4 before refinement, d = 256, oracle turn_blobs with fixed seeds):
  a  predict(x, c) at n = 4096 and n = 8192, 16 random must / cannot pairs: seconds per call
  b  predict_batch of --count utterances, n uniform in [300, 3000], 8 pairs each: utterances/s
     (on the parent the dense matrices send the batch to the per-utterance loop)
  c  the untouched path: tools/constrained_batch_probe.py's band-only config5 batch
The driver runs --pairs processes of this tree alternating with as many of the tree at --parent
(a checkout of the parent commit with its library built), where the constraints are passed as
the dense matrix; one JSON line per process and leg, appended to --out.

  python tools/pair_constraint_probe.py --parent DIR [--pairs 6] [--legs abc] [--count 512]
                                        [--out profiles/pair_constraint_probe.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pair_list(n, pairs, seed):
  """`pairs` distinct unordered pairs {i, j}, i != j, must-link / cannot-link alternating."""
  rng = np.random.default_rng(seed)
  seen = set()
  while len(seen) < pairs:
    i, j = sorted(int(v) for v in rng.integers(0, n, size=2))
    if i != j:
      seen.add((i, j))
  ordered = sorted(seen)
  return ordered[0::2], ordered[1::2]


def constraint(sca, n, pairs, seed, dense):
  must, cannot = pair_list(n, pairs, seed)
  if not dense:
    return sca.PairwiseConstraints(n, must_link=must, cannot_link=cannot)
  q = np.zeros((n, n))
  for (i, j) in must:
    q[i, j] = q[j, i] = 1.0
  for (i, j) in cannot:
    q[i, j] = q[j, i] = -1.0
  return q


def child(args):
  sys.path.insert(0, args.tree)
  sys.path.insert(0, os.path.join(args.tree, "oracle"))
  import spectral_oracle as so
  import spectralcluster_amd as sca
  sys.path.insert(0, os.path.join(args.tree, "tools"))
  import constrained_batch_probe as band_probe
  rec = {"tag": args.tag, "leg": args.leg, "dense": bool(args.dense)}
  if args.leg == "a":
    for n in (4096, 8192):
      x, _, _ = so.turn_blobs(n, 256, 6, seed=n, noise=0.8)
      c = constraint(sca, n, 16, n, args.dense)
      clusterer = band_probe.clusterer()
      clusterer.predict(x, c)  # warm-up: buffers, tile maps
      best = float("inf")
      for _ in range(3):
        t0 = time.perf_counter()
        clusterer.predict(x, c)
        best = min(best, time.perf_counter() - t0)
      rec["predict_s_n%d" % n] = round(best, 5)
  elif args.leg == "b":
    rng = np.random.default_rng(512)
    ns = rng.integers(300, 3001, 512)[:args.count]
    us = [so.turn_blobs(int(n), 256, 4, seed=70000 + i, noise=0.8)[0] for i, n in enumerate(ns)]
    cs = [constraint(sca, int(n), 8, 900 + i, args.dense) for i, n in enumerate(ns)]
    clusterer = band_probe.clusterer()
    clusterer.predict_batch(us, constraint_matrices=cs)  # warm-up
    t0 = time.perf_counter()
    clusterer.predict_batch(us, constraint_matrices=cs)
    rec["utterances"] = len(us)
    rec["utt_per_s"] = round(len(us) / (time.perf_counter() - t0), 1)
    routes = clusterer.last_batch_routes
    rec["routes"] = {str(r): routes.count(r) for r in sorted(set(routes))}
  else:
    us, cs = band_probe.conversations("config5", args.count)
    clusterer = band_probe.clusterer()
    clusterer.predict_batch(us, constraint_matrices=cs)
    t0 = time.perf_counter()
    clusterer.predict_batch(us, constraint_matrices=cs)
    rec["utterances"] = len(us)
    rec["utt_per_s"] = round(len(us) / (time.perf_counter() - t0), 1)
  line = json.dumps(rec)
  print(line, flush=True)
  if args.out:
    with open(args.out, "a") as f:
      f.write(line + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--parent", default=None, help="checkout of the parent commit, library built")
  ap.add_argument("--pairs", type=int, default=6)
  ap.add_argument("--legs", default="abc")
  ap.add_argument("--count", type=int, default=512)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_constraint_probe.jsonl"))
  ap.add_argument("--leg", default=None, help="(child) one leg in this process")
  ap.add_argument("--tree", default=ROOT)
  ap.add_argument("--dense", type=int, default=0)
  ap.add_argument("--tag", default="")
  args = ap.parse_args()
  if args.leg:
    return child(args)
  for leg in args.legs:
    for i in range(args.pairs):
      for tag, tree, dense in (("this", ROOT, 0), ("parent", args.parent, 1)):
        if tree is None:
          continue
        # leg c is the band-only batch on both trees: nothing to densify
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--tree", tree,
               "--dense", str(dense if leg != "c" else 0), "--count", str(args.count),
               "--out", args.out, "--tag", "%s%d" % (tag, i)]
        # (a failed or hung process ends the probe: nothing more is started on the device)
        subprocess.run(cmd, check=True, timeout=900)


if __name__ == "__main__":
  main()
