#!/usr/bin/env python
"""Throughput of a batch whose clusterer has min_clusters = 1 (the streaming / multi-stage
regime: the clusterer may say "one speaker"), against the same batch with min_clusters = 2.

Two compositions of 512 synthetic utterances (Gaussian blobs, fixed seeds, d = 256), the
ICASSP2018 options, max_clusters = 7, the default AffinityGmmBic condition:
  short    n uniform in [20, 128]: the mix of tools/short_batch_probe.py (the short route)
  config5  n uniform in [300, 3000]: BASELINE config 5 (the grouped block Lanczos route)
Per composition and min_clusters, after one untimed run of the whole batch, utterances/s of
`predict_batch(utterances)` for every one of --repeat runs (the spread is the point: compare the
slowest run of one tree with the fastest of another).  A tree from before
`sc_predict_batch_single` runs the min_clusters = 1 call as its per-utterance loop: run this file
with --root pointing at that tree for the yardstick (`form` says which ran).  One JSON line per
composition and min_clusters on stdout; --out appends them to a file.

  python tools/single_check_batch_probe.py [--count 512] [--repeat 6] [--only short|config5]
                                           [--min-clusters 1|2] [--root TREE] [--out FILE]
                                           [--tag NAME]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _inputs  # noqa: E402


def utterances(name, count):
  if name == "short":
    rng = np.random.default_rng(2018)
    ns, ks = rng.integers(20, 129, 512), rng.integers(2, 7, 512)
    seeds = [50000 + i for i in range(512)]
  else:
    rng = np.random.default_rng(512)
    ns, ks = rng.integers(300, 3001, 512), rng.integers(2, 8, 512)
    seeds = list(range(512))
  return [_inputs.blobs(int(n), 256, int(k), seed=s)
          for n, k, s in list(zip(ns, ks, seeds))[:count]]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--count", type=int, default=512)
  ap.add_argument("--repeat", type=int, default=6)
  ap.add_argument("--only", choices=["short", "config5"], default=None)
  ap.add_argument("--min-clusters", type=int, choices=[1, 2], default=None)
  ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  ap.add_argument("--out", default=None)
  ap.add_argument("--tag", default="")
  args = ap.parse_args()
  sys.path.insert(0, os.path.abspath(args.root))
  import spectralcluster_amd as sca
  for name in ([args.only] if args.only else ["short", "config5"]):
    us = utterances(name, args.count)
    for min_clusters in ([args.min_clusters] if args.min_clusters else [1, 2]):
      c = sca.SpectralClusterer(min_clusters=min_clusters, max_clusters=7,
                                refinement_options=sca.configs.icassp2018_refinement_options)
      # warm-up: the whole batch once -- lanes, streams, arenas and pinned staging are created
      # by the first batch that needs them, and a batch of 32 needs fewer than one of 512
      c.predict_batch(us)
      rates, labels = [], []
      for _ in range(args.repeat):
        t0 = time.perf_counter()
        labels = c.predict_batch(us)
        rates.append(round(len(us) / (time.perf_counter() - t0), 1))
      single = getattr(c, "last_batch_single", None)
      routes = c.last_batch_routes
      rec = {"tag": args.tag, "workload": name, "min_clusters": min_clusters,
             "utterances": len(us), "d": 256,
             "form": ("sc_predict_batch_single" if single is not None else
                      "loop" if min_clusters == 1 else "sc_predict_batch_grouped"),
             "utt_per_s": rates, "slowest": min(rates), "fastest": max(rates),
             "single": None if single is None else int(sum(single)),
             "routes": {str(r): routes.count(r) for r in sorted(set(routes))},
             # (the same clusters on either tree: a checksum of the results)
             "clusters_sum": int(sum(np.unique(l).size for l in labels))}
      line = json.dumps(rec)
      print(line, flush=True)
      if args.out:
        with open(args.out, "a") as f:
          f.write(line + "\n")


if __name__ == "__main__":
  main()
