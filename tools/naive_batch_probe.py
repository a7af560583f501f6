#!/usr/bin/env python
"""Throughput of the batches that meet the Naive fallback type -- what a default FallbackOptions
selects -- with `predict_batch(..., batch_naive_fallback=True)`, against the same batches with the
Agglomerative type and no new flag (the untouched legs).

512 synthetic utterances per leg (Gaussian blobs, fixed seeds, d = 256), the ICASSP2018 options,
max_clusters = 7, the default FallbackOptions thresholds (0.5):
  reduced         n uniform in [20, 400], spectral_min_embeddings = 100, max_spectral_size = 128
                  (the `fallback` composition of tools/reduced_batch_probe.py)
  single_short    n uniform in [20, 128], min_clusters = 1, the FallbackClusterer condition, every
                  fourth utterance one speaker (tools/fallback_condition_batch_probe.py `short`)
  single_config5  n uniform in [300, 3000], otherwise the same (its `config5`)
Each composition runs twice: `type` naive with every batch flag the tree knows, and `type`
agglomerative with the flags the parent of `batch_naive_fallback` knows.  Per leg, after one untimed
run of the whole batch, utterances/s of every one of --repeat runs.  A tree from before the flag
runs the naive legs as its per-utterance loop: run this file with --root pointing at that tree for
the yardstick (`form` says which ran).  One JSON line per leg on stdout; --out appends them.

  python tools/naive_batch_probe.py [--count 512] [--repeat 1] [--only LEG] [--type naive|agglomerative]
                                    [--root TREE] [--out FILE] [--tag NAME]
"""
import argparse
import inspect
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _inputs  # noqa: E402

LEGS = ("reduced", "single_short", "single_config5")


def utterances(leg, count):
  if leg == "reduced":
    rng = np.random.default_rng(3015)
    ns, ks = rng.integers(20, 401, 512), rng.integers(2, 7, 512)
    seeds = [90000 + i for i in range(512)]
  elif leg == "single_short":
    rng = np.random.default_rng(2018)
    ns, ks = rng.integers(20, 129, 512), rng.integers(2, 7, 512)
    seeds = [50000 + i for i in range(512)]
  else:
    rng = np.random.default_rng(512)
    ns, ks = rng.integers(300, 3001, 512), rng.integers(2, 8, 512)
    seeds = list(range(512))
  if leg != "reduced":
    ks[::4] = 1
  return [_inputs.blobs(int(n), 256, int(k), seed=s) for n, k, s in list(zip(ns, ks, seeds))[:count]]


def clusterer(sca, leg, kind):
  fallback_type = (sca.FallbackClustererType.Naive if kind == "naive"
                   else sca.FallbackClustererType.Agglomerative)
  kwargs = dict(max_clusters=7, refinement_options=sca.configs.icassp2018_refinement_options)
  if leg == "reduced":
    return sca.SpectralClusterer(
        min_clusters=2, max_spectral_size=128,
        fallback_options=sca.FallbackOptions(spectral_min_embeddings=100,
                                             fallback_clusterer_type=fallback_type), **kwargs)
  return sca.SpectralClusterer(
      min_clusters=1,
      fallback_options=sca.FallbackOptions(
          single_cluster_condition=sca.SingleClusterCondition.FallbackClusterer,
          fallback_clusterer_type=fallback_type), **kwargs)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--count", type=int, default=512)
  ap.add_argument("--repeat", type=int, default=1)
  ap.add_argument("--only", choices=LEGS, default=None)
  ap.add_argument("--type", choices=("naive", "agglomerative"), default=None)
  ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  ap.add_argument("--out", default=None)
  ap.add_argument("--tag", default="")
  args = ap.parse_args()
  sys.path.insert(0, os.path.abspath(args.root))
  import spectralcluster_amd as sca
  known = inspect.signature(sca.SpectralClusterer.predict_batch).parameters
  for leg in ([args.only] if args.only else LEGS):
    us = utterances(leg, args.count)
    for kind in ([args.type] if args.type else ("naive", "agglomerative")):
      flags = {}
      if leg != "reduced" and "batch_fallback_condition" in known:
        flags["batch_fallback_condition"] = True
      if kind == "naive" and "batch_naive_fallback" in known:
        flags["batch_naive_fallback"] = True
      c = clusterer(sca, leg, kind)
      c.predict_batch(us, **flags)  # untimed: arenas, streams, pinned staging
      rates, labels = [], []
      for _ in range(args.repeat):
        t0 = time.perf_counter()
        labels = c.predict_batch(us, **flags)
        rates.append(round(len(us) / (time.perf_counter() - t0), 1))
      routes = c.last_batch_routes
      single = getattr(c, "last_batch_single", None)
      rec = {"tag": args.tag, "leg": leg, "type": kind, "utterances": len(us), "d": 256,
             "flags": sorted(flags), "form": "loop" if set(routes) == {0} else "library",
             "utt_per_s": rates,
             "routes": {str(r): routes.count(r) for r in sorted(set(routes))},
             "single": None if single is None else int(sum(single)),
             # (the same clusters on either tree: a checksum of the results)
             "clusters_sum": int(sum(np.unique(l).size for l in labels))}
      line = json.dumps(rec)
      print(line, flush=True)
      if args.out:
        with open(args.out, "a") as f:
          f.write(line + "\n")


if __name__ == "__main__":
  main()
