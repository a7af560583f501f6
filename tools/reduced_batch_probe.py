#!/usr/bin/env python
"""Throughput of a batch whose clusterer sets `max_spectral_size` and / or
`fallback_options.spectral_min_embeddings` (the options a production diarization clusterer sets).

Two compositions of 512 synthetic utterances (Gaussian blobs, fixed seeds, d = 256), the
ICASSP2018 options with min_clusters = 2, max_clusters = 7:
  reduce    n uniform in [300, 3000], max_spectral_size = 256: every utterance is pre-clustered
            (complete linkage) and its 256 centroids take the spectral path
  fallback  n uniform in [20, 400], spectral_min_embeddings = 100, max_spectral_size = 128 and
            the agglomerative fallback: about a fifth are fallback members, the ones above 128
            rows are pre-clustered, the rest are clustered as they are
Per composition, after a warm-up on the first 32 utterances, utterances/s of
`predict_batch(utterances)` (best of --repeat).  A tree from before `sc_predict_batch_reduced`
runs the same call as its per-utterance loop: run this file with --root pointing at that tree for
the yardstick (`form` says which ran).  One JSON line per composition on stdout; --out appends them
to a file.

  python tools/reduced_batch_probe.py [--count 512] [--repeat 1] [--only reduce|fallback]
                                      [--root TREE] [--out FILE] [--tag NAME]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _inputs  # noqa: E402

WORKLOADS = {"reduce": (300, 3000, 3014), "fallback": (20, 400, 3015)}


def utterances(name, count):
  lo, hi, seed = WORKLOADS[name]
  rng = np.random.default_rng(seed)
  ns = rng.integers(lo, hi + 1, 512)[:count]
  ks = rng.integers(2, 7, 512)[:count]
  return [_inputs.blobs(int(n), 256, int(k), seed=90000 + i) for i, (n, k) in enumerate(zip(ns, ks))]


def clusterer(sca, name):
  kwargs = dict(min_clusters=2, max_clusters=7,
                refinement_options=sca.configs.icassp2018_refinement_options)
  if name == "reduce":
    return sca.SpectralClusterer(max_spectral_size=256, **kwargs)
  return sca.SpectralClusterer(
      max_spectral_size=128,
      fallback_options=sca.FallbackOptions(
          spectral_min_embeddings=100,
          fallback_clusterer_type=sca.FallbackClustererType.Agglomerative), **kwargs)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--count", type=int, default=512)
  ap.add_argument("--repeat", type=int, default=1)
  ap.add_argument("--only", choices=sorted(WORKLOADS), default=None)
  ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  ap.add_argument("--out", default=None)
  ap.add_argument("--tag", default="")
  args = ap.parse_args()
  sys.path.insert(0, os.path.abspath(args.root))
  import spectralcluster_amd as sca
  for name in ([args.only] if args.only else ["reduce", "fallback"]):
    us = utterances(name, args.count)
    c = clusterer(sca, name)
    c.predict_batch(us[:32])  # warm-up: arenas, streams, pinned staging
    best, labels = 0.0, []
    for _ in range(args.repeat):
      c.last_batch_reduced = None
      t0 = time.perf_counter()
      labels = c.predict_batch(us)
      best = max(best, len(us) / (time.perf_counter() - t0))
    kinds = getattr(c, "last_batch_reduced", None)
    routes = c.last_batch_routes
    rec = {"tag": args.tag, "workload": name, "utterances": len(us),
           "n": list(WORKLOADS[name][:2]), "d": 256, "repeat": args.repeat,
           "form": "sc_predict_batch_reduced" if kinds is not None else "loop",
           "utt_per_s": round(best, 1),
           "kinds": {str(k): kinds.count(k) for k in sorted(set(kinds))} if kinds else None,
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
