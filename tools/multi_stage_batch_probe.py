#!/usr/bin/env python
"""Throughput of a batch whose clusterer sets the three options of a robust offline diarizer
together: `fallback_options.spectral_min_embeddings`, `max_spectral_size` and `min_clusters=1`.

Two compositions of 512 synthetic utterances (Gaussian blobs, fixed seeds, d = 256; every fourth
utterance holds ONE speaker, the others 2 .. 6), the ICASSP2018 options, max_clusters = 7, the
agglomerative fallback type with threshold 0.5:
  mixed   n uniform in [20, 400], spectral_min_embeddings = 100, max_spectral_size = 128: about a
          fifth are fallback members, the ones above 128 rows are pre-clustered and their
          centroids tested, the rest are tested and clustered as they are
  reduce  n uniform in [300, 3000], max_spectral_size = 256: every utterance is pre-clustered, its
          256 centroids are tested and take the spectral path
each under the AffinityGmmBic and under the FallbackClusterer single-cluster condition.  Per leg,
after a warm-up on the first 32 utterances, utterances/s of
`predict_batch(utterances, batch_multi_stage=True)` (best of --repeat).  A tree from before the
flag runs the same batch as its per-utterance loop: run this file with --root pointing at that
tree for the yardstick (`form` says which ran).  One JSON line per leg on stdout; --out appends
them to a file.

  python tools/multi_stage_batch_probe.py [--count 512] [--repeat 1] [--only mixed|reduce]
                                          [--condition AffinityGmmBic|FallbackClusterer]
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

WORKLOADS = {"mixed": (20, 400, 3015), "reduce": (300, 3000, 3014)}
CONDITIONS = ("AffinityGmmBic", "FallbackClusterer")
THRESHOLD = 0.5


def utterances(name, count):
  lo, hi, seed = WORKLOADS[name]
  rng = np.random.default_rng(seed)
  ns = rng.integers(lo, hi + 1, 512)
  ks = rng.integers(2, 7, 512)
  ks[::4] = 1
  return [_inputs.blobs(int(n), 256, int(k), seed=90000 + i)
          for i, (n, k) in enumerate(list(zip(ns, ks))[:count])]


def clusterer(sca, name, condition):
  from spectralcluster_amd import fallback_clusterer as fb
  options = fb.FallbackOptions(
      spectral_min_embeddings=100 if name == "mixed" else 1,
      single_cluster_condition=getattr(fb.SingleClusterCondition, condition),
      fallback_clusterer_type=fb.FallbackClustererType.Agglomerative,
      agglomerative_threshold=THRESHOLD)
  return sca.SpectralClusterer(min_clusters=1, max_clusters=7,
                               refinement_options=sca.configs.icassp2018_refinement_options,
                               fallback_options=options,
                               max_spectral_size=128 if name == "mixed" else 256)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--count", type=int, default=512)
  ap.add_argument("--repeat", type=int, default=1)
  ap.add_argument("--only", choices=sorted(WORKLOADS), default=None)
  ap.add_argument("--condition", choices=CONDITIONS, default=None)
  ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  ap.add_argument("--out", default=None)
  ap.add_argument("--tag", default="")
  args = ap.parse_args()
  sys.path.insert(0, os.path.abspath(args.root))
  import spectralcluster_amd as sca
  has_flag = "batch_multi_stage" in inspect.signature(
      sca.SpectralClusterer.predict_batch).parameters
  kwargs = {"batch_multi_stage": True} if has_flag else {}
  for name in ([args.only] if args.only else ["mixed", "reduce"]):
    us = utterances(name, args.count)
    for condition in ([args.condition] if args.condition else CONDITIONS):
      c = clusterer(sca, name, condition)
      c.predict_batch(us[:32], **kwargs)  # warm-up: arenas, streams, pinned staging
      best, labels = 0.0, []
      for _ in range(args.repeat):
        c.last_batch_reduced = None
        t0 = time.perf_counter()
        labels = c.predict_batch(us, **kwargs)
        best = max(best, len(us) / (time.perf_counter() - t0))
      kinds = getattr(c, "last_batch_reduced", None)
      single = getattr(c, "last_batch_single", None)
      routes = c.last_batch_routes
      rec = {"tag": args.tag, "workload": name, "condition": condition, "utterances": len(us),
             "n": list(WORKLOADS[name][:2]), "d": 256, "repeat": args.repeat,
             "form": "sc_predict_batch_multi_stage" if kinds is not None else "loop",
             "utt_per_s": round(best, 1),
             "kinds": {str(k): kinds.count(k) for k in sorted(set(kinds))} if kinds else None,
             "single": None if single is None else int(sum(bool(v) for v in single)),
             "routes": {str(r): routes.count(r) for r in sorted(set(routes))},
             # (the same results on either tree: checksums)
             "clusters_sum": int(sum(np.unique(l).size for l in labels)),
             "all_zero": int(sum(not np.any(l) for l in labels))}
      line = json.dumps(rec)
      print(line, flush=True)
      if args.out:
        with open(args.out, "a") as f:
          f.write(line + "\n")


if __name__ == "__main__":
  main()
