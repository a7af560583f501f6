#!/usr/bin/env python
"""Throughput of a batch of SHORT utterances (n <= 128: the dense Jacobi eigensolver).

512 utterances, n uniform in [20, 128], d = 256, k in [2, 6] (oracle blobs, fixed seeds), under
the ICASSP2018 preset and under the same with a GraphCut Laplacian and max_clusters=20.  Per
configuration, after a warm-up batch, utterances/s of predict_batch(streams=1), (streams=8) and
(group=16), and how many utterances took which route where the library reports it (older builds
do not).  One JSON line per configuration on stdout; --out appends them to a file.

  python tools/short_batch_probe.py [--count 512] [--repeat 3] [--out FILE] [--tag NAME]
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


def utterances(count):
  rng = np.random.default_rng(2018)
  ns = rng.integers(20, 129, count)
  ks = rng.integers(2, 7, count)
  return [so.blobs(int(n), 256, int(k), seed=50000 + i) for i, (n, k) in enumerate(zip(ns, ks))]


def clusterer(name):
  kw = {}
  if name == "graphcut_max20":
    kw = {"laplacian_type": sca.LaplacianType.GraphCut, "max_clusters": 20}
  return sca.SpectralClusterer(
      min_clusters=2, max_clusters=kw.pop("max_clusters", 7),
      refinement_options=sca.configs.icassp2018_refinement_options, **kw)


def rate(c, utts, repeat, **kw):
  c.predict_batch(utts, **kw)  # warm-up: arenas, streams, pinned staging
  best = 0.0
  for _ in range(repeat):
    t0 = time.perf_counter()
    c.predict_batch(utts, **kw)
    best = max(best, len(utts) / (time.perf_counter() - t0))
  routes = getattr(c, "last_batch_routes", None)
  counts = None if routes is None else {str(r): routes.count(r) for r in sorted(set(routes))}
  return best, counts


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--count", type=int, default=512)
  ap.add_argument("--repeat", type=int, default=3)
  ap.add_argument("--out", default=None)
  ap.add_argument("--tag", default="")
  args = ap.parse_args()
  utts = utterances(args.count)
  for name in ("icassp2018", "graphcut_max20"):
    c = clusterer(name)
    rec = {"tag": args.tag, "config": name, "utterances": len(utts), "n": [20, 128], "d": 256}
    for key, kw in (("streams1", {"streams": 1}), ("streams8", {"streams": 8}),
                    ("group16", {"group": 16})):
      r, counts = rate(c, utts, args.repeat, **kw)
      rec[key + "_utt_per_s"] = round(r, 1)
      if key == "group16":
        rec["group16_routes"] = counts
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
      with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
  main()
