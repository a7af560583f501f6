#!/usr/bin/env python
"""Throughput of a batch, and of a stream pool, whose clusterer has min_clusters = 1 under the
FallbackClusterer single-cluster condition with the agglomerative fallback -- what the
multi-stage constructors set --, against the same batch with min_clusters = 2.

Batch legs: two compositions of 512 synthetic utterances (Gaussian blobs, fixed seeds, d = 256;
every fourth utterance holds ONE speaker, the others 2 .. 7), the ICASSP2018 options,
max_clusters = 7, agglomerative_threshold = 0.5:
  short    n uniform in [20, 128] (the short route)
  config5  n uniform in [300, 3000]: BASELINE config 5 (the grouped block Lanczos route)
Per composition and min_clusters, after one untimed run of the whole batch, utterances/s of
`predict_batch(utterances, batch_fallback_condition=True)` for every one of --repeat runs.  A tree
from before the flag runs the min_clusters = 1 call as its per-utterance loop: run this file with
--root pointing at that tree for the yardstick (`form` says which ran).  On a tree with the flag
the verdict call alone (`sc_batch_fallback_check`) is timed too, at the batch's threshold and at a
threshold above every distance (2.5: no chain ends early, the kernels' worst case).

Pool leg (--sessions S, 0 to skip): S multi-stage sessions (oracle turn_blobs, 4 speakers, d = 256,
L = 50, U1 = 100, U2 = 600, main clusterer min_clusters = 1) stepped together: 10 timed steps from
L rows (route 4 with the flags, 0 without) and 20 timed steps beyond U1 (route 1 with the flags, 2
without), each stretch after the same steps on other sessions; session-steps per second.

One JSON line per leg on stdout; --out appends them to a file.

  python tools/fallback_condition_batch_probe.py [--count 512] [--repeat 1] [--sessions 64]
                                                 [--only short|config5|pool]
                                                 [--min-clusters 1|2] [--root TREE]
                                                 [--out FILE] [--tag NAME]
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

THRESHOLD = 0.5
L, U1, U2, D = 50, 100, 600, 256


def utterances(name, count):
  if name == "short":
    rng = np.random.default_rng(2018)
    ns, ks = rng.integers(20, 129, 512), rng.integers(2, 7, 512)
    seeds = [50000 + i for i in range(512)]
  else:
    rng = np.random.default_rng(512)
    ns, ks = rng.integers(300, 3001, 512), rng.integers(2, 8, 512)
    seeds = list(range(512))
  ks[::4] = 1
  return [_inputs.blobs(int(n), D, int(k), seed=s) for n, k, s in list(zip(ns, ks, seeds))[:count]]


def emit(rec, out):
  line = json.dumps(rec)
  print(line, flush=True)
  if out:
    with open(out, "a") as f:
      f.write(line + "\n")


def make_clusterer(sca, min_clusters):
  from spectralcluster_amd import fallback_clusterer as fb
  options = fb.FallbackOptions(
      single_cluster_condition=fb.SingleClusterCondition.FallbackClusterer,
      fallback_clusterer_type=fb.FallbackClustererType.Agglomerative,
      agglomerative_threshold=THRESHOLD)
  return sca.SpectralClusterer(min_clusters=min_clusters, max_clusters=7,
                               refinement_options=sca.configs.icassp2018_refinement_options,
                               fallback_options=options)


def batch_legs(sca, args, has_flag):
  from spectralcluster_amd import utils
  for name in ("short", "config5"):
    if args.only not in (None, name):
      continue
    us = utterances(name, args.count)
    for min_clusters in ([args.min_clusters] if args.min_clusters else [1, 2]):
      c = make_clusterer(sca, min_clusters)
      kwargs = {"batch_fallback_condition": True} if has_flag and min_clusters == 1 else {}
      c.predict_batch(us, **kwargs)   # warm-up: the whole batch once (lanes, arenas, staging)
      rates, labels = [], []
      for _ in range(args.repeat):
        t0 = time.perf_counter()
        labels = c.predict_batch(us, **kwargs)
        rates.append(round(len(us) / (time.perf_counter() - t0), 1))
      single = getattr(c, "last_batch_single", None)
      routes = c.last_batch_routes
      rec = {"tag": args.tag, "workload": name, "min_clusters": min_clusters,
             "utterances": len(us), "d": D, "threshold": THRESHOLD,
             "form": ("sc_predict_batch_single_fallback" if single is not None else
                      "loop" if min_clusters == 1 else "sc_predict_batch_grouped"),
             "utt_per_s": rates, "slowest": min(rates), "fastest": max(rates),
             "single": (None if single is None else int(sum(single))),
             "routes": {str(r): routes.count(r) for r in sorted(set(routes))},
             # (the same clusters on either tree: a checksum of the results)
             "clusters_sum": int(sum(np.unique(l).size for l in labels))}
      if has_flag and min_clusters == 1:
        for key, threshold in (("verdicts_ms", THRESHOLD), ("verdicts_no_early_exit_ms", 2.5)):
          utils.cosine_single_cluster_check_batch(us, threshold)
          t0 = time.perf_counter()
          utils.cosine_single_cluster_check_batch(us, threshold)
          rec[key] = round(1e3 * (time.perf_counter() - t0), 2)
      emit(rec, args.out)


def pool_leg(sca, args, has_flag):
  import spectral_oracle as so
  from spectralcluster_amd import _lib
  count = args.sessions

  def conversations(first_seed):
    return [so.turn_blobs(U1 + 20, D, 4, seed=first_seed + i, noise=0.8)[0] for i in range(count)]

  def synchronize():
    _lib.default_handle().lib.sc_synchronize(_lib.default_handle().raw)

  kwargs = {"pool_early_stage": True, "pool_fallback_condition": True} if has_flag else {}
  pool = sca.MultiStageStreamPool(make_clusterer(sca, 1), fallback_threshold=THRESHOLD, L=L,
                                  U1=U1, U2=U2, capacity=count, d=D, **kwargs)
  ids = [pool.open() for _ in range(count)]

  def one_pass(convs):
    """10 steps from L rows, 20 steps beyond U1 -> seconds of both, routes, single answers."""
    routes, singles, seconds = {}, 0, []
    for first, steps in ((L, 10), (U1, 20)):
      for s, rows in zip(ids, convs):
        have = pool._sessions[s].num_embeddings
        pool.load(s, rows[have:first])
      synchronize()
      t0 = time.perf_counter()
      for t in range(first, first + steps):
        outs = pool.streaming_predict(ids, np.stack([rows[t] for rows in convs]))
        singles += sum(int(np.unique(o).size == 1) for o in outs)
        for r in pool.last_routes:
          routes[str(r)] = routes.get(str(r), 0) + 1
      synchronize()
      seconds.append(time.perf_counter() - t0)
    for s in ids:
      pool.reset(s)
    return seconds, routes, singles

  one_pass(conversations(90000))   # warm-up, other sessions
  (early_s, late_s), routes, singles = one_pass(conversations(80000))
  emit({"tag": args.tag, "workload": "pool", "sessions": count, "L_U1_U2": [L, U1, U2], "d": D,
        "min_clusters": 1, "flags": bool(kwargs), "threshold": THRESHOLD,
        "main_session_steps_per_s": round(count * 10 / early_s, 1),
        "beyond_u1_session_steps_per_s": round(count * 20 / late_s, 1),
        "routes": routes, "single_answers": singles}, args.out)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--count", type=int, default=512)
  ap.add_argument("--repeat", type=int, default=1)
  ap.add_argument("--sessions", type=int, default=64)
  ap.add_argument("--min-clusters", type=int, choices=[1, 2], default=None)
  ap.add_argument("--only", choices=["short", "config5", "pool"], default=None)
  ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  ap.add_argument("--out", default=None)
  ap.add_argument("--tag", default="")
  args = ap.parse_args()
  root = os.path.abspath(args.root)
  sys.path.insert(0, root)
  sys.path.insert(0, os.path.join(root, "oracle"))
  import spectralcluster_amd as sca
  has_flag = "batch_fallback_condition" in inspect.signature(
      sca.SpectralClusterer.predict_batch).parameters
  batch_legs(sca, args, has_flag)
  if args.sessions > 0 and args.only in (None, "pool"):
    pool_leg(sca, args, has_flag)


if __name__ == "__main__":
  main()
