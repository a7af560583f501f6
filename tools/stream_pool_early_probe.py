#!/usr/bin/env python
"""Throughput of S multi-stage streaming sessions over their first U1 rows, the stage before any
pre-clustering.

S fresh synthetic conversations (oracle turn_blobs, fixed seeds, 4 speakers, d = 256) under the
class defaults L = 50, U1 = 100, U2 = 600 are stepped together from their first row to row U1.
Steps 2 .. L - 1 (the agglomerative fallback) and steps L .. U1 (the main clusterer on the cache)
are timed separately, each ending in a synchronise, after a warm-up pass over the whole stretch
on other sessions (other seeds) of the same pool; session-steps per second.
  --mode pool   one MultiStageStreamPool, one streaming_predict call per step for all S sessions.
                With --early the pool is built with pool_early_stage=True (routes 3 and 4);
                without it every session runs main.predict on its own (route 0) -- that form
                uses nothing the flag added: run it with --root <a checkout of the commit before
                the flag> to time that build.
The route counts of the timed steps are reported.  One JSON line per S on stdout; --out appends
them to a file.

  python tools/stream_pool_early_probe.py --mode pool [--early] [--sessions 1,16,64,256]
                                          [--root DIR] [--out FILE] [--tag NAME]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("pool",), required=True)
ap.add_argument("--early", action="store_true")
ap.add_argument("--sessions", default="1,16,64,256")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
ap.add_argument("--tag", default="")
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import spectral_oracle as so  # noqa: E402
import spectralcluster_amd as sca  # noqa: E402
from spectralcluster_amd import _lib  # noqa: E402

L, U1, U2, D = 50, 100, 600, 256


def clusterer():
  return sca.SpectralClusterer(min_clusters=2, max_clusters=7,
                               refinement_options=sca.configs.icassp2018_refinement_options)


def conversations(count, first_seed):
  return [so.turn_blobs(U1, D, 4, seed=first_seed + i, noise=0.8)[0] for i in range(count)]


def synchronize():
  _lib.default_handle().lib.sc_synchronize(_lib.default_handle().raw)


def one_pass(pool, ids, convs):
  """Every session from its first row to row U1 -> seconds of the two stretches, route counts."""
  for s in ids:
    pool.reset(s)
  routes = {}
  marks = []
  for t in range(U1):            # step t appends row t + 1
    if t in (1, L - 1):
      synchronize()
      marks.append(time.perf_counter())
    pool.streaming_predict(ids, np.stack([rows[t] for rows in convs]))
    if t >= 1:
      for r in pool.last_routes:
        routes[str(r)] = routes.get(str(r), 0) + 1
  synchronize()
  marks.append(time.perf_counter())
  return marks[1] - marks[0], marks[2] - marks[1], routes


def main():
  for count in [int(v) for v in args.sessions.split(",")]:
    kwargs = {"pool_early_stage": True} if args.early else {}
    pool = sca.MultiStageStreamPool(clusterer(), L=L, U1=U1, U2=U2, capacity=count, d=D, **kwargs)
    ids = [pool.open() for _ in range(count)]
    one_pass(pool, ids, conversations(count, 90000))           # warm-up, other sessions
    fallback_s, main_s, routes = one_pass(pool, ids, conversations(count, 80000))
    rec = {"tag": args.tag, "mode": args.mode, "early": bool(args.early), "sessions": count,
           "L_U1_U2": [L, U1, U2], "d": D,
           "fallback_steps": L - 2, "main_steps": U1 - L + 1,
           "fallback_session_steps_per_s": round(count * (L - 2) / fallback_s, 1),
           "main_session_steps_per_s": round(count * (U1 - L + 1) / main_s, 1),
           "fallback_ms_per_step": round(1e3 * fallback_s / (L - 2), 3),
           "main_ms_per_step": round(1e3 * main_s / (U1 - L + 1), 3),
           "routes": routes}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
      with open(args.out, "a") as f:
        f.write(line + "\n")
    del pool


if __name__ == "__main__":
  main()
