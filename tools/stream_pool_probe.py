#!/usr/bin/env python
"""Throughput of S open multi-stage streaming sessions advanced one embedding each per step.

S synthetic conversations (oracle turn_blobs, fixed seeds, 4 speakers, d = 256) under the class
defaults L = 50, U1 = 100, U2 = 600; session i resumes with a cache of a size spread evenly over
(100, 600), so every step is the steady state beyond U1 (and the longest caches reach U2 and are
compressed).  After --warmup steps, --steps timed steps ending in a synchronise; session-steps per
second.
  --mode pool  one MultiStageStreamPool, one streaming_predict call per step for all S sessions
               (the route counts of the timed steps are reported);
  --mode loop  S MultiStageClusterer objects fed the same rows in a Python loop -- the yardstick.
               It uses nothing the pool added: run it with --root <a checkout of the commit
               before the pool> to time that build.
One JSON line per S on stdout; --out appends them to a file.

  python tools/stream_pool_probe.py --mode pool|loop [--sessions 1,16,64,256] [--steps 50]
                                    [--warmup 5] [--root DIR] [--out FILE] [--tag NAME]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("pool", "loop"), required=True)
ap.add_argument("--sessions", default="1,16,64,256")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
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


def conversations(count, steps):
  """Per session: the rows it resumes with and the rows of its steps."""
  starts = np.linspace(U1 + 10, U2 - 10, count).astype(int) if count > 1 else np.array([350])
  out = []
  for i, n in enumerate(starts):
    x, _, _ = so.turn_blobs(int(n) + steps, D, 4, seed=80000 + i, noise=0.8)
    out.append((x[:n], x[n:]))
  return out


def run_pool(convs, warmup, steps):
  pool = sca.MultiStageStreamPool(clusterer(), L=L, U1=U1, U2=U2, capacity=len(convs), d=D)
  ids = []
  for loaded, _ in convs:
    ids.append(pool.open())
    pool.load(ids[-1], loaded)
  routes = {}
  t0 = 0.0
  for t in range(warmup + steps):
    if t == warmup:
      _lib.default_handle().lib.sc_synchronize(_lib.default_handle().raw)
      t0 = time.perf_counter()
    pool.streaming_predict(ids, np.stack([rows[t] for _, rows in convs]))
    if t >= warmup:
      for r in pool.last_routes:
        routes[str(r)] = routes.get(str(r), 0) + 1
  _lib.default_handle().lib.sc_synchronize(_lib.default_handle().raw)
  return time.perf_counter() - t0, routes


def run_loop(convs, warmup, steps):
  main = clusterer()
  streams = []
  for loaded, _ in convs:
    s = sca.MultiStageClusterer(main, L=L, U1=U1, U2=U2)
    s.cache, s.num_embeddings = loaded.copy(), loaded.shape[0]   # resumed, as pool.load does
    streams.append(s)
  t0 = 0.0
  for t in range(warmup + steps):
    if t == warmup:
      _lib.default_handle().lib.sc_synchronize(_lib.default_handle().raw)
      t0 = time.perf_counter()
    for s, (_, rows) in zip(streams, convs):
      s.streaming_predict(rows[t])
  _lib.default_handle().lib.sc_synchronize(_lib.default_handle().raw)
  return time.perf_counter() - t0, None


def main():
  for count in [int(v) for v in args.sessions.split(",")]:
    convs = conversations(count, args.warmup + args.steps)
    seconds, routes = (run_pool if args.mode == "pool" else run_loop)(convs, args.warmup,
                                                                      args.steps)
    rec = {"tag": args.tag, "mode": args.mode, "sessions": count, "steps": args.steps,
           "warmup": args.warmup, "L_U1_U2": [L, U1, U2], "d": D,
           "session_steps_per_s": round(count * args.steps / seconds, 1),
           "ms_per_step": round(1e3 * seconds / args.steps, 3)}
    if routes is not None:
      rec["routes"] = routes
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
      with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
  main()
