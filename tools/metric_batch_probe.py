#!/usr/bin/env python
"""What `predict_batch(..., batch_any_metric=True)` buys a clusterer with custom_dist="euclidean",
and what the chain's iteration kernel costs per metric next to the single-workgroup kernel.

Batch legs (ICASSP2018 options, max_clusters = 7, d = 256, oracle blobs with fixed seeds; one
untimed call, then the best of --repeat timed calls, utterances/s):
  config5   the 512 utterances of BASELINE config 5, n in [300, 3000]
  short     512 clips, n in [20, 128] (tools/short_batch_probe.py's draw)
each with custom_dist = "euclidean" and "cosine".  This tree passes batch_any_metric=True; a tree
without the keyword (the parent commit) makes the same call without it.  The driver runs --pairs
fresh processes of this tree alternating with as many of the tree at --parent (a checkout of the
parent commit with its library built), and `bench.py --gpus 1 --steps 5 --warmup 1` of both trees
--bench times; one JSON line per process, appended to --out.

  python tools/metric_batch_probe.py --parent DIR [--pairs 6] [--bench 2] [--count 512]
                                     [--out profiles/metric_batch_probe.jsonl]

Kernel leg (this tree; the process to put under `rocprofv3 --kernel-trace --stats`):
  python tools/metric_batch_probe.py --leg kernels
runs the k-means stage alone on an (n, 8) embedding at n = 3000 and n = 8192, for every device
metric first as the chain (sc_stage_kmeans_trace_metric, form = chain) and then as the
single-workgroup kernel (form = single), in that order and nothing else.
  python tools/metric_batch_probe.py --summary RESULTS.db > profiles/metric_batch_kernel_stats.txt
turns the trace into the per-kernel table of tools/rocprof_summary.py followed by one row per
(n, metric): passes, the per-launch time of the working km_iter launches (a launch after the stop
rule has fired returns at once and is not counted), the kernel time of the whole chain, and the
k_kmeans launch of the same input.
"""
import argparse
import ctypes
import inspect
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_NS = (3000, 8192)
KERNEL_K = 8
KERNEL_METRICS = ("cosine", "euclidean", "sqeuclidean", "cityblock", "chebyshev", "correlation",
                  "braycurtis", "canberra")


def batches(so, count):
  rng = np.random.default_rng(512)  # (bench.py's batch512_sizes)
  ns, ks = rng.integers(300, 3001, 512)[:count], rng.integers(2, 8, 512)[:count]
  config5 = [so.blobs(int(n), 256, int(k), seed=i) for i, (n, k) in enumerate(zip(ns, ks))]
  rng = np.random.default_rng(2018)  # (tools/short_batch_probe.py's utterances)
  ns, ks = rng.integers(20, 129, 512)[:count], rng.integers(2, 7, 512)[:count]
  short = [so.blobs(int(n), 256, int(k), seed=50000 + i) for i, (n, k) in enumerate(zip(ns, ks))]
  return {"config5": config5, "short": short}


def child_batch(args):
  sys.path.insert(0, args.tree)
  sys.path.insert(0, os.path.join(args.tree, "oracle"))
  import spectral_oracle as so
  import spectralcluster_amd as sca
  flagged = "batch_any_metric" in inspect.signature(sca.SpectralClusterer.predict_batch).parameters
  rec = {"tag": args.tag, "leg": "batch", "flag": flagged, "repeat": args.repeat, "rates": {}}
  for name, utts in batches(so, args.count).items():
    for metric in ("euclidean", "cosine"):
      c = sca.SpectralClusterer(
          min_clusters=2, max_clusters=7, custom_dist=metric,
          refinement_options=sca.configs.icassp2018_refinement_options)
      kw = {"batch_any_metric": True} if flagged else {}
      c.predict_batch(utts, **kw)  # warm-up: arenas, tile maps
      best = float("inf")
      for _ in range(args.repeat):
        t0 = time.perf_counter()
        c.predict_batch(utts, **kw)
        best = min(best, time.perf_counter() - t0)
      routes = c.last_batch_routes
      rec["rates"]["%s_%s" % (name, metric)] = {
          "utterances": len(utts), "utt_per_s": round(len(utts) / best, 1),
          "routes": {str(r): routes.count(r) for r in sorted(set(routes))}}
  return rec


def kernel_input(n, k):
  rng = np.random.default_rng(n)
  centres = rng.standard_normal((k, k))
  return centres[rng.integers(0, k, size=n)] + rng.standard_normal((n, k))


def child_kernels(args):
  sys.path.insert(0, args.tree)
  from spectralcluster_amd import _lib
  handle = _lib.default_handle(0)
  rec = {"tag": args.tag, "leg": "kernels", "k": KERNEL_K, "calls": []}
  for n in KERNEL_NS:
    e = np.ascontiguousarray(kernel_input(n, KERNEL_K))
    for metric in KERNEL_METRICS:
      passes = {}
      for form, name in ((1, "chain"), (2, "single")):
        labels = np.empty(n, dtype=np.int64)
        iters, form_run = ctypes.c_int(0), ctypes.c_int(0)
        handle.check(handle.lib.sc_stage_kmeans_trace_metric(
            handle.raw, _lib.as_double_p(e), n, KERNEL_K, 300, form, _lib.KMEANS_METRICS[metric],
            ctypes.byref(form_run), None, None, None, None, None, None, None, 0,
            ctypes.byref(iters), None, _lib.as_int64_p(labels)))
        passes[name] = iters.value
      rec["calls"].append({"n": n, "metric": metric, "passes": passes})
  return rec


def summary(path):
  import sqlite3
  sys.path.insert(0, os.path.join(ROOT, "tools"))
  import rocprof_summary
  rocprof_summary.main(path)
  cur = sqlite3.connect(path).cursor()
  rows = list(cur.execute("select name, start, end from kernels order by start"))
  # the kernel leg's order: per (n, metric) one chain call (km_colsum ... km_iter) and then one
  # k_kmeans launch, which closes the pair
  calls, chain = [], []
  for name, start, end in rows:
    short = rocprof_summary.short_name(name)
    if "k_kmeans" in short:
      calls.append((chain, (end - start) / 1e3))
      chain = []
    elif "km_" in short:
      chain.append((short, start, end))
  want = [(n, m) for n in KERNEL_NS for m in KERNEL_METRICS]
  print("\n# the k-means stage alone, k = %d, per (n, metric): the chain (km_iter launches that "
        "did an assignment: count, median and max us per launch; kernel time of all its launches "
        "and first start to last end) and the single-workgroup k_kmeans launch on the same input"
        % KERNEL_K)
  if len(calls) != len(want):
    print("# %d chain / k_kmeans pairs found where the kernel leg makes %d: no table"
          % (len(calls), len(want)))
    return
  print("%6s %-12s %7s %12s %12s %14s %14s %12s" % (
      "n", "metric", "passes", "iter_med_us", "iter_max_us", "chain_sum_us", "chain_span_us",
      "k_kmeans_us"))
  for (n, metric), (chain, single_us) in zip(want, calls):
    iters = [(e - s) / 1e3 for name, s, e in chain if "km_iter" in name]
    working = [d for d in iters if d > 0.5 * max(iters)]
    total = sum((e - s) / 1e3 for _, s, e in chain)
    span = (max(e for _, _, e in chain) - min(s for _, s, _ in chain)) / 1e3
    print("%6d %-12s %7d %12.2f %12.2f %14.1f %14.1f %12.1f" % (
        n, metric, len(working), statistics.median(working), max(working), total, span,
        single_us))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--parent", default=None, help="checkout of the parent commit, library built")
  ap.add_argument("--pairs", type=int, default=6)
  ap.add_argument("--bench", type=int, default=2, help="bench.py runs per tree")
  ap.add_argument("--count", type=int, default=512)
  ap.add_argument("--repeat", type=int, default=3)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metric_batch_probe.jsonl"))
  ap.add_argument("--leg", default=None, help="(child) batch | kernels, in this process")
  ap.add_argument("--tree", default=ROOT)
  ap.add_argument("--tag", default="")
  ap.add_argument("--summary", default=None, help="rocpd database of a --leg kernels run")
  args = ap.parse_args()
  if args.summary:
    return summary(args.summary)
  if args.leg:
    rec = child_batch(args) if args.leg == "batch" else child_kernels(args)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
      with open(args.out, "a") as f:
        f.write(line + "\n")
    return
  trees = [("this", ROOT)] + ([("parent", os.path.abspath(args.parent))] if args.parent else [])
  # (a failed or hung process ends the probe: nothing more is started on the device)
  for i in range(args.pairs):
    for tag, tree in trees:
      subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "batch", "--tree", tree,
                      "--count", str(args.count), "--repeat", str(args.repeat), "--out", args.out,
                      "--tag", "%s%d" % (tag, i)], check=True, timeout=600)
  for i in range(args.bench):
    for tag, tree in trees:
      out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1",
                            "--steps", "5", "--warmup", "1"], check=True, timeout=900, cwd=tree,
                           capture_output=True, text=True).stdout
      result = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
      line = json.dumps({"tag": "%s%d" % (tag, i), "leg": "bench", "value": result.get("value"),
                         "unit": result.get("unit"),
                         "batch512": (result.get("batch512") or {}).get("value")})
      print(line, flush=True)
      with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
  main()
