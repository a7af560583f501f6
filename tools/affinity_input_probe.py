#!/usr/bin/env python
"""What it costs to cluster from an affinity the caller already holds.

Three workloads, each fed the same (n, n) matrices as NumPy float64, NumPy float32 and PyTorch
tensors on the GPU in float32 and float16:
  single   ms per call at n = 8192 (GraphCut Laplacian, max_clusters = 20, the ICASSP2018
           sequence): median, minimum and maximum over --repeat calls after a warm-up,
  batch    matrices/s over --count matrices of SURVEY.md's config 5 sizes (n in [300, 3000]),
  short    matrices/s over --short-count matrices of n in [20, 128]; best of --batch-repeat.
On a build with `predict_affinity` the calls are predict_affinity / predict_affinity_batch.  On
a build without it (the parent commit) the same work is the only way in that build has: a
clusterer whose `affinity_function` returns the matrix as a host float64 array -- a device
tensor is downloaded and widened inside that function, as a user of that build has to -- and a
predict() per matrix.
--kernel: instead of the legs above, a few `sc_set_affinity_array` calls on device sources at
n = 8192 and a device-to-device copy of the same traffic (n^2 (w + 8) / 2 bytes read and as many
written), then ONE batch call of each batch leg on float32 device tensors (the grouped ingest
launches of its groups and waves), for a `rocprofv3 --kernel-trace --stats` run.
One JSON line on stdout; --out appends it to a file (profiles/affinity_input_probe.jsonl).

  python tools/affinity_input_probe.py [--repeat 10] [--batch-repeat 2] [--count 64]
                                       [--short-count 512] [--kernel] [--out FILE] [--tag NAME]
"""
import argparse
import copy
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # (before the library: one HIP runtime in the process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import spectral_oracle as so  # noqa: E402
import spectralcluster_amd as sca  # noqa: E402

HAVE = hasattr(sca.SpectralClusterer, "predict_affinity")


def legs(mats):
  out = {"numpy_f64": mats, "numpy_f32": [a.astype(np.float32) for a in mats]}
  for name, dtype in (("device_f32", torch.float32), ("device_f16", torch.float16)):
    out[name] = [torch.from_numpy(a).to(dtype).cuda() for a in mats]
  torch.cuda.synchronize()
  return out


def as_host_f64(a):
  if isinstance(a, np.ndarray):
    return a.astype(np.float64, copy=False)
  return a.cpu().double().numpy()


def call(c, a):
  if HAVE:
    return c.predict_affinity(a)
  old = copy.copy(c)
  old.affinity_function = lambda _: as_host_f64(a)
  return old.predict(np.zeros((a.shape[0], 2)))


def call_batch(c, mats):
  if HAVE:
    return c.predict_affinity_batch(mats)
  return [call(c, a) for a in mats]


def clusterer(max_clusters):
  return sca.SpectralClusterer(min_clusters=2, max_clusters=max_clusters,
                               laplacian_type=sca.LaplacianType.GraphCut,
                               refinement_options=sca.configs.icassp2018_refinement_options)


def single(a, repeat, rec):
  c = clusterer(20)
  for name, (u,) in legs([a]).items():
    for _ in range(2):
      call(c, u)
    ms = []
    for _ in range(repeat):
      t0 = time.perf_counter()
      call(c, u)
      ms.append(1e3 * (time.perf_counter() - t0))
    rec[name] = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                 "max_ms": round(max(ms), 4)}


def batch(mats, repeat, rec, only=None):
  c = clusterer(7)
  for name, us in legs(mats).items():
    if only and name not in only:
      continue
    call_batch(c, us)
    best = 0.0
    for _ in range(repeat):
      t0 = time.perf_counter()
      call_batch(c, us)
      best = max(best, len(us) / (time.perf_counter() - t0))
    rec[name] = {"matrices_per_s": round(best, 1)}


def kernel_leg(a, rec):
  from spectralcluster_amd import _dlpack, _lib
  handle = _lib.default_handle()
  n = a.shape[0]
  for name, dtype, w in (("f64", torch.float64, 8), ("f32", torch.float32, 4),
                         ("f16", torch.float16, 2)):
    t = torch.from_numpy(a).to(dtype).cuda()
    for view_name, view in (("rows", t), ("transposed", t.t())):
      src = _dlpack.describe(view, lambda: handle, strided=True)
      for _ in range(5):
        handle.check(handle.lib.sc_set_affinity_array(handle.raw, ctypes.byref(src.array)))
      src.release()
    half = n * n * (w + 8) // 2  # a copy that reads and writes n^2 (w + 8) bytes in all
    x = torch.empty(half, dtype=torch.uint8, device="cuda")
    y = torch.empty_like(x)
    torch.cuda.synchronize()
    ms = []
    for _ in range(7):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      y.copy_(x)
      e1.record()
      torch.cuda.synchronize()
      ms.append(e0.elapsed_time(e1))
    rec[name] = {"traffic_bytes": n * n * (w + 8), "copy_ms_min": round(min(ms), 4),
                 "copy_GBps": round(n * n * (w + 8) / min(ms) / 1e6, 1)}
    del t, x, y


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeat", type=int, default=10)
  ap.add_argument("--batch-repeat", type=int, default=2)
  ap.add_argument("--count", type=int, default=64)
  ap.add_argument("--short-count", type=int, default=512)
  ap.add_argument("--kernel", action="store_true")
  ap.add_argument("--out", default=None)
  ap.add_argument("--tag", default="")
  args = ap.parse_args()
  big = so.affinity(so.blobs(8192, 64, 8, seed=8192))
  rec = {"tag": args.tag, "predict_affinity": HAVE}
  rng = np.random.default_rng(512)
  if args.kernel:
    k = {}
    kernel_leg(big, k)
    rec["kernel"] = {"n": 8192, "legs": k}
    c = clusterer(7)
    for name, sizes in (("batch", rng.integers(300, 3001, 512)[:args.count]),
                        ("short", rng.integers(20, 129, args.short_count))):
      us = [torch.from_numpy(so.affinity(so.blobs(int(n), 32, 2 + i % 3, seed=i))).float().cuda()
            for i, n in enumerate(sizes)]
      call_batch(c, us)
      routes = list(c.last_batch_routes)
      rec["kernel"][name] = {"matrices": len(us), "routes": {r: routes.count(r) for r in (0, 1, 2)}}
  else:
    ns = rng.integers(300, 3001, 512)[:args.count]
    ks = rng.integers(2, 8, 512)[:args.count]
    mats = [so.affinity(so.blobs(int(n), 64, int(k), seed=i))
            for i, (n, k) in enumerate(zip(ns, ks))]
    sns = rng.integers(20, 129, args.short_count)
    shorts = [so.affinity(so.blobs(int(n), 32, 2 + i % 3, seed=9000 + i))
              for i, n in enumerate(sns)]
    one, many, small = {}, {}, {}
    single(big, args.repeat, one)
    batch(mats, args.batch_repeat, many, only=("numpy_f64", "device_f32"))
    batch(shorts, args.batch_repeat, small, only=("numpy_f64", "device_f32"))
    rec["single"] = {"n": 8192, "repeat": args.repeat, "legs": one}
    rec["batch"] = {"matrices": len(mats), "n": [300, 3000], "repeat": args.batch_repeat,
                    "legs": many}
    rec["short"] = {"matrices": len(shorts), "n": [20, 128], "repeat": args.batch_repeat,
                    "legs": small}
  line = json.dumps(rec)
  print(line, flush=True)
  if args.out:
    with open(args.out, "a") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()
