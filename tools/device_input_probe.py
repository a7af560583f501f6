#!/usr/bin/env python
"""What the place and the dtype of the embeddings cost.

Two workloads, each fed the same values in five ways -- NumPy float64 (the path every release
has had), NumPy float32, and PyTorch tensors on the GPU in float64, float32 and float16:
  single   ms per predict() at n = 8192, d = 256 (GraphCut Laplacian, max_clusters = 20, the
           ICASSP2018 sequence): median, minimum and maximum over --repeat calls after a warm-up,
  batch    utterances/s of predict_batch(group=16) on SURVEY.md's config 5 (512 utterances,
           n in [300, 3000], d = 256, the ICASSP2018 preset): best of --batch-repeat.
The NumPy legs run first, before PyTorch has touched the device.  A build without the
described-array entry points runs the NumPy float64 leg alone, so the same script measures the
parent commit.  One JSON line on stdout; --out appends it to a file
(profiles/device_input_probe.jsonl).  PyTorch is used here, never by the package.

  python tools/device_input_probe.py [--repeat 30] [--batch-repeat 3] [--count 512]
                                     [--out FILE] [--tag NAME]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

# The producer of the device tensors is loaded before the library, as in a pipeline whose
# encoder runs first: the process then has one HIP runtime, the one PyTorch brings (loaded the
# other way round, PyTorch may find no device).  Every build is measured in this same state.
try:
  import torch
except ImportError:
  torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import spectral_oracle as so  # noqa: E402
import spectralcluster_amd as sca  # noqa: E402

try:
  from spectralcluster_amd import _dlpack  # noqa: F401,E402
  HAVE_ARRAYS = True
except ImportError:
  HAVE_ARRAYS = False


def host_legs(arrays):
  """name -> the list `arrays` (NumPy float64) as a host leg hands it over."""
  out = {"numpy_f64": arrays}
  if HAVE_ARRAYS:
    out["numpy_f32"] = [a.astype(np.float32) for a in arrays]
  return out


def device_legs(arrays):
  if not HAVE_ARRAYS or torch is None:
    return {}
  out = {name: [torch.from_numpy(a).to(dtype).cuda() for a in arrays]
         for name, dtype in (("device_f64", torch.float64), ("device_f32", torch.float32),
                             ("device_f16", torch.float16))}
  torch.cuda.synchronize()
  return out


def single(x, legs, repeat, rec):
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=20, laplacian_type=sca.LaplacianType.GraphCut,
                            refinement_options=sca.configs.icassp2018_refinement_options)
  for name, (u,) in legs([x]).items():
    for _ in range(3):
      c.predict(u)
    ms = []
    for _ in range(repeat):
      t0 = time.perf_counter()
      c.predict(u)
      ms.append(1e3 * (time.perf_counter() - t0))
    rec[name] = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                 "max_ms": round(max(ms), 4)}


def batch(utts, legs, repeat, rec):
  c = sca.configs.icassp2018_clusterer
  for name, us in legs(utts).items():
    c.predict_batch(us, group=16)  # warm-up: arenas, lanes, streams
    best = 0.0
    for _ in range(repeat):
      t0 = time.perf_counter()
      c.predict_batch(us, group=16)
      best = max(best, len(us) / (time.perf_counter() - t0))
    rec[name] = {"utt_per_s": round(best, 1)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeat", type=int, default=30)
  ap.add_argument("--batch-repeat", type=int, default=3)
  ap.add_argument("--count", type=int, default=512)
  ap.add_argument("--out", default=None)
  ap.add_argument("--tag", default="")
  args = ap.parse_args()
  x = so.blobs(8192, 256, 8, seed=8192)
  rng = np.random.default_rng(512)
  ns = rng.integers(300, 3001, 512)[:args.count]
  ks = rng.integers(2, 8, 512)[:args.count]
  utts = [so.blobs(int(n), 256, int(k), seed=i) for i, (n, k) in enumerate(zip(ns, ks))]
  one, many = {}, {}
  # the host legs first, before PyTorch has initialised the device -- the state in which a
  # build without device inputs runs its only leg; the device legs (PyTorch holding its own
  # streams, queues and device memory next to the library's) follow
  for legs in (host_legs, device_legs):
    single(x, legs, args.repeat, one)
    batch(utts, legs, args.batch_repeat, many)
  rec = {"tag": args.tag, "described_arrays": HAVE_ARRAYS,
         "single": {"n": 8192, "d": 256, "repeat": args.repeat, "legs": one},
         "batch": {"utterances": len(utts), "n": [300, 3000], "d": 256, "group": 16,
                   "repeat": args.batch_repeat, "legs": many}}
  line = json.dumps(rec)
  print(line, flush=True)
  if args.out:
    with open(args.out, "a") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()
