#!/usr/bin/env python
"""What the place and the dtype of a k-means input cost.

Three calls, each fed the same values in five ways -- NumPy float64 (the path every release has
had), NumPy float32, and PyTorch tensors on the GPU in float64, float32 and float16:
  custom_8192x256_k20    CustomKMeans(20, centroids).predict on (8192, 256)
  custom_200000x64_k10   CustomKMeans(10, centroids).predict on (200000, 64)
  run_8192x8_k8          run_kmeans on an (8192, 8) embedding, 8 clusters, cosine
ms per call: median, minimum and maximum over --repeat calls after a warm-up.  A build whose
k-means entries take host float64 arrays only (the parent commit) runs the same legs the only way
it can: the tensor is brought to the host, widened to float64 there and passed as always -- that
download and widening are inside its time, as they are inside a caller's.  PyTorch is loaded
before the library in every build, so all of them are measured in the same process state.

--copy adds the time of a device-to-device copy that moves the traffic of the float16 ingest of
each shape (n * dim * (2 + 8) bytes read + written), by HIP events around `Tensor.copy_`.

One JSON line on stdout; --out appends it to a file (profiles/kmeans_input_probe.jsonl).

  python tools/kmeans_input_probe.py [--repeat 20] [--legs a,b] [--shapes a,b] [--copy]
                                     [--out FILE] [--tag NAME]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import spectral_oracle as so  # noqa: E402
from spectralcluster_amd import custom_distance_kmeans as ckm  # noqa: E402

IN_PLACE = hasattr(ckm, "_describe")  # this build reads a described source where it is

SHAPES = {
    "custom_8192x256_k20": ("custom", 8192, 256, 20),
    "custom_200000x64_k10": ("custom", 200000, 64, 10),
    "run_8192x8_k8": ("run", 8192, 8, 8),
}
LEGS = {
    "numpy_f64": lambda x: x,
    "numpy_f32": lambda x: x.astype(np.float32),
    "device_f64": lambda x: torch.from_numpy(x).cuda(),
    "device_f32": lambda x: torch.from_numpy(x).to(torch.float32).cuda(),
    "device_f16": lambda x: torch.from_numpy(x).to(torch.float16).cuda(),
}


def call(kind, u, k, init):
  if not IN_PLACE and isinstance(u, torch.Tensor):
    u = u.cpu().double().numpy()
  if kind == "run":
    return ckm.run_kmeans(u, k, "cosine", 300)
  return ckm.CustomKMeans(k, centroids=init.copy()).predict(u)


def d2d_copy_ms(nbytes, repeat):
  """Median ms of a device-to-device copy of nbytes (nbytes read + nbytes written)."""
  src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
  dst = torch.empty_like(src)
  ms = []
  for i in range(repeat + 3):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    dst.copy_(src)
    b.record()
    b.synchronize()
    if i >= 3:
      ms.append(a.elapsed_time(b))
  return round(statistics.median(ms), 4)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeat", type=int, default=20)
  ap.add_argument("--legs", default=",".join(LEGS))
  ap.add_argument("--shapes", default=",".join(SHAPES))
  ap.add_argument("--copy", action="store_true")
  ap.add_argument("--out", default=None)
  ap.add_argument("--tag", default="")
  args = ap.parse_args()
  rec = {"tag": args.tag, "in_place": IN_PLACE, "repeat": args.repeat, "shapes": {}}
  for name in args.shapes.split(","):
    kind, n, dim, k = SHAPES[name]
    x = so.blobs(n, dim, k, seed=n + dim)
    init = x[np.linspace(0, n - 1, k).astype(int)].copy()
    legs = {}
    for leg in args.legs.split(","):
      u = LEGS[leg](x)
      torch.cuda.synchronize()
      for _ in range(3):
        call(kind, u, k, init)
      ms = []
      for _ in range(args.repeat):
        t0 = time.perf_counter()
        call(kind, u, k, init)
        ms.append(1e3 * (time.perf_counter() - t0))
      legs[leg] = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                   "max_ms": round(max(ms), 4)}
      del u
    rec["shapes"][name] = {"n": n, "dim": dim, "k": k, "legs": legs}
    if args.copy:
      half = n * dim * (2 + 8) // 2  # the copy reads and writes each of its bytes
      rec["shapes"][name]["f16_ingest_traffic_bytes"] = 2 * half
      rec["shapes"][name]["d2d_copy_same_traffic_ms"] = d2d_copy_ms(half, args.repeat)
  line = json.dumps(rec)
  print(line, flush=True)
  if args.out:
    with open(args.out, "a") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()
