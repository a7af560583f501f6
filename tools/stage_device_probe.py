#!/usr/bin/env python
"""What the building blocks cost a caller whose matrices live on the GPU.

At n = 8192 and n = 2048 it times `utils.compute_affinity_matrix` (d = 256), `CropDiagonal`,
`GaussianBlur`, `RowWiseThreshold`, `Diffuse`, `laplacian.compute_laplacian` and
`utils.compute_sorted_eigenvectors(count=21)` on four legs:
  device_f64   a float64 device tensor in, a float64 device tensor out,
  device_f32   the same in float32,
  numpy_f32    a NumPy float32 array in, a NumPy float32 `out`,
  numpy_f64    a NumPy float64 array in, `out=None`: the untouched path.
On a build with `out=` the call is `f(x, out=o)`.  On a build without it (the parent commit) the
same work is what a user of that build has to write: `.cpu().numpy()`, the function, then
`torch.from_numpy(result.astype(dtype)).to(device)` (an `.astype` alone for the NumPy leg).
Per step and leg: minimum and maximum ms over --repeat calls after a warm-up call.
--kernel: instead, a few device-to-device calls of one cheap operator per output dtype and layout
at n = 8192 (the egress kernels, for a `rocprofv3 --kernel-trace --stats` run) and a
device-to-device copy of the same traffic, n^2 (8 + w) bytes, timed in the same process.
One JSON line on stdout; --out appends it to a file (profiles/stage_device_probe.jsonl).

--legs numpy_f64 times the untouched path in a process that runs nothing else.

  python tools/stage_device_probe.py [--repeat 3] [--sizes 8192,2048] [--legs a,b] [--kernel]
                                     [--out FILE] [--tag NAME]
"""
import argparse
import inspect
import json
import os
import sys
import time

import numpy as np
import torch  # (before the library: one HIP runtime in the process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import spectralcluster_amd as sca  # noqa: E402
from spectralcluster_amd import laplacian, refinement, utils  # noqa: E402

HAVE = "out" in inspect.signature(utils.compute_affinity_matrix).parameters
COUNT = 21


def steps():
  return [
      ("affinity", utils.compute_affinity_matrix, "embeddings"),
      ("crop_diagonal", refinement.CropDiagonal().refine, "matrix"),
      ("gaussian_blur", refinement.GaussianBlur(1).refine, "matrix"),
      ("row_wise_threshold", refinement.RowWiseThreshold().refine, "matrix"),
      ("diffuse", refinement.Diffuse().refine, "matrix"),
      ("laplacian", laplacian.compute_laplacian, "matrix"),
      ("sorted_eigenvectors", None, "symmetric"),
  ]


def run(name, f, x, outs, leg):
  """One call of a step on a leg; returns its result(s) where the leg wants them."""
  device = leg.startswith("device")
  if name == "sorted_eigenvectors":
    if HAVE and leg != "numpy_f64":
      return utils.compute_sorted_eigenvectors(x, True, COUNT, out=outs)
    if leg == "numpy_f64":
      return utils.compute_sorted_eigenvectors(x, True, COUNT)
    w, v = utils.compute_sorted_eigenvectors(x.cpu().numpy() if device else x, True, COUNT)
    narrow = np.float64 if leg == "device_f64" else np.float32
    if device:
      return (torch.from_numpy(w.astype(narrow)).to("cuda"),
              torch.from_numpy(v.astype(narrow)).to("cuda"))
    return w.astype(narrow), v.astype(narrow)
  if leg == "numpy_f64":
    return f(x)
  if HAVE:
    return f(x, out=outs)
  if device:
    r = f(x.cpu().numpy())
    return torch.from_numpy(r.astype(np.float64 if leg == "device_f64" else np.float32)).to("cuda")
  return f(x).astype(np.float32)


def inputs(n, rng):
  emb = rng.standard_normal((n, 256))
  a = rng.uniform(0.05, 0.95, (n, n))
  s = (a + a.T) / 2
  return {"embeddings": emb, "matrix": a, "symmetric": s}


def on_leg(values, leg):
  if leg == "numpy_f64":
    return values
  if leg == "numpy_f32":
    return values.astype(np.float32)
  t = torch.from_numpy(values).to(torch.float64 if leg == "device_f64" else torch.float32).cuda()
  torch.cuda.synchronize()
  return t


def outputs(name, n, leg):
  if leg == "numpy_f64":
    return None
  shapes = [(COUNT,), (n, COUNT)] if name == "sorted_eigenvectors" else [(n, n)]
  if leg == "numpy_f32":
    made = [np.empty(s, dtype=np.float32) for s in shapes]
  else:
    dtype = torch.float64 if leg == "device_f64" else torch.float32
    made = [torch.empty(s, dtype=dtype, device="cuda") for s in shapes]
  return tuple(made) if len(made) == 2 else made[0]


LEGS = ("device_f64", "device_f32", "numpy_f32", "numpy_f64")


def timing(sizes, repeat, rec, legs=LEGS):
  rng = np.random.default_rng(8192)
  for n in sizes:
    data = inputs(n, rng)
    per_n = {}
    for name, f, what in steps():
      per_step = {}
      for leg in legs:
        x = on_leg(data[what], leg)
        outs = outputs(name, n, leg)
        ms = []
        for i in range(repeat + 1):
          torch.cuda.synchronize()
          t0 = time.perf_counter()
          run(name, f, x, outs, leg)
          torch.cuda.synchronize()
          if i:
            ms.append(1e3 * (time.perf_counter() - t0))
        per_step[leg] = {"min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}
        del x, outs
      per_n[name] = per_step
    rec["n%d" % n] = per_n


def kernel_leg(n, rec):
  rng = np.random.default_rng(1)
  a = torch.from_numpy(rng.uniform(0.05, 0.95, (n, n))).cuda()
  op = refinement.CropDiagonal()
  for name, dtype, w in (("f64", torch.float64, 8), ("f32", torch.float32, 4),
                         ("f16", torch.float16, 2), ("bf16", torch.bfloat16, 2)):
    base = torch.empty(n, n + 8, dtype=dtype, device="cuda")
    for view in (torch.empty(n, n, dtype=dtype, device="cuda"),       # rows, 16-byte stores
                 base[:, 1:1 + n],                                    # rows, scalar stores
                 torch.empty(n, n, dtype=dtype, device="cuda").t(),   # tile, 16-byte stores
                 base.t()[1:1 + n, :n]):                              # tile, scalar stores
      for _ in range(3):
        op.refine(a, out=view)
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
    del x, y, base


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeat", type=int, default=3)
  ap.add_argument("--sizes", default="8192,2048")
  ap.add_argument("--legs", default=",".join(LEGS))
  ap.add_argument("--kernel", action="store_true")
  ap.add_argument("--out", default=None)
  ap.add_argument("--tag", default="")
  args = ap.parse_args()
  rec = {"tag": args.tag, "out_parameter": HAVE}
  if args.kernel:
    k = {}
    kernel_leg(8192, k)
    rec["kernel"] = {"n": 8192, "legs": k}
  else:
    rec["repeat"] = args.repeat
    timing([int(s) for s in args.sizes.split(",")], args.repeat, rec, args.legs.split(","))
  line = json.dumps(rec)
  print(line, flush=True)
  if args.out:
    with open(args.out, "a") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()
