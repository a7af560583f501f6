#!/usr/bin/env python
"""What labels and centroids cost a caller whose embeddings live on the GPU.

Legs (each: minimum and maximum ms over --repeat calls after a warm-up call):
  single_device_f32 / _f64   `get_cluster_centroids` at n = 8192, d = 256, k = 8 on device tensors,
                             the result into a device tensor;
  single_numpy_f64           NumPy float64 in, `out=None`: the untouched path;
  batch_long                 512 utterances of n in [300, 3000] (BASELINE config 5), d = 256,
                             device float32, as one `get_cluster_centroids_batch`;
  batch_short                512 utterances of n in [20, 128];
  predict / predict_out      `predict(x)` and `predict(x, out=labels)` at n = 8192, labels ending
                             in a device tensor either way.
On a build without `out=` (the parent commit) the same work is what a user of that build has to
write: `.cpu().numpy()`, `utils.get_cluster_centroids` per utterance,
`torch.from_numpy(...).to(device)`.
--kernel: instead, a few device-to-device calls at n = 8192 per dtype (for a `rocprofv3
--kernel-trace --stats` run) and a device-to-device copy of n * d * w bytes timed in the same
process.
--root DIR imports the package from another checkout (the parent commit's build).
One JSON line on stdout; --out appends it to a file (profiles/centroid_device_probe.jsonl).

  python tools/centroid_device_probe.py [--repeat 3] [--legs a,b] [--kernel] [--root DIR]
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

LEGS = ("single_device_f32", "single_device_f64", "single_numpy_f64", "batch_long", "batch_short",
        "predict", "predict_out")
N, D, K = 8192, 256, 8


def timed(call, repeat):
  ms = []
  for i in range(repeat + 1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    if i:
      ms.append(1e3 * (time.perf_counter() - t0))
  return {"min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def single(utils, have, dtype, repeat):
  rng = np.random.default_rng(1)
  x = torch.from_numpy(rng.standard_normal((N, D))).to(dtype).cuda()
  labels = torch.from_numpy(rng.integers(0, K, size=N)).cuda()
  out = torch.empty(K, D, dtype=dtype, device="cuda")
  if have:
    return timed(lambda: utils.get_cluster_centroids(x, labels, out=out), repeat)

  def parent():
    c = utils.get_cluster_centroids(x.cpu().numpy(), labels.cpu().numpy())
    out.copy_(torch.from_numpy(c).to("cuda"))
  return timed(parent, repeat)


def single_numpy(utils, repeat):
  rng = np.random.default_rng(1)
  x = rng.standard_normal((N, D))
  labels = rng.integers(0, K, size=N)
  return timed(lambda: utils.get_cluster_centroids(x, labels), repeat)


def batch(utils, have, low, high, repeat):
  rng = np.random.default_rng(5)
  xs, ls, outs = [], [], []
  for _ in range(512):
    n = int(rng.integers(low, high + 1))
    xs.append(torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).cuda())
    ls.append(torch.from_numpy(rng.integers(0, K, size=n)).cuda())
    outs.append(torch.empty(K, D, dtype=torch.float32, device="cuda"))
  if have:
    return timed(lambda: utils.get_cluster_centroids_batch(xs, ls, outs), repeat)

  def parent():
    for x, l, o in zip(xs, ls, outs):
      c = utils.get_cluster_centroids(x.cpu().numpy(), l.cpu().numpy())
      o[:c.shape[0]].copy_(torch.from_numpy(c).to("cuda"))
  return timed(parent, repeat)


def predict(sca, have_out, use_out, repeat):
  rng = np.random.default_rng(9)
  centres = rng.standard_normal((K, D)) * 3.0
  x = torch.from_numpy((centres[np.arange(N) % K] + rng.standard_normal((N, D))).astype(
      np.float32)).cuda()
  options = sca.RefinementOptions(gaussian_blur_sigma=1, p_percentile=0.95,
                                  refinement_sequence=sca.ICASSP2018_REFINEMENT_SEQUENCE)
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=16, refinement_options=options)
  labels = torch.empty(N, dtype=torch.int64, device="cuda")
  if use_out and have_out:
    return timed(lambda: c.predict(x, out=labels), repeat)
  if use_out:
    return timed(lambda: labels.copy_(torch.from_numpy(c.predict(x)).to("cuda")), repeat)
  return timed(lambda: c.predict(x), repeat)


def kernel_leg(utils, rec):
  rng = np.random.default_rng(1)
  values = rng.standard_normal((N, D))
  labels = torch.from_numpy(rng.integers(0, K, size=N)).cuda()
  for name, dtype, w in (("f64", torch.float64, 8), ("f32", torch.float32, 4),
                         ("f16", torch.float16, 2), ("bf16", torch.bfloat16, 2)):
    x = torch.from_numpy(values).to(dtype).cuda()
    out = torch.empty(K, D, dtype=dtype, device="cuda")
    for _ in range(3):
      utils.get_cluster_centroids(x, labels, out=out)
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
    rec[name] = {"source_bytes": N * D * w, "copy_ms_min": round(min(ms), 4),
                 "copy_GBps": round(2 * N * D * w / min(ms) / 1e6, 1)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeat", type=int, default=3)
  ap.add_argument("--legs", default=",".join(LEGS))
  ap.add_argument("--kernel", action="store_true")
  ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  ap.add_argument("--out", default=None)
  ap.add_argument("--tag", default="")
  args = ap.parse_args()
  sys.path.insert(0, os.path.abspath(args.root))
  import spectralcluster_amd as sca
  from spectralcluster_amd import utils
  have = "out" in inspect.signature(utils.get_cluster_centroids).parameters
  rec = {"tag": args.tag, "out_parameter": have}
  if args.kernel:
    k = {}
    kernel_leg(utils, k)
    rec["kernel"] = {"n": N, "d": D, "k": K, "legs": k}
  else:
    rec["repeat"] = args.repeat
    for leg in args.legs.split(","):
      if leg == "single_device_f32":
        rec[leg] = single(utils, have, torch.float32, args.repeat)
      elif leg == "single_device_f64":
        rec[leg] = single(utils, have, torch.float64, args.repeat)
      elif leg == "single_numpy_f64":
        rec[leg] = single_numpy(utils, args.repeat)
      elif leg == "batch_long":
        rec[leg] = batch(utils, have, 300, 3000, args.repeat)
      elif leg == "batch_short":
        rec[leg] = batch(utils, have, 20, 128, args.repeat)
      elif leg in ("predict", "predict_out"):
        rec[leg] = predict(sca, have, leg == "predict_out", args.repeat)
      else:
        raise SystemExit("unknown leg " + leg)
  line = json.dumps(rec)
  print(line, flush=True)
  if args.out:
    with open(args.out, "a") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()
