#!/usr/bin/env python
"""What it costs to cluster with a dense (n, n) constraint matrix the caller already holds.

Every leg is fed the same constraint matrices as NumPy float64, NumPy float32 and PyTorch tensors
on the GPU in float32 and float16 (the batch legs: NumPy float64 and device float32):
  single   ms per `predict(x, q)` at n = 4096 and 8192, d = 256, the Turn-to-Diarize preset:
           median, minimum and maximum over --repeat calls after a warm-up,
  batch    utterances/s over --count utterances of SURVEY.md's config 5 sizes (n in [300, 3000]),
           a dense symmetric constraint each, ConstraintPropagation before refinement,
  short    utterances/s over --short-count utterances of n in [20, 128]; best of --batch-repeat,
  band     the untouched path: the batch leg's utterances with a `ConstraintMatrix` each.
On a build with `DenseConstraints` the constraint goes in wrapped.  On a build without it (the
parent commit) the same work is the only way in that build has: a device tensor is downloaded and
widened on the host, a single call is `predict(x, q64)` and a batch the per-utterance loop
`predict_batch` falls back to for an ndarray constraint.
--kernel: instead of the legs above, ONE batch call of the batch and the short leg on device
float32 constraints, for a `rocprofv3 --kernel-trace --stats` run.
One JSON line on stdout; --out appends it to a file (profiles/constraint_input_probe.jsonl).

  python tools/constraint_input_probe.py [--sizes 4096,8192] [--repeat 5] [--batch-repeat 2]
                                         [--count 64] [--short-count 512] [--kernel]
                                         [--out FILE] [--tag NAME]
"""
import argparse
import copy
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

HAVE = hasattr(sca, "DenseConstraints")


def dense_q(truth, seed):
  """+1 / -1 on a third of all pairs (same / another speaker), a few fractional weights."""
  n = len(truth)
  rng = np.random.default_rng(seed)
  sign = np.where(truth[:, None] == truth[None, :], 1.0, -1.0)
  weight = rng.choice([1.0, 1.0, 1.0, 0.5, 0.25, 0.75], size=(n, n))
  q = np.where(rng.random((n, n)) < 1.0 / 3.0, sign * weight, 0.0)
  return np.triu(q) + np.triu(q, 1).T


def legs(qs, only=None):
  out = {"numpy_f64": qs, "numpy_f32": [q.astype(np.float32) for q in qs]}
  for name, dtype in (("device_f32", torch.float32), ("device_f16", torch.float16)):
    if not only or name in only:
      out[name] = [torch.from_numpy(q).to(dtype).cuda() for q in qs]
  torch.cuda.synchronize()
  return {k: v for k, v in out.items() if not only or k in only}


def wrap(q):
  if HAVE:
    return sca.DenseConstraints(q)
  if isinstance(q, np.ndarray):
    return q.astype(np.float64, copy=False)
  return q.cpu().double().numpy()  # what a user of that build has to do


def batch_clusterer():
  options = sca.RefinementOptions(
      p_percentile=0.9, thresholding_type=sca.ThresholdType.Percentile,
      thresholding_with_binarization=True, thresholding_preserve_diagonal=True,
      symmetrize_type=sca.SymmetrizeType.Average,
      refinement_sequence=sca.TURNTODIARIZE_REFINEMENT_SEQUENCE)
  return sca.SpectralClusterer(
      min_clusters=2, max_clusters=7, refinement_options=options,
      laplacian_type=sca.LaplacianType.GraphCut, row_wise_renorm=True,
      constraint_options=sca.ConstraintOptions(
          constraint_name=sca.ConstraintName.ConstraintPropagation, apply_before_refinement=True,
          constraint_propagation_alpha=0.4))


def single(n, repeat, rec):
  x, truth, _ = so.turn_blobs(n, 256, 4, seed=n, noise=0.2)
  for name, (q,) in legs([dense_q(truth, n)]).items():
    ms = []
    for i in range(repeat + 1):
      c = copy.deepcopy(sca.configs.turntodiarize_clusterer)  # (AutoTune keeps state)
      t0 = time.perf_counter()
      c.predict(x, wrap(q))
      if i:  # (the first call warms up)
        ms.append(1e3 * (time.perf_counter() - t0))
    rec[name] = {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
                 "max_ms": round(max(ms), 3)}


def batch(us, forms, repeat, rec, names):
  c = batch_clusterer()
  for name in names:
    cs = forms[name]

    def run():
      t0 = time.perf_counter()  # (on the parent the download and the widening are in the time)
      c.predict_batch(us, constraint_matrices=cs if name == "band" else [wrap(q) for q in cs])
      return len(us) / (time.perf_counter() - t0)

    run()  # warm-up
    best = max([run() for _ in range(repeat)] or [0.0])
    routes = list(c.last_batch_routes)
    rec[name] = {"utterances_per_s": round(best, 1),
                 "routes": {r: routes.count(r) for r in (0, 1, 2)}}


def inputs(sizes, d, seed0):
  xs, truths, scores = [], [], []
  for i, n in enumerate(sizes):
    x, truth, sc = so.turn_blobs(int(n), d, 2 + i % 3, seed=seed0 + i, noise=0.2)
    xs.append(np.ascontiguousarray(x)), truths.append(truth), scores.append(sc)
  return xs, truths, scores


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--sizes", default="4096,8192")
  ap.add_argument("--repeat", type=int, default=5)
  ap.add_argument("--batch-repeat", type=int, default=2)
  ap.add_argument("--count", type=int, default=64)
  ap.add_argument("--short-count", type=int, default=512)
  ap.add_argument("--kernel", action="store_true")
  ap.add_argument("--out", default=None)
  ap.add_argument("--tag", default="")
  args = ap.parse_args()
  rec = {"tag": args.tag, "dense_constraints": HAVE}
  rng = np.random.default_rng(512)
  big_ns = rng.integers(300, 3001, 512)[:args.count]
  short_ns = rng.integers(20, 129, args.short_count)
  for key, sizes, d, seed0 in (("batch", big_ns, 64, 0), ("short", short_ns, 32, 9000)):
    if len(sizes) == 0:
      continue
    us, truths, scores = inputs(sizes, d, seed0)
    qs = [dense_q(t, seed0 + i) for i, t in enumerate(truths)]
    forms = legs(qs, only=("numpy_f64", "device_f32") if not args.kernel else ("device_f32",))
    forms["band"] = [sca.ConstraintMatrix(list(sc), 1) for sc in scores]
    names = ["device_f32"] if args.kernel else ["numpy_f64", "device_f32"]
    if key == "batch" and not args.kernel:
      names.append("band")
    out = {}
    batch(us, forms, 0 if args.kernel else args.batch_repeat, out, names)
    rec[key] = {"utterances": len(us), "n": [int(min(sizes)), int(max(sizes))], "legs": out}
    del forms
  if not args.kernel:
    rec["single"] = {}
    for n in [int(v) for v in args.sizes.split(",") if v]:
      one = {}
      single(n, args.repeat, one)
      rec["single"][str(n)] = {"repeat": args.repeat, "legs": one}
  line = json.dumps(rec)
  print(line, flush=True)
  if args.out:
    with open(args.out, "a") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()
