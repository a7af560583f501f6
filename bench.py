#!/usr/bin/env python
"""Benchmark of the hot path: SpectralClusterer.predict() calls/s on MI355X.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N > 1 the
driver launches one rank per GPU with `python -m torch.distributed.run` (this file reads
RANK / LOCAL_RANK / WORLD_SIZE / MASTER_PORT from the environment; it does not import
torch -- ranks meet over RCCL through the C ABI, `sc_comm_*`).  Prints ONE JSON line on
rank 0.

Headline workload (BASELINE.json configs[2], the one `metric` is quoted on): n=8192 d=256
synthetic Gaussian blobs (8 speakers), ICASSP2018 refinement, GraphCut Laplacian,
eigengap k in [2, 20], cosine k-means.  One "step" = one `sc_predict` -- the call
`SpectralClusterer.predict()` makes: H2D of X (16.8 MB from a pageable numpy buffer), the
whole device pipeline, D2H of the labels.  The same K steps through `sc_run_resident`
(embeddings already in HBM: the same pipeline without the H2D) are reported as `resident`.
Multi-GPU = independent replicas (every rank runs the same per-GPU work, no data-path
collective, weak scaling).

Extra keys (not the headline): `batch512` = BASELINE config 5 (512 utterances, n in
[300, 3000], LPT-partitioned over the ranks, one grouped batch per rank -- 16 utterances per launch,
three lanes -- labels all-gathered; the multi-stream form and the plain loop are
timed beside it) in utterances/s, and `autotune16` = config 4 (16-value p_percentile sweep at
n=4096, grid round-robin over the ranks) in ms per sweep -- the quantities the 8-GPU
target is stated on; both carry their own `roofline` (algorithmic flops + HBM bytes -> floor)
and, on one GPU, `projected`: every rank's share of a world of 2 / 4 / 8 timed on its own on
this GPU (what N GPUs would give, fixed per-rank costs included).  `hard8192` = the headline
configuration on UNSTRUCTURED N(0, I) embeddings (clustered spectrum: which eigen path
finished, passes, restart cycles).  `autotune16_ttd` = config 4's Turn-to-Diarize variant.
`--workload batch512|autotune16` makes one of them the `value`.

A plain run does only what the headline needs: set-up, W warm-up steps, the K timed steps, the
result line (`metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step`, ...).
Everything else above -- `resident`, the per-kernel and whole-call rooflines, the explicit fp64
Diffuse route, the workload legs and their projections, the concurrent / pipelined legs, the CPU
baselines, the parity checks against the stored reference labels -- runs with `--full`.
`--dump-outputs DIR` writes what the last timed step returned as float64 .npy files: `labels`
(n) and `eigenvalues` (the leading eigenvalues the call reports); the inputs are seeded, so two
builds run with the same arguments can be compared output for output.
"""

import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# the grouped batch (config 5) keeps nine streams busy: eight hardware queues instead of the
# runtime's four.  Must be in the environment before the first HIP call.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

N_SAMPLES, N_FEATURES, N_SPEAKERS, SEED = 8192, 256, 8, 0
MAX_CLUSTERS = 20
PEAK_F64_MFMA_TFLOPS = 78.6   # MI355X fp64 matrix peak
PEAK_I8_MFMA_TOPS = 5000.0    # MI355X int8 matrix peak, dense: 2x the bf16 rate (MI355X_MICROARCH.md:
                              # "I8 ~2x bf16 rate", bf16 ~2.5 PF dense; microbenchmarked 4404)
PEAK_HBM_TBS = 8.0            # MI355X HBM3E (MI355X_MICROARCH.md)
ACHIEVABLE_HBM_TBS = 6.3      # what a streaming copy reaches (MI355X_MICROARCH.md: 6.29 measured)
GEMM_TILE = 128               # gemm_f64.hip block tile


def blobs(n, d, k, seed, noise=0.3):
  """SURVEY.md section 8(d) generator (same as oracle/spectral_oracle.blobs)."""
  rng = np.random.default_rng(seed)
  centers = rng.standard_normal((k, d))
  lab = np.sort(rng.integers(0, k, n))
  return np.ascontiguousarray(centers[lab] + noise * rng.standard_normal((n, d))), lab


def ari(a, b):
  """Adjusted Rand index (Hubert & Arabie 1985) from the contingency table."""
  a = np.asarray(a).ravel()
  b = np.asarray(b).ravel()
  _, ai = np.unique(a, return_inverse=True)
  _, bi = np.unique(b, return_inverse=True)
  table = np.zeros((ai.max() + 1, bi.max() + 1), dtype=np.int64)
  np.add.at(table, (ai, bi), 1)
  pairs = lambda t: int((t * (t - 1) // 2).sum())
  both, rows, cols = pairs(table), pairs(table.sum(axis=1)), pairs(table.sum(axis=0))
  total = a.size * (a.size - 1) // 2
  expected = rows * cols / total if total else 0.0
  top = 0.5 * (rows + cols)
  return 1.0 if top == expected else float((both - expected) / (top - expected))


def host_cpu():
  model = platform.processor() or "unknown"
  try:
    with open("/proc/cpuinfo") as f:
      for line in f:
        if line.startswith("model name"):
          model = line.split(":", 1)[1].strip()
          break
  except OSError:
    pass
  try:
    from threadpoolctl import threadpool_info
    threads = max([p.get("num_threads", 1) for p in threadpool_info()] or [1])
  except Exception:  # pylint: disable=broad-except
    threads = os.cpu_count() or 1
  return model, os.cpu_count() or 1, int(threads)


def promote_as_run(roofline, floor_s, elapsed, note):
  """The roofline of a leg whose utterances / values take the matrix-free Diffuse: the TOP-level
  floor_ms / frac price the route that runs (a fraction above 1 against the
  explicit route's floor is not a roofline fraction); the explicit route's figures -- the
  yardstick of rounds 1-3 -- move to `explicit_route`."""
  explicit = {"note": "what the same work would cost with the n^3 fp64 Diffuse product (the "
                      "yardstick of rounds 1-3); not the route that runs"}
  for key in ("floor_ms", "frac", "frac_at_achievable_hbm", "flops", "hbm_bytes",
              "achieved_tflops", "floor_terms"):
    if key in roofline:
      explicit[key] = roofline.pop(key)
  roofline["explicit_route"] = explicit
  roofline["floor_ms"] = 1e3 * floor_s
  roofline["frac"] = floor_s / elapsed
  roofline["route"] = "as run: " + note
  return roofline


def cpu_baseline_legs(gpu_clusterer, full_size=True):
  """Two CPU legs on the host cores, on a BOUNDED sample of the headline workload
  (n=2048 instead of 8192: the full size costs ~160 s per call; cost ~ n^3):
    port               -- oracle/spectral_oracle.predict: the reference's algorithm
                          (np.linalg.eig on the non-symmetric n x n matrix);
    algorithm_matched  -- oracle/spectral_oracle.predict_algorithm_matched: the DEVICE
                          path's algorithm on the CPU (folded scaling vectors + scipy eigsh
                          on the symmetric operator), so the hardware speed-up is not
                          conflated with the dgeev -> Lanczos algorithmic win."""
  sys.path.insert(0, os.path.join(ROOT, "oracle"))
  import spectral_oracle as so
  n_s = 2048
  x = so.blobs(n_s, N_FEATURES, N_SPEAKERS, SEED)
  cfg = so.icassp2018_config(laplacian_type=so.LAPLACIAN_GRAPH_CUT,
                             max_clusters=MAX_CLUSTERS)
  model, nproc, threads = host_cpu()

  def timed(fn, budget_s, max_reps):
    reps, spent, result = 0, 0.0, None
    while reps < max_reps and spent < budget_s:
      t0 = time.perf_counter()
      result = fn()
      spent += time.perf_counter() - t0
      reps += 1
    return spent / reps, reps, result

  port_s, port_reps, port_labels = timed(lambda: so.predict(x, cfg), 20.0, 3)
  # the CPU number beside the headline on the SAME configuration and the same box:
  # the oracle port once at n = 8192 (np.linalg.eig of an 8192 x 8192 matrix: ~200 s on the GPU
  # box's 64 cores).  Skipped (and said so) when the n = 2048 sample predicts more than 15 minutes
  # -- its n^3 extrapolation divided by the 2.5 it has overstated by on every box so far -- or
  # with --cpu-baseline-sample-only.
  full = None
  if full_size:
    est = port_s * (N_SAMPLES / float(n_s)) ** 3
    if est <= 900.0 * 2.5:  # (the n^3 extrapolation overstates 2-3x: dgeev is not the only term)
      xf = so.blobs(N_SAMPLES, N_FEATURES, N_SPEAKERS, SEED)
      t0 = time.perf_counter()
      full_labels = so.predict(xf, cfg)
      full = {"seconds_per_call": time.perf_counter() - t0, "labels": full_labels, "x": xf}
    else:
      full = {"skipped": "the n=%d sample (%.1f s) predicts ~%.0f s at n=%d" % (
          n_s, port_s, est / 2.5, N_SAMPLES)}
  am_s, am_reps, (am_labels, _) = timed(lambda: so.predict_algorithm_matched(x, cfg),
                                        10.0, 5)
  # the GPU sat idle for ~30 s of CPU legs: the first call meets idle clocks.  Report that
  # latency on its own, then warm the device (>= 50 ms of work) before timing the sample.
  t0 = time.perf_counter()
  gpu_clusterer.predict(x)
  first_after_idle_s = time.perf_counter() - t0
  t0 = time.perf_counter()
  while time.perf_counter() - t0 < 0.25:
    gpu_clusterer.predict(x)
  reps = 50
  t0 = time.perf_counter()
  for _ in range(reps):
    glab = gpu_clusterer.predict(x)
  gpu_s = (time.perf_counter() - t0) / reps
  common = {"unit": "calls/s", "cores": threads, "cpu_model": model, "nproc": nproc,
            "gpu_same_sample_calls_per_s": 1.0 / gpu_s,
            "gpu_first_call_after_idle_ms": 1e3 * first_after_idle_s}
  sample_row = {"value": 1.0 / port_s, "seconds_per_call": port_s,
                "sample": ("oracle/spectral_oracle.predict (np.linalg.eig) on n=%d d=%d k=%d "
                           "blobs, same config; %d reps" % (n_s, N_FEATURES, N_SPEAKERS, port_reps)),
                "gpu_same_sample_calls_per_s": 1.0 / gpu_s,
                "ari_gpu_vs_cpu_sample": ari(glab, port_labels)}
  if full is not None and "seconds_per_call" in full:
    # the headline configuration itself: value / sample describe THIS run; the n = 2048 sample
    # stays as a second key
    gfull = gpu_clusterer.predict(full["x"])
    port = dict(common, value=1.0 / full["seconds_per_call"], kind="port",
                sample=("oracle/spectral_oracle.predict (np.linalg.eig) on the headline "
                        "configuration itself: n=%d d=%d k=%d blobs, GraphCut, max_clusters=%d; "
                        "one call" % (N_SAMPLES, N_FEATURES, N_SPEAKERS, MAX_CLUSTERS)),
                seconds_per_call=full["seconds_per_call"],
                ari_gpu_vs_cpu_sample=ari(gfull, full["labels"]),
                n2048_sample=sample_row)
    port["gpu_same_sample_calls_per_s"] = None  # (the headline `value` of this record is that figure)
  else:
    port = dict(common, kind="port", **sample_row)
    port["n8192_note"] = (
        (full or {}).get("skipped", "--cpu-baseline-sample-only") + "; the reference itself at "
        "n=8192 (same config, this repo's golden generator, 8 vCPU container): "
        "parity.reference_seconds_per_call_8vcpu")
  matched = dict(common, value=1.0 / am_s, kind="algorithm_matched",
                 sample=("oracle/spectral_oracle.predict_algorithm_matched (NumPy refinement, "
                         "scaling vectors folded, scipy.sparse.linalg.eigsh k=%d on the symmetric "
                         "operator) on the same n=%d sample; %d reps"
                         % (MAX_CLUSTERS + 1, n_s, am_reps)),
                 seconds_per_call=am_s,
                 ari_vs_port_labels=ari(am_labels, port_labels),
                 ari_gpu_vs_cpu_sample=ari(glab, am_labels))
  return port, matched


def concurrent_leg(_lib, cfg, x, steps, streams=2):
  """Throughput of independent predict() calls issued from `streams` host threads on
  `streams` handles (HIP streams) of the same GPU: the single-workgroup phases of one
  call overlap the GEMM of the other.  Extra information only."""
  import threading
  pool = _lib.handle_pool(None, streams)
  n, d = x.shape
  per = max(1, steps // streams)
  ready = []
  for h in pool:
    lab = np.empty(n, dtype=np.int64)
    diag = _lib.ScDiag()
    h.check(h.lib.sc_set_embeddings(h.raw, _lib.as_double_p(x), n, d))
    h.check(h.lib.sc_run_resident(h.raw, cfg, _lib.as_int64_p(lab), diag))  # warm-up
    ready.append((h, lab, diag))

  def run(h, lab, diag):
    for _ in range(per):
      h.check(h.lib.sc_run_resident(h.raw, cfg, _lib.as_int64_p(lab), diag))

  for h, _, _ in ready:
    h.check(h.lib.sc_synchronize(h.raw))
  t0 = time.perf_counter()
  threads = [threading.Thread(target=run, args=r) for r in ready]
  for t in threads:
    t.start()
  for t in threads:
    t.join()
  dt = time.perf_counter() - t0
  return {"streams": streams, "calls": per * streams, "value": per * streams / dt,
          "unit": "calls/s"}


def pipelined_leg(_lib, handle, cfg, x, steps):
  """Throughput of `steps` independent predict() calls handed over as ONE batch
  (sc_predict_batch): the upload of call i + 1 rides under call i's pipeline (helper thread, copy
  stream, two embeddings buffers: api.hip predict_sequence).  Four distinct utterances (the
  headline's generator, other seeds) in turn;
  every call uploads its 16.8 MB.  The per-call latency is the headline's; this is calls/s."""
  import ctypes
  n, d = x.shape
  hosts = [x] + [blobs(n, d, N_SPEAKERS, SEED + 100 + i)[0] for i in range(3)]
  count = max(4, steps)
  xs = [hosts[i % 4] for i in range(count)]
  labs = [np.empty(n, dtype=np.int64) for _ in range(count)]
  xp = (ctypes.POINTER(ctypes.c_double) * count)(*[_lib.as_double_p(u) for u in xs])
  lp = (ctypes.POINTER(ctypes.c_int64) * count)(*[_lib.as_int64_p(l) for l in labs])
  ns = (ctypes.c_int * count)(*([n] * count))
  diags = (_lib.ScDiag * count)()

  def run(streams):
    handle.check(handle.lib.sc_predict_batch_streams(handle.raw, xp, ns, d, count, cfg, lp, diags,
                                                     streams))

  out = {"calls": count, "unit": "calls/s",
         "step": "sc_predict_batch_streams of %d x (n=%d, d=%d): every call's H2D inside, "
                 "overlapped with the previous call's kernels" % (count, n, d)}
  for streams in (1, 2):
    run(streams)  # warm-up (buffers, copy streams)
    handle.check(handle.lib.sc_synchronize(handle.raw))
    t0 = time.perf_counter()
    run(streams)
    dt = time.perf_counter() - t0
    key = "value" if streams == 1 else "value_two_streams"
    out[key] = count / dt
    out["ms_per_call" if streams == 1 else "ms_per_call_two_streams"] = 1e3 * dt / count
  out["labels_equal_first_and_fifth"] = bool(np.array_equal(labs[0], labs[4])) if count > 4 else None
  out["note"] = ("value: one stream (one pipeline at a time, uploads underneath); "
                 "value_two_streams: two handles / streams / host threads, each with its own "
                 "prefetched sequence -- one call's launch-bound eigen and k-means chains under "
                 "the other's streaming kernels")
  return out


def batch512_sizes():
  """BASELINE config 5 (same draw as oracle/make_golden.batch512_inputs)."""
  rng = np.random.default_rng(512)
  return rng.integers(300, 3001, 512), rng.integers(2, 8, 512)


def tri_tiles(n):
  nt = (n + GEMM_TILE - 1) // GEMM_TILE
  return nt * (nt + 1) // 2


FREE_MIN_N = 2048  # default route switch of the matrix-free Diffuse (free_api.hip): single calls
FREE_MIN_N_GROUP = 1536  # ... members of a grouped batch (switches.h)


def icassp_floor_seconds(n, d, passes, free_min_n=FREE_MIN_N):
  """Floor of one ICASSP2018 predict() AS IT RUNS: the explicit route below FREE_MIN_N
  (`icassp_work`), the matrix-free route from there on -- n^2 d fp64 flops + 4 n^3 int8 ops
  (upper triangle, 2 ops per MAC) at their MFMA peaks; A1 write, Crop+Blur R/W, Thr+Sym R/W,
  n^2 * 2 B of digits (written by the Thr+Sym pass: no read of their own), T written and read
  once as fp32 upper-triangle tiles, one read of A for the exact statistics, 2 x passes
  half-matrix products; 8 TB/s."""
  nn = float(n) * n
  if n < free_min_n:
    flops, hbm = icassp_work(n, d, passes)
    return flops / (PEAK_F64_MFMA_TFLOPS * 1e12) + hbm / (PEAK_HBM_TBS * 1e12)
  mat = nn * 8.0
  hbm = 5.0 * mat + nn * 2.0 + 2 * nn * 2.0 + mat + 2.0 * passes * 0.5 * mat + n * d * 8.0
  return (nn * d / (PEAK_F64_MFMA_TFLOPS * 1e12) + 4.0 * nn * n / (PEAK_I8_MFMA_TOPS * 1e12) +
          hbm / (PEAK_HBM_TBS * 1e12))


def icassp_work(n, d, passes):
  """Algorithmic work of one ICASSP2018 predict() (fused lower bound): the
  two products with their symmetry exploited, n^2 (n + d) flops (no tile rounding: padding a
  300-row utterance to 384 is the implementation's cost, not the problem's); A1 write,
  Crop+Blur R/W, Threshold+Symmetrize R/W, Diffuse R/W (normalise + Laplacian folded) = 7
  n^2 passes, plus one per executed block matvec."""
  flops = float(n) * n * (n + d)
  hbm = (7.0 + passes) * n * n * 8.0 + n * d * 8.0
  return flops, hbm


def workload_roofline(flops, hbm_bytes, seconds):
  """A whole workload against its floor: MFMA time of its flops + HBM time of its
  algorithmic bytes at the 8 TB/s peak (the stages are data-dependent, so the two add).
  `frac_at_achievable_hbm` prices the bytes at the 6.3 TB/s a streaming copy reaches."""
  mfma_s = flops / (PEAK_F64_MFMA_TFLOPS * 1e12)
  floor = mfma_s + hbm_bytes / (PEAK_HBM_TBS * 1e12)
  floor63 = mfma_s + hbm_bytes / (ACHIEVABLE_HBM_TBS * 1e12)
  return {"flops": flops, "hbm_bytes": hbm_bytes, "floor_ms": 1e3 * floor,
          "measured_ms": 1e3 * seconds, "achieved_tflops": flops / seconds / 1e12,
          "frac": floor / seconds, "frac_at_achievable_hbm": floor63 / seconds,
          "floor_terms": "flops / %.1f TF/s (fp64 MFMA peak) + bytes / %.1f TB/s (HBM3E peak); "
                         "frac_at_achievable_hbm uses %.1f TB/s (measured streaming copy)"
                         % (PEAK_F64_MFMA_TFLOPS, PEAK_HBM_TBS, ACHIEVABLE_HBM_TBS)}


def batch512_leg(sca, multigpu, comm, fence, group=16, streams=8, project=True):
  """Config 5: the 512 utterances are LPT-partitioned over the ranks by size alone, so each
  rank only synthesises its own share and uploads it itself; per rank ONE grouped batch
  (`group` utterances per launch, three lanes); labels all-gathered.  The multi-stream form
  (one host thread and arena per stream) is timed beside it."""
  ns, ks = batch512_sizes()
  sizes = [int(n) for n in ns]
  owned = multigpu.lpt_assignment(sizes, comm.size)[comm.rank]
  everything = comm.size == 1 and project
  have = range(512) if everything else owned
  mine = {i: blobs(sizes[i], N_FEATURES, int(ks[i]), seed=i)[0] for i in have}
  clusterer = sca.configs.icassp2018_clusterer

  def timed(reps=1, **how):
    clusterer.predict_batch([mine[i] for i in owned], **how)  # the WHOLE share: warm arenas
    secs = []
    for _ in range(reps):
      fence()
      t0 = time.perf_counter()
      labels = multigpu.predict_batch_sharded(
          comm, None, mine, sizes=sizes,
          predict_many_fn=lambda share: clusterer.predict_batch(share, **how))
      fence()
      secs.append(comm.allreduce_max(time.perf_counter() - t0))
    return labels, float(np.median(secs)), secs

  _, t_streams, _ = timed(streams=streams)
  _, t_loop, _ = timed(streams=1)
  # (three host threads share the chip inside a grouped batch: the median of three passes)
  labels, elapsed, passes_s = timed(reps=3, group=group)
  diags = clusterer.last_batch_diags
  passes = {i: int(dg.eig_matvec_passes) for i, dg in zip(owned, diags)}
  out = {"value": 512 / elapsed, "unit": "utterances/s", "seconds": elapsed,
         "mode": "grouped: three lanes (host threads) per GPU, %d utterances per launch; median "
                 "of 3 passes" % group,
         "passes_seconds": passes_s,
         "utterances": 512, "n_gpus": comm.size,
         "scaling": "strong", "partition": "LPT on multigpu.cost_model",
         "multi_stream": {"value": 512 / t_streams, "streams_per_gpu": streams,
                          "host_threads_per_gpu": streams},
         "plain_loop": {"value": 512 / t_loop}}
  if comm.size == 1:
    flops = hbm = 0.0
    for i in owned:
      f, b = icassp_work(sizes[i], N_FEATURES, passes[i])
      flops += f
      hbm += b
    out["roofline"] = workload_roofline(flops, hbm, elapsed)
    out["roofline"]["matvec_passes_mean"] = float(np.mean(list(passes.values())))
    as_run = sum(icassp_floor_seconds(sizes[i], N_FEATURES, passes[i], FREE_MIN_N_GROUP)
                 for i in owned)
    promote_as_run(out["roofline"], as_run, elapsed,
                   "utterances of n >= %d take the matrix-free Diffuse: their floor is the int8 "
                   "digit product + the extra passes over A instead of the fp64 product"
                   % FREE_MIN_N_GROUP)
  gpath = os.path.join(ROOT, "tests", "golden", "batch512.npz")
  if comm.rank == 0 and os.path.exists(gpath):
    g = np.load(gpath)
    ref, pos, ok = g["labels"], 0, 0
    for i, n in enumerate(sizes):
      ok += ari(labels[i], ref[pos:pos + n]) == 1.0
      pos += n
    out["ari1_vs_reference_labels"] = int(ok)
  if everything:
    out["projected"] = project_shares(
        lambda world: multigpu.lpt_assignment(sizes, world),
        lambda share: clusterer.predict_batch([mine[i] for i in share], group=group),
        elapsed, fence,
        "each rank's LPT share of the 512 utterances as its own predict_batch(group=%d) on "
        "this one GPU (median over 3 interleaved rounds per share, like the whole job's time): arenas warm (a "
        "long-lived server process), pageable H2D of the share and the group pipeline's "
        "fill/drain inside; the all-gather of < 1 MB of labels is not" % group)
  return out


def project_shares(partition, run_share, t_whole, fence, note):
  """What a world of 2 / 4 / 8 GPUs would give, measured on ONE: every rank's share runs on
  its own here (they are independent), so the job takes max over ranks of the share times.
  `sum_share_s` > `t_whole` is the fixed per-rank cost that strong scaling does not divide."""
  rows = {}
  for world in (2, 4, 8):
    # Three ROUNDS over all shares, the median per share (like `t_whole`, the median of three
    # passes of the whole job).  Interleaved, not three passes of one share back to back: a
    # transient of some tens of milliseconds on the box (host scheduling, clocks) then meets
    # different shares in different rounds instead of all three trials of one -- a single pass
    # of a 12 ms share, or three in a row, put one share at 14-19 ms in about every second run,
    # and the maximum over 8 shares collects it.
    shares = partition(world)
    trials = [[] for _ in shares]
    for _ in range(3):
      for idx, share in enumerate(shares):
        if not share:
          trials[idx].append(0.0)
          continue
        fence()
        t0 = time.perf_counter()
        run_share(share)
        fence()
        trials[idx].append(time.perf_counter() - t0)
    secs = [float(np.median(t)) for t in trials]
    rows[str(world)] = {"max_share_s": max(secs), "sum_share_s": sum(secs),
                        "share_ms": [round(1e3 * v, 2) for v in secs],
                        "imbalance": max(secs) / (sum(secs) / world),
                        "speedup": t_whole / max(secs)}
  rows["one_gpu_s"] = t_whole
  rows["method"] = note
  return rows


def autotune16_leg(sca, multigpu, comm, fence, variant="icassp", project=True):
  """Config 4: one AutoTune level of 16 p_percentile values at n=4096, the grid
  round-robin over the ranks, (ratio, n_clusters) all-gathered per level.  `variant`
  "ttd": the Turn-to-Diarize refinement (Percentile threshold + binarisation + preserved
  diagonal + Average symmetrisation, reference configs.py:49-59) under the same sweep."""
  n = 4096
  x, _ = blobs(n, N_FEATURES, N_SPEAKERS, 4096)

  def make():
    if variant == "ttd":
      opts = sca.RefinementOptions(
          p_percentile=0.95, thresholding_soft_multiplier=0.01,
          thresholding_type=sca.ThresholdType.Percentile,
          thresholding_with_binarization=True, thresholding_preserve_diagonal=True,
          symmetrize_type=sca.SymmetrizeType.Average,
          refinement_sequence=[sca.RefinementName.RowWiseThreshold,
                               sca.RefinementName.Symmetrize])
    else:
      opts = sca.RefinementOptions(
          gaussian_blur_sigma=1, p_percentile=0.95, thresholding_soft_multiplier=0.01,
          refinement_sequence=sca.ICASSP2018_REFINEMENT_SEQUENCE)
    return sca.SpectralClusterer(
        min_clusters=2, max_clusters=MAX_CLUSTERS, laplacian_type=sca.LaplacianType.GraphCut,
        refinement_options=opts, row_wise_renorm=variant == "ttd",
        autotune=sca.AutoTune(p_percentile_min=0.55, p_percentile_max=0.95,
                              init_search_step=0.025, search_level=1))

  multigpu.predict_autotune_distributed(comm, make(), x)  # warm-up
  reps = 3
  fence()
  t0 = time.perf_counter()
  for _ in range(reps):
    c = make()
    labels = multigpu.predict_autotune_distributed(comm, c, x)
  fence()
  elapsed = comm.allreduce_max(time.perf_counter() - t0) / reps
  out = {"value": 1e3 * elapsed, "unit": "ms/sweep", "p_values": 16, "n_samples": n,
         "n_gpus": comm.size, "scaling": "strong", "refinement": variant,
         "final_p": float(c.refinement_options.p_percentile),
         "best_p": float(c.last_best_p)}
  sweep = getattr(c, "last_sweep_diags", None)
  if comm.size == 1 and sweep:
    # one sweep: affinity (1 product, 1 n^2 write), [Crop+Blur once: 2 n^2], then per value
    # threshold+symmetrise (2 n^2) [+ Diffuse: 1 product, 2 n^2] + its matvec passes; the
    # winner's eigenvectors are adopted from the sweep; k-means is O(n k)
    mat = n * n * 8.0
    prod = float(n) * n  # flops per unit of K of a symmetric product (n^2 K)
    per_value_passes = [int(d.eig_matvec_passes) for d in sweep]
    diffuse = variant != "ttd"
    evals = len(sweep)
    flops = prod * N_FEATURES + (evals * prod * n if diffuse else 0.0)
    hbm = (mat + n * N_FEATURES * 8.0 + (2 * mat if diffuse else 0.0) +
           evals * (2 * mat + (2 * mat if diffuse else 0.0)) + sum(per_value_passes) * mat)
    out["roofline"] = workload_roofline(flops, hbm, elapsed)
    out["roofline"]["matvec_passes_per_value"] = per_value_passes
    out["eig_paths"] = [int(d.eig_path) for d in sweep]
    if diffuse and n >= FREE_MIN_N:
      # as it runs: every value on the matrix-free Diffuse (floor_ms / frac above keep pricing
      # the explicit route, the yardstick of rounds 1-3)
      nn = float(n) * n
      hbm_free = (mat + n * N_FEATURES * 8.0 + 2 * mat +
                  evals * (2 * mat + mat + nn * 2.0 + 2 * nn * 2.0 + mat) +
                  sum(per_value_passes) * 2 * 0.5 * mat)
      floor = (prod * N_FEATURES / (PEAK_F64_MFMA_TFLOPS * 1e12) +
               evals * 4.0 * nn * n / (PEAK_I8_MFMA_TOPS * 1e12) + hbm_free / (PEAK_HBM_TBS * 1e12))
      promote_as_run(out["roofline"], floor, elapsed,
                     "matrix-free Diffuse per value: int8 digit product at 5 POP/s + its passes "
                     "over A; 2 half-matrix products per executed block pass")
  gname = "autotune_ttd_n4096.npz" if variant == "ttd" else "autotune_n4096.npz"
  gpath = os.path.join(ROOT, "tests", "golden", gname)
  if os.path.exists(gpath):
    g = np.load(gpath)
    out["final_p_reference"] = float(g["final_p"] if "final_p" in g else g["best_p"])
    out["best_p_reference"] = float(g["grid"][int(np.argmin(g["ratios"]))])
    out["ari_vs_reference_labels"] = ari(labels, g["labels"])
    out["reference_seconds_8vcpu"] = float(g["ref_seconds"])
  if comm.size == 1 and project:
    grid = list(make().autotune.get_percentile_range())
    c2 = make()
    handle = c2._handle()
    c2._upload(handle, x)

    from spectralcluster_amd import _lib
    parts = {}

    def run_share(ps, timed_parts=False):
      # what one rank does per sweep: upload + affinity, its values as one grouped sweep
      # (Crop + Blur once per rank inside), and -- on the rank that evaluated the winner only
      # -- adopting its eigenvectors + k-means (the labels are then broadcast: n int32)
      def lap(name, t0):
        if timed_parts:
          fence()
          parts[name] = parts.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()
      t = time.perf_counter()
      c2._upload(handle, x)
      t = lap("upload_affinity_s", t)
      c2._eig_sweep(handle, ps)
      t = lap("sweep_s", t)
      if out["best_p"] in [float(p) for p in ps]:
        dg = c2._adopt_or_evaluate(handle, out["best_p"])
        lab = np.empty(n, dtype=np.int64)
        handle.check(handle.lib.sc_cluster(handle.raw, c2.build_config(out["best_p"]),
                                           max(int(dg.n_clusters_raw), 2), _lib.as_int64_p(lab),
                                           dg))
        lap("winner_kmeans_s", t)

    run_share(grid)
    fence()
    t0 = time.perf_counter()
    run_share(grid)
    fence()
    whole = time.perf_counter() - t0
    out["projected"] = project_shares(
        lambda world: [grid[r::world] for r in range(world)], run_share, whole, fence,
        "each rank's round-robin share of the 16 values (upload + affinity + Crop/Blur are "
        "per rank; the winner's eigenvectors are adopted and clustered on the rank that "
        "evaluated it) on this one GPU; the all-gather of 16 x 2 doubles and the broadcast of "
        "n int32 labels are not")
    # where a rank's time goes at world = 8 (2 values per rank), summed over the 8 shares
    for share in [grid[r::8] for r in range(8)]:
      run_share(share, timed_parts=True)
    out["projected"]["world8_parts_sum_s"] = dict(parts)
  return out


def hard8192_leg(sca, _lib):
  """The headline configuration on UNSTRUCTURED embeddings (N(0, I), n=8192, d=256): the 21
  eigenvalues the GraphCut eigengap reads sit on the edge of a dense bulk.  predict() must
  return (np.linalg.eig always does); the record says what that costs and which path did it."""
  rng = np.random.default_rng(8192)
  x = np.ascontiguousarray(rng.standard_normal((N_SAMPLES, N_FEATURES)))
  c = sca.SpectralClusterer(
      min_clusters=2, max_clusters=MAX_CLUSTERS,
      refinement_options=sca.configs.icassp2018_refinement_options,
      laplacian_type=sca.LaplacianType.GraphCut)
  c.predict(x)
  reps = 2
  t0 = time.perf_counter()
  for _ in range(reps):
    labels = c.predict(x)
  ms = 1e3 * (time.perf_counter() - t0) / reps
  dg = c.last_diag
  names = {1: "dense Jacobi", 2: "block Lanczos", 5: "dense values + Lanczos vectors",
           6: "dense landing pad (tridiagonalisation + bisection + inverse iteration)"}
  return {"input": "N(0, I) embeddings, n=%d d=%d, default_rng(8192)" % (N_SAMPLES, N_FEATURES),
          "ms_per_call": ms, "unit": "ms/call", "eig_path": int(dg.eig_path),
          "eig_path_name": names.get(int(dg.eig_path), "?"),
          "eig_fallback_reason": int(dg.eig_fallback),
          "matvec_passes": int(dg.eig_matvec_passes), "restart_cycles": int(dg.eig_cycles),
          "basis": int(dg.eig_basis), "n_clusters_raw": int(dg.n_clusters_raw),
          "n_clusters": int(dg.n_clusters), "labels_used": int(np.unique(labels).size),
          "eig_ms": float(dg.stage_times_ms().get("eig", 0.0)),
          "leading_eigenvalues": [float(v) for v in dg.eigenvalue_array()[:6]]}


def kernel_roofline(stage_ms, passes):
  """Per-kernel roofline rows from the run's own hipEvent timers (sc_set_profiling(2)):
  algorithmic bytes / flops over the measured time."""
  n, d = N_SAMPLES, N_FEATURES
  nt = (n + GEMM_TILE - 1) // GEMM_TILE
  mat = n * n * 8.0
  rows = []

  def hbm(name, key, nbytes, note):
    us = 1e3 * stage_ms[key]
    if us > 0:
      tbs = nbytes / (us * 1e-6) / 1e12
      rows.append({"kernel": name, "bound": "hbm", "us": us, "bytes": nbytes,
                   "achieved": tbs, "peak": PEAK_HBM_TBS, "unit": "TB/s",
                   "frac": tbs / PEAK_HBM_TBS, "note": note})

  def mfma(name, key, flops, note):
    us = 1e3 * stage_ms[key]
    if us > 0:
      tf = flops / (us * 1e-6) / 1e12
      rows.append({"kernel": name, "bound": "mfma", "us": us, "flops": flops,
                   "achieved": tf, "peak": PEAK_F64_MFMA_TFLOPS, "unit": "TFLOP/s",
                   "frac": tf / PEAK_F64_MFMA_TFLOPS, "note": note})

  tri = nt * (nt + 1) // 2 * 2.0 * GEMM_TILE * GEMM_TILE
  if stage_ms.get("free_product", 0.0) > 0:
    # matrix-free Diffuse: the digit product runs on the int8 matrix cores
    us = 1e3 * stage_ms["free_product"]
    tiles_run = stage_ms.get("_tiles_run") or nt * (nt + 1) // 2
    ops = 4.0 * tiles_run * 2.0 * GEMM_TILE * GEMM_TILE * ((n + 63) // 64 * 64)
    tops = ops / (us * 1e-6) / 1e12
    rows.append({"kernel": "k_gemm_i8_sym (digit product of the matrix-free Diffuse)",
                 "bound": "mfma", "us": us, "flops": ops, "achieved": tops,
                 "peak": PEAK_I8_MFMA_TOPS, "unit": "TFLOP/s", "frac": tops / PEAK_I8_MFMA_TOPS,
                 "note": "int8 multiply-adds counted as 2 ops; 4 digit products (hh, hl, lh, ll) "
                         "of the %d upper-triangle tiles (of %d) on the skip list; includes "
                         "k_free_tile_flags and k_i8_tail_finish" % (tiles_run, nt * (nt + 1) // 2)})
    t32 = nt * (nt + 1) // 2 * GEMM_TILE * GEMM_TILE * 4.0
    nblk = (n + 63) // 64
    hbm("k_free_partials_reduce (row partials of the quantiser fused into threshold+symmetrise)",
        "free_quantize", n * nblk * 12.0 + n * 16.0,
        "the digits are written by k_threshold_symmetrize_digits; what is left is the sum of "
        "its per-block partials: n * n/64 * 12 B read")
    hbm("k_t32_candidates", "free_scan", t32 * tiles_run / (nt * (nt + 1) // 2),
        "1 read of the fp32 tiles of T that were computed (row maxima come from the product's epilogue)")
    hbm("k_free_row_stats (exact rowmax / rowsum of S)", "free_stats", 1.0 * mat,
        "one read of A: a row's candidates are itself or rows of its own cluster, read a moment "
        "earlier by their own workgroups (PMC: 546 MB from HBM per launch at n = 8192 = 1.02 n^2 "
        "* 8 B); y1 = A 1 comes from L2")
  else:
    mfma("k_gemm_nt<EpiNone,SYM> (Diffuse)", "diffuse", tri * n, "upper-triangle tiles")
  mfma("k_gemm_nt<EpiAffinity,SYM> (affinity)", "affinity_gemm", tri * d,
       "K=%d: write floor %.0f us" % (d, mat / (PEAK_HBM_TBS * 1e12) * 1e6))
  hbm("k_gaussian_blur_stream<4> (CropDiagonal+GaussianBlur)", "blur", 2 * mat,
      "1 read + 1 write of n^2")
  if stage_ms.get("free_product", 0.0) > 0:
    hbm("k_threshold_symmetrize_digits (RowWiseThreshold+Symmetrize + the digits of the "
        "matrix-free Diffuse)", "threshold_sym",
        2 * mat + n * n * 2.0 + n * ((n + 63) // 64) * 12.0,
        "1 read + 1 write of n^2 * 8 B + n^2 * 2 B of digits + the row partials")
  else:
    hbm("k_threshold_symmetrize (RowWiseThreshold+Symmetrize)", "threshold_sym", 2 * mat,
        "1 read + 1 write of n^2")
  # (matrix-free Diffuse: an operator application is two products with A)
  products = passes * (2 if stage_ms.get("free_product", 0.0) > 0 else 1)
  hbm("block matvec of the eigen stage", "matvec", products * mat,
      "%g products x n^2 * 8 B (SURVEY 8d's algorithmic figure)" % products)
  if rows and rows[-1]["kernel"].startswith("block matvec"):
    # what the kernel actually moves: it reads the upper-triangle tiles only (n >= 4096) and
    # writes + re-reads two 128 x 8 slabs per tile
    moved = products * tri_tiles(n) * (GEMM_TILE * GEMM_TILE * 8.0 + 2 * 2 * GEMM_TILE * 8 * 8.0)
    r = rows[-1]
    r["bytes_moved"] = moved
    r["moved_tbs"] = moved / (r["us"] * 1e-6) / 1e12
    r["moved_frac_of_peak"] = r["moved_tbs"] / PEAK_HBM_TBS
    r["bytes_moved_source"] = ("analytic: upper-triangle tiles + per-tile slabs; rocprofv3 "
                               "FETCH_SIZE x2 of the same kernel: profiles/r03_*_pmc*")
  return rows


def headline_record(args, world, elapsed, comm, multigpu):
  """The keys of the result line that a plain run and --full share: the headline figure of the
  K timed predict() calls and what it was measured on."""
  k = args.steps
  return {
      "metric": "predict() calls/sec, n=8192 d=256 ICASSP2018 (GraphCut, eigengap "
                "k in [2,20], cosine k-means)",
      "value": world * k / elapsed, "unit": "calls/s", "n_gpus": world, "steps": k,
      "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / k,
      "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
      "dtype": "f64", "data": "synthetic",
      "config": {"workload": "icassp2018_graphcut_n8192_d256_k8_max20",
                 "n_samples": N_SAMPLES, "n_features": N_FEATURES,
                 "speakers": N_SPEAKERS, "parallelism": "replicas x%d" % world,
                 "step": "sc_predict = SpectralClusterer.predict(): H2D of X (16.8 MB, "
                         "pageable numpy buffer), the device pipeline, D2H of the labels",
                 "collectives": ("none" if world == 1 else
                                 "RCCL via the C ABI (sc_comm_*)"
                                 if isinstance(comm, multigpu.RcclComm) else
                                 "TCP fallback (RCCL did not come up: %s)"
                                 % getattr(comm, "note", ""))},
  }


def select_workload(out, extras, workload):
  """--workload batch512 | autotune16: that leg's figure becomes `value` (the predict() figure
  moves to `headline_predict8192`; `ms_per_step` stays that of the K timed steps)."""
  out.update(extras)
  if workload == "predict8192":
    return
  leg = extras[workload]
  out["headline_predict8192"] = {"value": out["value"], "unit": out["unit"],
                                 "ms_per_step": out["ms_per_step"]}
  out["metric"] = ("BASELINE config 5: 512 utterances n in [300,3000] d=256, ICASSP2018"
                   if workload == "batch512" else
                   "BASELINE config 4: AutoTune 16-value sweep, n=4096 d=256, GraphCut")
  out["value"], out["unit"] = leg["value"], leg["unit"]
  out["scaling"] = "strong"
  out["higher_is_better"] = workload == "batch512"
  out["config"]["workload"] = workload


def dump_outputs(directory, **arrays):
  """--dump-outputs: each array as DIR/<name>.npy in float64 (labels and eigenvalues of one
  n = 8192 call: 64 KB and 1 KB)."""
  os.makedirs(directory, exist_ok=True)
  for name, a in arrays.items():
    np.save(os.path.join(directory, name + ".npy"), np.asarray(a, dtype=np.float64))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--gpus", type=int, default=None,
                  help="ranks (one per GPU of this node).  Under a launcher (WORLD_SIZE set) it "
                       "must equal the world size; without one, N > 1 starts the N ranks itself")
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--workload", default="predict8192",
                  choices=["predict8192", "batch512", "autotune16"])
  ap.add_argument("--full", action="store_true",
                  help="everything beside the headline: resident path, rooflines, explicit "
                       "Diffuse route, workload legs and projections, concurrent / pipelined "
                       "legs, CPU baselines, parity against the stored reference labels")
  ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                  help="write the last timed step's outputs to DIR/<name>.npy (float64)")
  ap.add_argument("--no-cpu-baseline", action="store_true", help="(with --full)")
  ap.add_argument("--cpu-baseline-sample-only", action="store_true",
                  help="(with --full) CPU baseline on the n=2048 sample only (skip the one "
                       "n=8192 oracle call)")
  ap.add_argument("--no-concurrent", action="store_true", help="(with --full)")
  ap.add_argument("--no-extras", action="store_true",
                  help="(with --full) skip the batch512 / autotune16 legs")
  args = ap.parse_args()
  if args.steps < 1 or args.warmup < 0:
    ap.error("--steps must be >= 1 and --warmup >= 0")

  from spectralcluster_amd import multigpu
  if "WORLD_SIZE" not in os.environ and (args.gpus or 1) > 1:
    # `python bench.py --gpus N` with no launcher around it: this process becomes the launcher
    # (one rank per GPU, same arguments), rank 0 prints the JSON line on our stdout
    sys.exit(multigpu.launch_local_ranks(
        [sys.executable, os.path.abspath(__file__)] + sys.argv[1:], args.gpus))
  world = int(os.environ.get("WORLD_SIZE", "1"))
  rank = int(os.environ.get("RANK", "0"))
  local_rank = int(os.environ.get("LOCAL_RANK", "0"))
  if args.gpus is not None and args.gpus != world:
    sys.exit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks" % (args.gpus, world))
  if os.environ.get("SC_BENCH_LAUNCH_ECHO"):
    # launch check without a GPU (tests/test_distributed_cpu.py): the ranks meet over the TCP
    # rendezvous the real run starts with, and rank 0 prints what a run would report about it
    sock = multigpu.SocketComm.from_env(rank, world) if world > 1 else multigpu.LocalComm()
    seen = [int(b.decode()) for b in sock.allgather_bytes(str(rank).encode())]
    sock.barrier()
    if rank == 0:
      print(json.dumps({"n_gpus": world, "ranks_seen": seen, "launch": "echo"}), flush=True)
    sock.close()
    return

  import spectralcluster_amd as sca
  from spectralcluster_amd import _lib

  # (one rank per GPU; on a box with fewer GPUs than ranks -- a 1-GPU test box -- ranks share)
  handle = _lib.default_handle(local_rank % max(1, _lib.device_count()))
  lib = handle.lib
  # (librccl prints a version banner on stdout when its first communicator comes up: stdout is
  #  this program's ONE JSON line, so fd 1 points at stderr while the ranks meet)
  sys.stdout.flush()
  saved_stdout = os.dup(1)
  os.dup2(2, 1)
  try:
    comm = multigpu.RcclComm.from_env(handle)  # RCCL (C ABI) for N > 1, identity for N = 1
  finally:
    sys.stdout.flush()
    os.dup2(saved_stdout, 1)
    os.close(saved_stdout)
  clusterer = sca.SpectralClusterer(
      min_clusters=2, max_clusters=MAX_CLUSTERS,
      refinement_options=sca.configs.icassp2018_refinement_options,
      laplacian_type=sca.LaplacianType.GraphCut, device=local_rank)
  cfg = clusterer.build_config()

  # per-rank utterance (different seed per rank: independent replicas)
  x, truth = blobs(N_SAMPLES, N_FEATURES, N_SPEAKERS, SEED + rank)
  labels = np.empty(N_SAMPLES, dtype=np.int64)
  diag = _lib.ScDiag()

  def step():
    handle.check(lib.sc_run_resident(handle.raw, cfg, _lib.as_int64_p(labels), diag))

  def step_h2d():
    handle.check(lib.sc_predict(handle.raw, _lib.as_double_p(x), N_SAMPLES, N_FEATURES, cfg,
                                _lib.as_int64_p(labels), diag))

  def fence():
    handle.check(lib.sc_synchronize(handle.raw))  # this rank's stream has drained ...
    comm.barrier()                                # ... and every rank has arrived

  def timed(fn, k, collect=None):
    fence()
    t0 = time.perf_counter()
    for _ in range(k):
      fn()
      if collect is not None:
        collect()
    fence()
    return comm.allreduce_max(time.perf_counter() - t0)

  for _ in range(args.warmup):
    step_h2d()
  names = _lib.STAGE_NAMES
  stage_sum = np.zeros(len(names))
  passes = [0]

  def collect():
    stage_sum[:] += [diag.stage_ms[i] for i in range(len(names))]
    passes[0] += diag.eig_matvec_passes

  k = args.steps
  # THE timed region: K predict() calls (the per-stage timers are summed for --full only)
  elapsed = timed(step_h2d, k, collect if args.full else None)
  if args.dump_outputs and rank == 0:
    dump_outputs(args.dump_outputs, labels=labels, eigenvalues=diag.eigenvalue_array())

  if not args.full:
    extras = {}
    if args.workload == "batch512":
      extras["batch512"] = batch512_leg(sca, multigpu, comm, fence, project=False)
    elif args.workload == "autotune16":
      extras["autotune16"] = autotune16_leg(sca, multigpu, comm, fence, project=False)
    if rank == 0:
      out = headline_record(args, world, elapsed, comm, multigpu)
      select_workload(out, extras, args.workload)
      print(json.dumps(out), flush=True)
    comm.barrier()
    comm.close()
    return

  handle.check(lib.sc_set_embeddings(handle.raw, _lib.as_double_p(x), N_SAMPLES,
                                     N_FEATURES))
  stage_ms = {name: float(stage_sum[i] / k) for i, name in enumerate(names)}
  passes_per_call = passes[0] / k
  eig_info = {"matvec_passes_per_call": passes_per_call, "block": int(diag.eig_block),
              "basis": int(diag.eig_basis), "cycles": int(diag.eig_cycles),
              "path": int(diag.eig_path)}
  predict_labels = labels.copy()
  n_clusters = int(diag.n_clusters)
  eigenvalues = diag.eigenvalue_array()

  step()
  res_sum = np.zeros(len(names))

  def collect_res():
    res_sum[:] += [diag.stage_ms[i] for i in range(len(names))]

  elapsed_resident = timed(step, k, collect_res)
  resident_stage_ms = {name: float(res_sum[i] / k) for i, name in enumerate(names)}
  resident_labels = labels.copy()

  # per-kernel timers (a few extra steps with event pairs around the hot kernels)
  handle.check(lib.sc_set_profiling(handle.raw, 2))
  fine_sum = np.zeros(len(names))
  fine_k = max(3, min(k, 10))
  for _ in range(fine_k):
    step()
    fine_sum += [diag.stage_ms[i] for i in range(len(names))]
  handle.check(lib.sc_set_profiling(handle.raw, 1))
  fine_ms = {name: float(fine_sum[i] / fine_k) for i, name in enumerate(names)}

  # the same call with the explicit fp64 Diffuse product (sc_config.diffuse_mode = 1): the
  # route rounds 1-3 measured, kept as the row the matrix-free route is compared with
  cfg_explicit = clusterer.build_config()
  cfg_explicit.diffuse_mode = 1
  labels_explicit = np.empty(N_SAMPLES, dtype=np.int64)
  diag_x = _lib.ScDiag()

  def step_explicit():
    handle.check(lib.sc_run_resident(handle.raw, cfg_explicit, _lib.as_int64_p(labels_explicit),
                                     diag_x))

  step_explicit()
  kx = max(3, min(k, 10))
  xsum = np.zeros(len(names))

  def collect_x():
    xsum[:] += [diag_x.stage_ms[i] for i in range(len(names))]

  elapsed_explicit = timed(step_explicit, kx, collect_x)
  explicit_ms = {name: float(xsum[i] / kx) for i, name in enumerate(names)}

  extras = {}
  if not args.no_extras or args.workload != "predict8192":
    if not args.no_extras or args.workload == "batch512":
      extras["batch512"] = batch512_leg(sca, multigpu, comm, fence)
    if not args.no_extras or args.workload == "autotune16":
      extras["autotune16"] = autotune16_leg(sca, multigpu, comm, fence)
    if not args.no_extras:
      extras["autotune16_ttd"] = autotune16_leg(sca, multigpu, comm, fence, variant="ttd",
                                                project=False)
      if world == 1:
        extras["hard8192"] = hard8192_leg(sca, _lib)

  if rank == 0:
    nt = (N_SAMPLES + GEMM_TILE - 1) // GEMM_TILE
    flops = nt * (nt + 1) // 2 * 2.0 * GEMM_TILE * GEMM_TILE * N_SAMPLES
    free = stage_ms.get("free_product", 0.0) > 0  # the matrix-free Diffuse ran (default here)
    # explicit route: the fp64 Diffuse GEMM is the dominant kernel
    xdiffuse_s = explicit_ms["diffuse"] * 1e-3
    xachieved = flops / xdiffuse_s / 1e12 if xdiffuse_s > 0 else 0.0
    if free:
      # Round 6: the digit product walks a skip list (sc_diag.free_tiles_run of the upper
      # triangle's tiles; the others are proven free of row maxima and candidates).  Its
      # algorithmic work is that of the tiles that HAVE to be computed: 4 digit products x
      # tiles_run x 2 * 128^2 * K, K rounded up to the 64-wide stage.
      tiles_total = nt * (nt + 1) // 2
      tiles_run = int(diag.free_tiles_run) or tiles_total
      per_tile = 4.0 * 2.0 * GEMM_TILE * GEMM_TILE * ((N_SAMPLES + 63) // 64 * 64)
      ops = per_tile * tiles_run
      prod_s = stage_ms["free_product"] * 1e-3
      achieved = ops / prod_s / 1e12
      i8 = {"bound": "mfma", "kernel": "k_free_tile_flags + k_gemm_i8_sym + k_i8_tail_finish "
                                       "(exact int8-digit product of the matrix-free Diffuse "
                                       "over its skip list)",
            "achieved": achieved, "peak": PEAK_I8_MFMA_TOPS, "unit": "TFLOP/s",
            "frac": achieved / PEAK_I8_MFMA_TOPS, "traffic": None,
            "tiles_run": tiles_run, "tiles_total": tiles_total,
            "ops_note": "int8 multiply-add = 2 ops; peak = dense int8 MFMA (2x the 2.5 PF bf16 "
                        "rate, MI355X_MICROARCH.md); 4 digit products hh, hl, lh, ll of the "
                        "tiles that ran",
            "flops_per_launch": ops, "avg_launch_ms": stage_ms["free_product"],
            "all_tiles_equivalent_tops": per_tile * tiles_total / prod_s / 1e12}
      # ... which leaves the affinity GEMM (fp64 MFMA, K = d) as the longest kernel of the call
      aff_s = stage_ms.get("affinity_gemm", 0.0) * 1e-3
      aff_flops = tiles_total * 2.0 * GEMM_TILE * GEMM_TILE * N_FEATURES
      aff = {"bound": "mfma", "kernel": "k_gemm_nt<EpiAffinity,SYM> (cosine affinity, fp64 "
                                        "MFMA, upper-triangle tiles, crop value in the epilogue)",
             "achieved": aff_flops / aff_s / 1e12 if aff_s > 0 else 0.0,
             "peak": PEAK_F64_MFMA_TFLOPS, "unit": "TFLOP/s", "traffic": None,
             "flops_per_launch": aff_flops, "avg_launch_ms": stage_ms.get("affinity_gemm", 0.0),
             "note": "K = %d is %d K-tiles: prologue / epilogue bound; its write floor is "
                     "n^2 * 8 B / 8 TB/s = %.0f us" % (N_FEATURES, N_FEATURES // 16,
                                                      N_SAMPLES * N_SAMPLES * 8.0 / 8e12 * 1e6)}
      aff["frac"] = aff["achieved"] / PEAK_F64_MFMA_TFLOPS
      if aff_s > prod_s:
        roof = aff
        roof["dominant_by"] = ("longest kernel of the call in the timed region (hipEvents): "
                               "%.0f us against %.0f us of the digit product" %
                               (1e6 * aff_s, 1e6 * prod_s))
        roof["i8_product"] = i8
      else:
        roof = i8
        roof["affinity_gemm"] = aff
    else:
      diffuse_s = stage_ms["diffuse"] * 1e-3
      achieved = flops / diffuse_s / 1e12 if diffuse_s > 0 else 0.0
      roof = {"bound": "mfma", "kernel": "k_gemm_nt<EpiNone,SYM> (Diffuse)",
              "achieved": achieved, "peak": PEAK_F64_MFMA_TFLOPS, "unit": "TFLOP/s",
              "frac": achieved / PEAK_F64_MFMA_TFLOPS, "traffic": None,
              "flops_per_launch": flops, "avg_launch_ms": stage_ms["diffuse"]}
    fine_ms["_tiles_run"] = int(diag.free_tiles_run) if free else 0
    roof["kernels"] = kernel_roofline(fine_ms, passes_per_call)
    roof["fp64_diffuse_route"] = {
        "kernel": "k_gemm_nt<EpiNone,SYM> (Diffuse), sc_config.diffuse_mode = 1",
        "bound": "mfma", "achieved": xachieved, "peak": PEAK_F64_MFMA_TFLOPS,
        "unit": "TFLOP/s", "frac": xachieved / PEAK_F64_MFMA_TFLOPS, "flops_per_launch": flops,
        "avg_launch_ms": explicit_ms["diffuse"], "traffic": None,
        "resident_ms_per_step": 1e3 * elapsed_explicit / kx,
        "stage_ms": {kk: explicit_ms[kk] for kk in ("affinity", "refine", "diffuse", "scaling",
                                                    "eig", "kmeans", "total")},
        "labels_equal_with_default_route": bool(np.array_equal(labels_explicit, predict_labels))}
    # whole call against its floors (SURVEY 8d arithmetic, symmetry exploited, 8 TB/s):
    #   explicit route: (n^3 + n^2 d) fp64 flops on MFMA + (7 + passes) n^2 * 8 B
    #   matrix-free:    n^2 d fp64 flops + the digit product on the int8 cores + A1 write,
    #                   Crop+Blur R/W, Thr+Sym R/W + n^2 * 2 B of digits from the same pass, T
    #                   written and read once (fp32 upper triangle), one read of A for the exact
    #                   statistics, and 2 x passes half-matrix products
    nn = float(N_SAMPLES) * N_SAMPLES
    mat = nn * 8.0
    x_floor = ((nn * (N_SAMPLES + N_FEATURES)) / (PEAK_F64_MFMA_TFLOPS * 1e12) +
               ((7.0 + passes_per_call) * mat + N_SAMPLES * N_FEATURES * 8.0) / (PEAK_HBM_TBS * 1e12))
    # (round 6: the int8 term counts the tiles the skip list left -- the work that has to be done)
    i8_share = (float(diag.free_tiles_run) / (nt * (nt + 1) // 2)
                if free and diag.free_tiles_run > 0 else 1.0)
    f_floor = (nn * N_FEATURES / (PEAK_F64_MFMA_TFLOPS * 1e12) +
               i8_share * 4.0 * nn * N_SAMPLES / (PEAK_I8_MFMA_TOPS * 1e12) +
               (5.0 * mat + nn * 2.0 + 2 * nn * 2.0 + mat + 2.0 * passes_per_call * 0.5 * mat +
                N_SAMPLES * N_FEATURES * 8.0) / (PEAK_HBM_TBS * 1e12))
    whole = {"measured_ms": 1e3 * elapsed / k,
             "floor_ms": 1e3 * (f_floor if free else x_floor),
             "frac": (f_floor if free else x_floor) / (elapsed / k),
             "route": "matrix-free Diffuse" if free else "explicit fp64 Diffuse",
             "explicit_route_floor_ms": 1e3 * x_floor,
             "matrix_free_route_floor_ms": 1e3 * f_floor,
             "int8_share_of_tiles": i8_share,
             "measured_over_explicit_route_floor": (elapsed / k) / x_floor,
             "note": "floors: MFMA time of the flops/ops at peak + algorithmic HBM bytes at "
                     "8 TB/s, stages data-dependent so they add; H2D of X inside measured_ms"}
    out = headline_record(args, world, elapsed, comm, multigpu)
    out.update({
        "resident": {
            "value": world * k / elapsed_resident, "unit": "calls/s",
            "ms_per_step": 1e3 * elapsed_resident / k,
            "step": "sc_run_resident: the same pipeline with the embeddings already in HBM "
                    "(no H2D of X; labels D2H inside)",
            "stage_ms": {kk: v for kk, v in resident_stage_ms.items()
                         if kk in ("affinity", "refine", "diffuse", "scaling", "eig", "kmeans",
                                   "total")}},
        "roofline": roof,
        "whole_call": whole,
        "stage_ms": {kk: v for kk, v in stage_ms.items()
                     if kk in ("affinity", "refine", "diffuse", "scaling", "eig", "kmeans",
                               "total", "free_quantize", "free_product", "free_scan",
                               "free_stats") and (v > 0 or not kk.startswith("free_"))},
        "diffuse_path": int(diag.diffuse_path),
        "eig": eig_info,
        "parity": {"n_clusters": n_clusters, "ari_vs_truth": ari(predict_labels, truth),
                   "labels_equal_with_resident_path": bool(np.array_equal(resident_labels,
                                                                         predict_labels))},
    })
    gpath = os.path.join(ROOT, "tests", "golden", "e2e_n8192_lap4_max20.npz")
    if os.path.exists(gpath):
      g = np.load(gpath)
      w = eigenvalues[g["consumed_index"]]
      rel = np.abs(w - g["consumed_eigenvalues"]) / np.maximum(
          np.abs(g["consumed_eigenvalues"]), 1e-12)
      out["parity"]["ari_vs_reference_labels"] = ari(predict_labels, g["labels"])
      out["parity"]["max_rel_err_consumed_eigenvalues"] = float(np.max(rel))
      # the bulk values (~0.99999) pass 1e-5 for any Ritz value in range: the meaningful
      # figure is the error on the informative (non-bulk) eigenvalues
      informative = g["consumed_eigenvalues"] < 0.5
      if informative.any():
        out["parity"]["max_rel_err_informative_eigenvalues"] = float(np.max(rel[informative]))
      out["parity"]["reference_seconds_per_call_8vcpu"] = float(g["ref_seconds"])
    tpath = os.path.join(ROOT, "profiles", "pmc_traffic_diffuse.json")
    if os.path.exists(tpath):  # HBM bytes per Diffuse launch from a separate --pmc run
      t = json.load(open(tpath))
      target = out["roofline"]["fp64_diffuse_route"]  # (that file describes the fp64 GEMM)
      target["traffic"] = t["hbm_bytes_per_launch"]
      target["traffic_source"] = t["source"]
      # stamped with the kernel source it was measured on: stale once gemm_f64.hip changes
      import hashlib
      src = os.path.join(ROOT, "spectralcluster_amd", "csrc", "gemm_f64.hip")
      now = hashlib.sha256(open(src, "rb").read()).hexdigest()[:16]
      target["traffic_measured_on"] = {
          "commit": t.get("commit"), "gemm_f64_sha16": t.get("gemm_f64_sha16"),
          "kernel_source_unchanged_since": t.get("gemm_f64_sha16") == now}
    ipath = os.path.join(ROOT, "profiles", "pmc_traffic_i8.json")
    if free and os.path.exists(ipath):  # HBM bytes per digit-product launch (separate --pmc run)
      t = json.load(open(ipath))
      import hashlib
      src = os.path.join(ROOT, "spectralcluster_amd", "csrc", "diffuse_free.hip")
      now = hashlib.sha256(open(src, "rb").read()).hexdigest()[:16]
      tgt = out["roofline"].get("i8_product", out["roofline"])
      tgt["traffic"] = t["hbm_bytes_per_launch"]
      tgt["traffic_source"] = t["source"]
      tgt["algorithmic_bytes_per_launch"] = t["algorithmic_bytes_per_launch"]
      tgt["traffic_measured_on"] = {
          "commit": t.get("commit"), "diffuse_free_sha16": t.get("diffuse_free_sha16"),
          "kernel_source_unchanged_since": t.get("diffuse_free_sha16") == now}
    apath = os.path.join(ROOT, "profiles", "pmc_traffic_affinity.json")
    if free and "i8_product" in out["roofline"] and os.path.exists(apath):
      t = json.load(open(apath))  # HBM bytes per affinity-GEMM launch (separate --pmc run)
      import hashlib
      src = os.path.join(ROOT, "spectralcluster_amd", "csrc", "gemm_f64.hip")
      now = hashlib.sha256(open(src, "rb").read()).hexdigest()[:16]
      out["roofline"]["traffic"] = t["hbm_bytes_per_launch"]
      out["roofline"]["traffic_source"] = t["source"]
      out["roofline"]["algorithmic_bytes_per_launch"] = t["algorithmic_bytes_per_launch"]
      out["roofline"]["traffic_measured_on"] = {
          "commit": t.get("commit"), "gemm_f64_sha16": t.get("gemm_f64_sha16"),
          "kernel_source_unchanged_since": t.get("gemm_f64_sha16") == now}
    select_workload(out, extras, args.workload)
    if world == 1 and not args.no_concurrent:
      out["concurrent_streams"] = concurrent_leg(_lib, cfg, x, args.steps)
      out["pipelined_uploads"] = pipelined_leg(_lib, handle, cfg, x, args.steps)
    if world == 1 and not args.no_cpu_baseline:
      out["cpu_baseline"], out["cpu_baseline_algorithm_matched"] = cpu_baseline_legs(
          clusterer, full_size=not args.cpu_baseline_sample_only)
    print(json.dumps(out), flush=True)
  comm.barrier()
  comm.close()


if __name__ == "__main__":
  main()
