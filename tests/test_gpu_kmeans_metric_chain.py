"""GPU: the chain's iteration kernel under every custom_dist metric (csrc/kmeans_chain.hip:
km_iter<KC, M> and its grouped form km_iter_g) through sc_stage_kmeans_trace_metric /
sc_stage_kmeans_trace_group_metric, against the longdouble trace of tests/_kmeans_metric_ref.py
(whose float64 twin tests/test_kmeans_metric_trace_reference_host.py holds to scipy's cdist and
spectral_oracle.run_kmeans_metric).

Seeds, first labels, labels and pass counts are compared exactly (rows whose reference margin is
below the distance tolerance excluded, at most LABEL_CAP of them); the mean distance of every
pass, the Lloyd centroids and the final centroids within `_kmeans_ref.tolerances`: 8 x the
deviation of the float64 NumPy trace from the longdouble one, at least 4 ulp.  The
single-workgroup kernel answers to the same reference on one case; the grouped form is the chain
alone bit for bit; cosine through the new entries is the old entries bit for bit.
"""

import ctypes

import numpy as np
import pytest

import _kmeans_metric_ref as mr
import _kmeans_ref as kr
from spectralcluster_amd import _lib

pytestmark = pytest.mark.gpu

AUTO, CHAIN, SINGLE = 0, 1, 2
I32 = ctypes.POINTER(ctypes.c_int)
TRACE_KEYS = ("col_means", "seeds", "last_candidates", "last_potentials", "lloyd_centroids",
              "first_labels", "mean_dist", "centroids", "labels")


def _i32(a):
  return a.ctypes.data_as(I32)


def _code(metric):
  return _lib.KMEANS_METRICS[metric]


def device_trace(handle, e, k, metric, max_iter=300, form=CHAIN, old_entry=False):
  """sc_stage_kmeans_trace_metric as a dict (`old_entry`: sc_stage_kmeans_trace, cosine)."""
  e = np.ascontiguousarray(e, dtype=np.float64)
  n = e.shape[0]
  cap = max_iter + 2
  out = {"col_means": np.full(k, np.nan), "seeds": np.full(k, -1, dtype=np.int32),
         "last_candidates": np.full(8, -1, dtype=np.int32), "last_potentials": np.full(8, np.nan),
         "lloyd_centroids": np.full((k, k), np.nan),
         "first_labels": np.full(n, -1, dtype=np.int64), "mean_dist": np.full(cap, np.nan),
         "centroids": np.full((k, k), np.nan), "labels": np.full(n, -1, dtype=np.int64)}
  form_run, iters = ctypes.c_int(0), ctypes.c_int(0)
  tail = (ctypes.byref(form_run),
          _lib.as_double_p(out["col_means"]), _i32(out["seeds"]), _i32(out["last_candidates"]),
          _lib.as_double_p(out["last_potentials"]), _lib.as_double_p(out["lloyd_centroids"]),
          _lib.as_int64_p(out["first_labels"]), _lib.as_double_p(out["mean_dist"]), cap,
          ctypes.byref(iters), _lib.as_double_p(out["centroids"]), _lib.as_int64_p(out["labels"]))
  if old_entry:
    assert metric == "cosine"
    handle.check(handle.lib.sc_stage_kmeans_trace(
        handle.raw, _lib.as_double_p(e), n, k, max_iter, form, *tail))
  else:
    handle.check(handle.lib.sc_stage_kmeans_trace_metric(
        handle.raw, _lib.as_double_p(e), n, k, max_iter, form, _code(metric), *tail))
  out["form"], out["iterations"] = form_run.value, iters.value
  out["mean_dist"] = out["mean_dist"][:iters.value]
  return out


def device_trace_group(handle, inputs, metric, max_iter=300, old_entry=False):
  """sc_stage_kmeans_trace_group_metric; inputs: (n, k) arrays, None = an idle position."""
  count = len(inputs)
  ns = np.array([0 if e is None else e.shape[0] for e in inputs], dtype=np.int32)
  ks = np.array([0 if e is None else e.shape[1] for e in inputs], dtype=np.int32)
  es = np.concatenate([np.ascontiguousarray(e, dtype=np.float64).ravel()
                       for e in inputs if e is not None])
  rows, cap = int(ns.sum()), max_iter + 2
  col_means, seeds = np.full((count, 32), np.nan), np.full((count, 32), -1, dtype=np.int32)
  cands, pots = np.full((count, 8), -1, dtype=np.int32), np.full((count, 8), np.nan)
  lloyd, cent = np.full((count, 1024), np.nan), np.full((count, 1024), np.nan)
  first, labels = np.full(rows, -1, dtype=np.int64), np.full(rows, -1, dtype=np.int64)
  hist, iters = np.full((count, cap), np.nan), np.zeros(count, dtype=np.int32)
  tail = (_lib.as_double_p(col_means), _i32(seeds), _i32(cands), _lib.as_double_p(pots),
          _lib.as_double_p(lloyd), _lib.as_int64_p(first), _lib.as_double_p(hist), cap, _i32(iters),
          _lib.as_double_p(cent), _lib.as_int64_p(labels))
  if old_entry:
    assert metric == "cosine"
    handle.check(handle.lib.sc_stage_kmeans_trace_group(
        handle.raw, _lib.as_double_p(es), _i32(ns), _i32(ks), count, max_iter, *tail))
  else:
    handle.check(handle.lib.sc_stage_kmeans_trace_group_metric(
        handle.raw, _lib.as_double_p(es), _i32(ns), _i32(ks), count, max_iter, _code(metric),
        *tail))
  outs, at = [], 0
  for z in range(count):
    n, k = int(ns[z]), int(ks[z])
    if n == 0:
      outs.append(None)
      continue
    outs.append({"col_means": col_means[z, :k], "seeds": seeds[z, :k],
                 "last_candidates": cands[z], "last_potentials": pots[z],
                 "lloyd_centroids": lloyd[z, :k * k].reshape(k, k),
                 "first_labels": first[at:at + n], "mean_dist": hist[z, :iters[z]],
                 "centroids": cent[z, :k * k].reshape(k, k), "labels": labels[at:at + n],
                 "iterations": int(iters[z])})
    at += n
  return outs


def assert_same_bits(got, want, keys=TRACE_KEYS):
  assert got["iterations"] == want["iterations"]
  for key in keys:
    a, b = np.asarray(got[key]), np.asarray(want[key])
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), key


def check_against_reference(got, case, metric, max_iter=300, chain=True):
  """Discrete results exactly, continuous ones within the host-made tolerance; every figure is
  printed before anything is asserted."""
  ref, _, tol = mr.metric_reference(case, metric, max_iter)
  names = ("lloyd_centroids", "mean_dist", "centroids") if chain else ("centroids",)
  errs = {}
  for name in names:
    want = np.asarray(ref[name])
    have = np.asarray(got[name], dtype=kr.LD)
    errs[name] = float(np.max(np.abs(have - want))) if have.shape == want.shape else np.inf
    print("%s %s %s: error %.3g, tolerance %.3g (yardstick %.3g)" % (
        metric, case, name, errs[name], tol[name][0], tol[name][1]))
  print("%s %s: passes %d, reference %d" % (metric, case, got["iterations"], ref["iterations"]))
  assert np.array_equal(got["seeds"], ref["seeds"])
  assert got["iterations"] == ref["iterations"]
  for name in names:
    assert errs[name] <= tol[name][0], (name, errs[name], tol[name])
  unsure = kr.uncertain_rows(ref, tol["mean_dist"][0])
  if chain:
    keep = ~unsure[0]
    assert np.mean(keep) >= 1 - kr.LABEL_CAP
    assert np.array_equal(got["first_labels"][keep], ref["first_labels"][keep])
  keep = ~unsure[-1]
  assert np.mean(keep) >= 1 - kr.LABEL_CAP
  assert np.array_equal(got["labels"][keep], ref["labels"][keep])


PAIRS = [(m, c) for m in mr.METRICS for c in mr.cases_of(m)]


@pytest.mark.parametrize("metric,case", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_chain_against_the_traced_reference(handle, metric, case):
  got = device_trace(handle, kr.overlap_input(case), case[1], metric, 300, CHAIN)
  assert got["form"] == 1
  check_against_reference(got, case, metric)


@pytest.mark.parametrize("metric", mr.METRICS)
def test_single_workgroup_form_answers_to_the_same_reference(handle, metric):
  case = mr.SINGLE_CASE
  got = device_trace(handle, kr.overlap_input(case), case[1], metric, 300, SINGLE)
  assert got["form"] == 2
  check_against_reference(got, case, metric, chain=False)
  # auto is what the single call chooses for a metric other than cosine: this kernel
  auto = device_trace(handle, kr.overlap_input(case), case[1], metric, 300, AUTO)
  assert auto["form"] == 2
  assert_same_bits(auto, got, ("seeds", "centroids", "labels"))


@pytest.mark.parametrize("metric", mr.GROUP_METRICS)
def test_grouped_chain_is_the_chain(handle, metric):
  """One grouped launch: members of k = 2 .. 21 (the widest sizes everyone's register tile), an
  idle position, members leaving in different enqueues -- each has exactly the trace of the single
  chain form under the same metric."""
  members = [kr.overlap_input(c) for c in mr.group_members_of(metric)]
  inputs = members[:2] + [None] + members[2:]
  alone = [None if e is None else device_trace(handle, e, e.shape[1], metric, 300, CHAIN)
           for e in inputs]
  grouped = device_trace_group(handle, inputs, metric, 300)
  for g, a in zip(grouped, alone):
    if a is None:
      assert g is None
      continue
    assert_same_bits(g, a)


@pytest.mark.parametrize("max_iter", [1, 2, 5])
def test_max_iter_cuts_the_euclidean_run(handle, max_iter):
  case = mr.MAX_ITER_CASE
  got = device_trace(handle, kr.overlap_input(case), case[1], "euclidean", max_iter, CHAIN)
  assert got["iterations"] == max_iter + 1
  check_against_reference(got, case, "euclidean", max_iter)


@pytest.mark.parametrize("metric", mr.METRICS)
def test_one_cluster(handle, metric):
  """k = 1: nothing to assign; the pass count is the stop rule's alone, and the chain's is the
  single-workgroup kernel's."""
  case = mr.K1_CASE
  e = kr.overlap_input(case)
  chain = device_trace(handle, e, 1, metric, 300, CHAIN)
  single = device_trace(handle, e, 1, metric, 300, SINGLE)
  print("%s k = 1: passes chain %d, single %d" % (metric, chain["iterations"],
                                                 single["iterations"]))
  assert np.all(chain["labels"] == 0) and np.all(single["labels"] == 0)
  assert chain["iterations"] == single["iterations"]


def test_cosine_through_the_metric_entries_is_the_old_entries(handle):
  for case in [(129, 3, 1.0, 1), (300, 17, 3.0, 1), (300, 32, 3.0, 1)]:
    e = kr.overlap_input(case)
    for form, keys in ((CHAIN, TRACE_KEYS), (SINGLE, ("seeds", "centroids", "labels"))):
      old = device_trace(handle, e, case[1], "cosine", 300, form, old_entry=True)
      new = device_trace(handle, e, case[1], "cosine", 300, form)
      assert new["form"] == old["form"]
      assert_same_bits(new, old, keys)
  inputs = [kr.overlap_input(c) for c in mr.GROUP_MEMBERS]
  inputs = inputs[:2] + [None] + inputs[2:]
  old = device_trace_group(handle, inputs, "cosine", 300, old_entry=True)
  new = device_trace_group(handle, inputs, "cosine", 300)
  for g, a in zip(new, old):
    if a is None:
      assert g is None
      continue
    assert_same_bits(g, a)
