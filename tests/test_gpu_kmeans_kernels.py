"""GPU: the k-means kernels (csrc/kmeans_chain.hip: the chain km_colsum ... km_cosine in its three
register widths and its grouped form; csrc/kmeans.hip: the single-workgroup kernel and its large-k
form) against the traced reference of tests/_kmeans_ref.py, through sc_stage_kmeans_trace /
sc_stage_kmeans_trace_group: seeds, Lloyd-step centroids, first assignment, the mean distance of
every pass, the number of passes, final centroids and labels -- not the final labels alone.

a. exact-arithmetic inputs (small integers, column sums 0): everything through the Lloyd step
   bit for bit, no tolerance.
b. overlapping inputs (noise 1.0 and 3.0: 2-14 passes): seeds and pass counts exactly (the inputs
   keep every such decision of the reference 1e-9 away from its other outcome; the host test
   asserts it), continuous results within a tolerance made of host numbers alone -- 8 x the
   deviation of the plain float64 NumPy oracle from the longdouble trace, at least 4 ulp of the
   quantity's largest magnitude.  Yardsticks (that deviation) over the committed cases:
     column means        0 .. 1.1e-15   (largest at n = 2049, k = 17)
     Lloyd centroids     0 .. 3.0e-15   (n = 7680, k = 32)
     mean distances      0 .. 1.5e-16   (n = 700, k = 64)
     final centroids     0 .. 3.1e-15   (n = 7680 / 7681, k = 32)
   Labels: every row, except rows whose reference margin is below the distance tolerance (none
   in the committed cases; the host test caps them at 1 %).
c. rules of the custom loop: a cluster whose only member is row 0 keeps its centroid, an empty
   cluster, max_iter cutting the run, max_iter beyond the chain's ring of mean distances.
d. the grouped chain against the chain alone, bit for bit, members finishing in different
   enqueues, both member orders.
e. the values a handle caches between calls.
"""

import ctypes

import numpy as np
import pytest

import _kmeans_ref as kr
from spectralcluster_amd import _lib

pytestmark = pytest.mark.gpu

AUTO, CHAIN, SINGLE = 0, 1, 2
I32 = ctypes.POINTER(ctypes.c_int)


def _i32(a):
  return a.ctypes.data_as(I32)


def device_trace(handle, e, k, max_iter=300, form=CHAIN):
  """sc_stage_kmeans_trace as a dict; chain-only outputs stay NaN / -1 for the other forms."""
  e = np.ascontiguousarray(e, dtype=np.float64)
  n = e.shape[0]
  cap = max_iter + 2
  out = {"col_means": np.full(k, np.nan), "seeds": np.full(k, -1, dtype=np.int32),
         "last_candidates": np.full(8, -1, dtype=np.int32), "last_potentials": np.full(8, np.nan),
         "lloyd_centroids": np.full((k, k), np.nan),
         "first_labels": np.full(n, -1, dtype=np.int64), "mean_dist": np.full(cap, np.nan),
         "centroids": np.full((k, k), np.nan), "labels": np.full(n, -1, dtype=np.int64)}
  form_run, iters = ctypes.c_int(0), ctypes.c_int(0)
  handle.check(handle.lib.sc_stage_kmeans_trace(
      handle.raw, _lib.as_double_p(e), n, k, max_iter, form, ctypes.byref(form_run),
      _lib.as_double_p(out["col_means"]), _i32(out["seeds"]), _i32(out["last_candidates"]),
      _lib.as_double_p(out["last_potentials"]), _lib.as_double_p(out["lloyd_centroids"]),
      _lib.as_int64_p(out["first_labels"]), _lib.as_double_p(out["mean_dist"]), cap,
      ctypes.byref(iters), _lib.as_double_p(out["centroids"]), _lib.as_int64_p(out["labels"])))
  out["form"], out["iterations"] = form_run.value, iters.value
  out["mean_dist"] = out["mean_dist"][:iters.value]
  return out


def device_trace_group(handle, inputs, max_iter=300):
  """sc_stage_kmeans_trace_group; inputs: (n, k) arrays, None = an idle position."""
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
  handle.check(handle.lib.sc_stage_kmeans_trace_group(
      handle.raw, _lib.as_double_p(es), _i32(ns), _i32(ks), count, max_iter,
      _lib.as_double_p(col_means), _i32(seeds), _i32(cands), _lib.as_double_p(pots),
      _lib.as_double_p(lloyd), _lib.as_int64_p(first), _lib.as_double_p(hist), cap, _i32(iters),
      _lib.as_double_p(cent), _lib.as_int64_p(labels)))
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


TRACE_KEYS = ("col_means", "seeds", "last_candidates", "last_potentials", "lloyd_centroids",
              "first_labels", "mean_dist", "centroids", "labels")


def assert_same_bits(got, want, keys=TRACE_KEYS):
  assert got["iterations"] == want["iterations"]
  for key in keys:
    a, b = np.asarray(got[key]), np.asarray(want[key])
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), key


def check_against_reference(got, case, max_iter=300, chain=True):
  """Discrete results exactly, continuous ones within the host-made tolerance."""
  ref, _, tol = kr.overlap_reference(case, max_iter)
  k = case[1]
  assert np.array_equal(got["seeds"], ref["seeds"])
  assert got["iterations"] == ref["iterations"]
  unsure = kr.uncertain_rows(ref, tol["mean_dist"][0])
  names = kr.CONTINUOUS if chain else ("centroids",)
  for name in names:
    want = np.asarray(ref[name])
    err = float(np.max(np.abs(np.asarray(got[name], dtype=kr.LD) - want)))
    print("%s %s: error %.3g, tolerance %.3g (yardstick %.3g)" % (case, name, err,
                                                                  tol[name][0], tol[name][1]))
  for name in names:
    want = np.asarray(ref[name])
    err = float(np.max(np.abs(np.asarray(got[name], dtype=kr.LD) - want)))
    assert err <= tol[name][0], (name, err, tol[name])
  if chain:
    keep = ~unsure[0]
    assert np.mean(keep) >= 1 - kr.LABEL_CAP
    assert np.array_equal(got["first_labels"][keep], ref["first_labels"][keep])
    if k > 1:
      last = ref["rounds"][-1]
      assert np.array_equal(got["last_candidates"][:ref["trials"]], last["candidates"])
      assert int(np.argmin(got["last_potentials"][:ref["trials"]])) == last["winner"]
  keep = ~unsure[-1]
  assert np.mean(keep) >= 1 - kr.LABEL_CAP
  assert np.array_equal(got["labels"][keep], ref["labels"][keep])


# ------------------------------------------------------------------------------ a. exact
@pytest.mark.parametrize("form", [CHAIN, SINGLE], ids=["chain", "single"])
@pytest.mark.parametrize("name", sorted(kr.EXACT_CASES))
def test_exact_inputs_bit_for_bit(handle, name, form):
  e = kr.exact_input(name)
  k = e.shape[1]
  ref = kr.trace(e, k, 300, np.float64)
  got = device_trace(handle, e, k, 300, form)
  assert got["form"] == form
  assert np.array_equal(got["seeds"], ref["seeds"])
  if form == CHAIN:
    trials, last = ref["trials"], ref["rounds"][-1]
    assert np.all(got["col_means"] == 0.0)
    assert np.array_equal(got["last_candidates"][:trials], last["candidates"])
    assert np.array_equal(got["last_potentials"][:trials], last["trial_potentials"])
    assert int(np.argmin(got["last_potentials"][:trials])) == last["winner"]
    assert got["lloyd_centroids"].tobytes() == ref["lloyd_centroids"].tobytes()
  # (the chain keeps the candidate rows of its last k-means++ round only; of the earlier rounds
  #  the seeds, each round's winning candidate, are compared)


# ------------------------------------------------------------------------------ b. overlapping
@pytest.mark.parametrize("case", kr.OVERLAP_CASES + kr.BOUNDARY_CASES[:1], ids=str)
def test_chain_against_the_traced_reference(handle, case):
  got = device_trace(handle, kr.overlap_input(case), case[1], 300, CHAIN)
  assert got["form"] == 1
  check_against_reference(got, case)


@pytest.mark.parametrize("case", kr.SINGLE_CASES + kr.BIG_CASES, ids=str)
def test_single_workgroup_forms_against_the_traced_reference(handle, case):
  got = device_trace(handle, kr.overlap_input(case), case[1], 300, SINGLE)
  assert got["form"] == (3 if case[1] > 64 else 2)
  check_against_reference(got, case, chain=False)
  if case[1] > 32:  # the chain does not take more than 32 clusters, and says so
    with pytest.raises(_lib.UnsupportedOnDeviceError):
      device_trace(handle, kr.overlap_input(case), case[1], 300, CHAIN)


def test_route_boundary_at_k32(handle):
  """n = 7680 is the last the chain takes at k = 32 (its partial sums: 60 workgroups x 1088);
  7681 rows run the single-workgroup kernel."""
  inside, beyond = kr.BOUNDARY_CASES
  got = device_trace(handle, kr.overlap_input(inside), 32, 300, AUTO)
  assert got["form"] == 1
  with pytest.raises(_lib.UnsupportedOnDeviceError):
    device_trace(handle, kr.overlap_input(beyond), 32, 300, CHAIN)
  got = device_trace(handle, kr.overlap_input(beyond), 32, 300, AUTO)
  assert got["form"] == 2
  check_against_reference(got, beyond, chain=False)


# ------------------------------------------------------------------------------ c. loop rules
@pytest.mark.parametrize("form", [CHAIN, SINGLE], ids=["chain", "single"])
@pytest.mark.parametrize("case", [kr.ROW0_ALONE_CASE, kr.EMPTY_CLUSTER_CASE], ids=str)
def test_row0_alone_and_empty_cluster(handle, case, form):
  got = device_trace(handle, kr.overlap_input(case), case[1], 300, form)
  check_against_reference(got, case, chain=form == CHAIN)


@pytest.mark.parametrize("form", [CHAIN, SINGLE], ids=["chain", "single"])
@pytest.mark.parametrize("max_iter", [1, 2, 3, 4, 5, 8])
def test_max_iter_cuts_the_run(handle, max_iter, form):
  case = kr.MAX_ITER_CASE
  got = device_trace(handle, kr.overlap_input(case), case[1], max_iter, form)
  assert got["iterations"] == max_iter + 1
  check_against_reference(got, case, max_iter, chain=form == CHAIN)


@pytest.mark.parametrize("form", [CHAIN, SINGLE], ids=["chain", "single"])
def test_max_iter_beyond_the_mean_distance_ring(handle, form):
  """max_iter = 600 (the chain keeps 512 mean distances) on a converging input: as max_iter = 300."""
  case = (300, 9, 3.0, 1)
  e = kr.overlap_input(case)
  want = device_trace(handle, e, 9, 300, form)
  got = device_trace(handle, e, 9, 600, form)
  keys = TRACE_KEYS if form == CHAIN else ("seeds", "centroids", "labels")
  assert_same_bits(got, want, keys)
  check_against_reference(got, case, chain=form == CHAIN)


# ------------------------------------------------------------------------------ d. grouped
@pytest.mark.parametrize("reverse", [False, True], ids=["in_order", "reversed"])
def test_grouped_chain_is_the_chain(handle, reverse):
  """Every member of a grouped launch -- other members' k widening its register tile, idle
  positions, members finishing in different enqueues -- has exactly the trace of the chain run on
  it alone."""
  inputs = [kr.overlap_input(c) for c in kr.GROUP_MEMBERS]
  twin = kr.overlap_input((129, 3, 3.0, 1))
  inputs = inputs[:3] + [None] + inputs[3:] + [twin, twin]
  if reverse:
    inputs = inputs[::-1]
  alone = [None if e is None else device_trace(handle, e, e.shape[1], 300, CHAIN)
           for e in inputs]
  assert len({(t["iterations"] + 3) // 4 for t in alone if t is not None}) >= 3
  grouped = device_trace_group(handle, inputs, 300)
  for z, (g, a) in enumerate(zip(grouped, alone)):
    if a is None:
      assert g is None
      continue
    assert_same_bits(g, a)


# ------------------------------------------------------------------------------ e. handle state
def test_cached_seed_constants_follow_n_and_k():
  """The first centre depends on n, the random numbers and the trial count on k; a handle keeps
  both between calls.  (n1, k1), (n2, k1), (n1, k2), (n1, k1) on one handle: as on fresh ones."""
  def stage(h, e):
    n, k = e.shape
    labels, cent = np.empty(n, dtype=np.int64), np.empty((k, k))
    iters = ctypes.c_int(0)
    h.check(h.lib.sc_stage_kmeans(h.raw, _lib.as_double_p(np.ascontiguousarray(e)), n, k, 300,
                                  _lib.as_int64_p(labels), _lib.as_double_p(cent),
                                  ctypes.byref(iters)))
    return labels, cent, iters.value
  sequence = [(300, 9, 3.0, 1), (129, 9, 1.0, 1), (300, 17, 3.0, 1), (300, 9, 3.0, 1)]
  kept = _lib.Handle(0)
  try:
    for case in sequence:
      e = kr.overlap_input(case)
      fresh = _lib.Handle(0)
      try:
        want = stage(fresh, e)
      finally:
        fresh.close()
      got = stage(kept, e)
      assert got[2] == want[2] == kr.overlap_reference(case)[0]["iterations"]
      assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
      assert np.array_equal(got[0], kr.overlap_reference(case)[0]["labels"])
  finally:
    kept.close()
