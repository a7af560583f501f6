"""GPU: the agglomerative linkage kernels (csrc/ahc.hip) directly, through sc_stage_linkage and
sc_stage_cosine_distances: the raw merge list of every form -- slot pairs, heights, sizes, chain
order -- against the NumPy port of scipy's loop in tests/_linkage_ref.py, not the labels after
the host cut alone.  The forms: 0 sc_ahc's distance + chain kernels, 1 the batch's, 2 the batch's
LDS kernel, 3 the stream pool's distance + chain kernels, 4 the pool's LDS kernel, 5 / 6 the
verdict forms of the batch's chain and LDS kernels.

a. merge lists bit for bit (`tobytes`), forms 0-4, both linkages where a form has them, on inputs
   whose distances are exact -- quantised to 1, 3 and 8 levels of 1/8 (14-610 tied scans per
   problem, the previous chain element wins 1-127 of them), the long chain (the chain grows to n
   elements), clipped cosines -- and on continuous cosines.  Sizes 2 .. 128 on every form, 129,
   257, 1023, 1024, 1025, 2049 (two full passes of the 1024 threads plus one row) on the chain
   forms.  tests/test_linkage_reference_host.py asserts what the inputs exercise.
b. the forms against each other: the same bytes.
c. the verdict forms: at a merge height, one step above and one step below it -- the lowest, the
   median and the highest distinct height, and a threshold above and below all -- the record is
   {first height in chain order >= threshold, 0} or {largest height, 1}, bit for bit.
d. a mixed batch in two member orders with a table offset, a member whose `bad` word is set and
   members of fewer than two rows: every member's result is its stand-alone one, the others keep
   the caller's fill value.
e. labels through the host cut against sklearn (metric="precomputed") on the quantised inputs.
f. equal embedding rows give bit-equal distance columns on the single-call and the batch route,
   D exactly symmetric -- also at the smallest shape at which the single call's symmetric product
   would split its leftover tiles over K (n = 3969, d = 256 on 256 CUs), which is where the two
   columns of a pair used to differ in the last bit until sc_ahc's product took whole-K tiles;
   the public clustering calls equal sklearn on such arrays: the partition always, the label
   numbering wherever the data settle it (numbering_is_settled).  The diagonal of D is zero.

Every matrix lies on the device with a pitch above n and padding of distance 0, and the entry
fails when a kernel writes behind a member's cluster sizes or its chain.
"""

import ctypes
import functools

import numpy as np
import pytest
from scipy.cluster.hierarchy import linkage as scipy_linkage
from scipy.spatial.distance import pdist
from sklearn.cluster import AgglomerativeClustering

import spectral_oracle as so

import _linkage_ref as lr
from spectralcluster_amd import _lib
from spectralcluster_amd import utils

pytestmark = pytest.mark.gpu

SINGLE, BATCH, BATCH_LDS, POOL, POOL_LDS, CHAIN_VERDICT, LDS_VERDICT = range(7)
SMALL = (2, 3, 4, 17, 63, 64, 65, 127, 128)
CHAIN_ONLY = (129, 257, 1023, 1024, 1025, 2049)
KINDS = ("q1", "q3", "q8", "chain", "clip", "cont")
METHODS = (lr.COMPLETE, lr.AVERAGE)
FILL = -7.0  # what the outputs hold before a call


def list_forms(n, method):
  forms = [SINGLE, BATCH, POOL]
  if n <= 128 and method == lr.AVERAGE:
    forms += [BATCH_LDS, POOL_LDS]
  return forms


def run_linkage(handle, form, method, cs, first=0, threshold=0.0, bad=None, cut=None):
  """sc_stage_linkage on the cosine matrices cs.  Returns the members' merge lists (forms 0-4) or
  records (5, 6), FILL where nothing was written; with cut = (n_clusters, distance_threshold)
  also their labels (-1 where none were written)."""
  ns = np.array([c.shape[0] for c in cs], dtype=np.int32)
  flat = np.concatenate([np.ascontiguousarray(c, dtype=np.float64).ravel() for c in cs])
  verdict = form in (CHAIN_VERDICT, LDS_VERDICT)
  zrows = np.maximum(ns - 1, 0)
  z = np.full((int(zrows.sum()), 4), FILL)
  records = np.full((len(cs), 2), FILL)
  labels = np.full(int(ns.sum()), -1, dtype=np.int64)
  bad_words = None if bad is None else np.asarray(bad, dtype=np.int32)
  handle.check(handle.lib.sc_stage_linkage(
      handle.raw, form, method, len(cs), _lib.as_int32_p(ns), _lib.as_double_p(flat), first,
      float(threshold), None if bad_words is None else _lib.as_int32_p(bad_words),
      None if verdict else _lib.as_double_p(z), _lib.as_double_p(records) if verdict else None,
      None if cut is None else _lib.as_int64_p(labels), 0 if cut is None else int(cut[0]),
      0.0 if cut is None else float(cut[1])))
  if verdict:
    return list(records)
  zs = np.split(z, np.cumsum(zrows)[:-1])
  if cut is None:
    return zs
  return zs, np.split(labels, np.cumsum(ns)[:-1])


def same_bits(a, b):
  a, b = np.asarray(a), np.asarray(b)
  return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- a, b: merge lists ---------------------------------------------------------------------

@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", SMALL + CHAIN_ONLY)
def test_merge_lists_bit_for_bit(handle, n, method):
  cs = [lr.cosines(kind, n) for kind in KINDS]
  want = [lr.reference(kind, n, method)[0] for kind in KINDS]
  by_form = {}
  for form in list_forms(n, method):
    got = run_linkage(handle, form, method, cs)
    by_form[form] = got
    for kind, g, w in zip(KINDS, got, want):
      assert same_bits(g, w), (form, kind, np.flatnonzero((g != w).any(axis=1))[:4])
  for form, got in by_form.items():  # (b) -- what (a) implies, said directly
    for g, w in zip(got, by_form[BATCH]):
      assert same_bits(g, w), form


def test_members_one_at_a_time_equal_the_batch(handle):
  """Form 0 member by member and a batch of one: the launches of a single call."""
  for n, kind, method in ((65, "q8", lr.COMPLETE), (257, "q3", lr.AVERAGE),
                          (128, "cont", lr.AVERAGE)):
    want = lr.reference(kind, n, method)[0]
    for form in list_forms(n, method):
      assert same_bits(run_linkage(handle, form, method, [lr.cosines(kind, n)])[0], want), form


# ---- c: verdict forms ----------------------------------------------------------------------

def thresholds_of(z):
  heights = np.unique(z[:, 2])
  picks = {heights[0], heights[len(heights) // 2], heights[-1]}
  out = set()
  for v in picks:
    out.update((v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)))
  out.update((heights[-1] + 1.0, heights[0] - 1.0))
  return sorted(out)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SMALL + CHAIN_ONLY)
def test_verdict_records(handle, n, kind):
  z = lr.reference(kind, n, lr.AVERAGE)[0]
  c = lr.cosines(kind, n)
  forms = (CHAIN_VERDICT, LDS_VERDICT) if n <= 128 else (CHAIN_VERDICT,)
  for t in thresholds_of(z):
    want = lr.verdict_record(z, t)
    for form in forms:
      got = run_linkage(handle, form, lr.AVERAGE, [c], threshold=t)[0]
      assert same_bits(got, want), (form, t, got, want)


def test_verdict_tied_heights_shared_threshold(handle):
  """Several members under one threshold at a height many of their merges share."""
  picks = [("q3", 64), ("q8", 65), ("q1", 17), ("clip", 128), ("q8", 127)]
  cs = [lr.cosines(kind, n) for kind, n in picks]
  zs = [lr.reference(kind, n, lr.AVERAGE)[0] for kind, n in picks]
  for t in (0.125, 0.25, 0.375, 0.5, 1.0):
    for form in (CHAIN_VERDICT, LDS_VERDICT):
      got = run_linkage(handle, form, lr.AVERAGE, cs, threshold=t)
      for g, z in zip(got, zs):
        assert same_bits(g, lr.verdict_record(z, t)), (form, t)


# ---- d: independence, table offset, members left alone ---------------------------------------

MIXED = (("q8", 65), ("q1", 1), ("q3", 17), ("clip", 128), ("q1", 0), ("cont", 64), ("chain", 3),
         ("q8", 2), ("chain", 127))
MIXED_CHAIN = MIXED + (("q3", 129), ("chain", 257))


def mixed_members(form, order):
  members = list(MIXED if form in (BATCH_LDS, POOL_LDS, LDS_VERDICT) else MIXED_CHAIN)
  if order:
    members = [members[i] for i in np.random.default_rng(11).permutation(len(members))]
  return members


def member_cosines(kind, n):
  return lr.cosines(kind, n) if n >= 2 else np.ones((n, n))


@pytest.mark.parametrize("order", (0, 1))
@pytest.mark.parametrize("form", range(7))
def test_mixed_batch_offset_and_members_left_alone(handle, form, order):
  members = mixed_members(form, order)
  cs = [member_cosines(kind, n) for kind, n in members]
  method = lr.AVERAGE
  verdict = form in (CHAIN_VERDICT, LDS_VERDICT)
  first = 0 if form in (SINGLE, POOL) else 2
  bad = None
  if form not in (POOL, POOL_LDS):
    bad = np.zeros(len(members), dtype=np.int32)
    bad[[i for i, (_, n) in enumerate(members) if n >= 17][1]] = 1
  threshold = 0.375
  got = run_linkage(handle, form, method, cs, first=first, threshold=threshold, bad=bad)
  touched = 0
  for i, ((kind, n), g) in enumerate(zip(members, got)):
    if i < first or n < 2 or (bad is not None and bad[i]):
      assert np.all(g == FILL), (i, kind, n)
      continue
    touched += 1
    alone = run_linkage(handle, form, method, [cs[i]], threshold=threshold)[0]
    assert same_bits(g, alone), (i, kind, n)
    z = lr.reference(kind, n, method)[0]
    assert same_bits(g, lr.verdict_record(z, threshold) if verdict else z), (i, kind, n)
  assert touched >= 4


def test_arguments_are_checked_before_a_launch(handle):
  c = [lr.cosines("q3", 129)]
  small = [lr.cosines("q3", 17)]
  for form, method, cs, kw in ((BATCH_LDS, lr.AVERAGE, c, {}), (POOL_LDS, lr.AVERAGE, c, {}),
                               (LDS_VERDICT, lr.AVERAGE, c, {}),
                               (BATCH_LDS, lr.COMPLETE, small, {}),
                               (CHAIN_VERDICT, lr.COMPLETE, small, {}), (7, lr.AVERAGE, small, {}),
                               (BATCH, 3, small, {}), (BATCH, lr.AVERAGE, small, {"first": 1}),
                               (POOL, lr.AVERAGE, small + small, {"first": 1}),
                               (BATCH, lr.AVERAGE, [np.ones((1, 1))], {}),
                               (BATCH, lr.AVERAGE, small, {"cut": (18, 0.0)})):
    with pytest.raises(ValueError):
      run_linkage(handle, form, method, cs, **kw)


# ---- e: labels through the cut ---------------------------------------------------------------

def sklearn_labels(d, method, **how):
  model = AgglomerativeClustering(metric="precomputed", linkage=lr.METHOD_NAMES[method], **how)
  return model.fit_predict(d)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind,n", [("q3", 17), ("q8", 64), ("q3", 65), ("q8", 128), ("q1", 63),
                                    ("q3", 129), ("q8", 257), ("q3", 1025)])
def test_labels_through_the_cut(handle, kind, n, method):
  c = lr.cosines(kind, n)
  d = lr.distances(c).copy()
  np.fill_diagonal(d, 0.0)
  heights = np.unique(lr.reference(kind, n, method)[0][:, 2])
  tied = float(heights[len(heights) // 2])
  cuts = [(k, 0.0) for k in (1, 2, 7, n)] + [(0, tied)]
  forms = list_forms(n, method) if n <= 257 else [BATCH]
  for k, t in cuts:
    how = {"n_clusters": k} if k else {"n_clusters": None, "distance_threshold": t}
    want = sklearn_labels(d, method, **how)
    for form in forms:
      _, labels = run_linkage(handle, form, method, [c], cut=(k, t))
      assert np.array_equal(labels[0], want), (form, k, t)


# ---- f: equal rows, equal distances ----------------------------------------------------------

def device_distances(handle, route, x):
  n, d = x.shape
  out = np.full((n, n), np.nan)
  handle.check(handle.lib.sc_stage_cosine_distances(handle.raw, route, _lib.as_double_p(x), n, d,
                                                    _lib.as_double_p(out)))
  return out


@functools.lru_cache(maxsize=None)
def split_tail_shape():
  """The smallest (n, d) at which launch_variant (gemm_f64.hip) runs a full wave of whole tiles
  AND splits the leftover tiles over K, so that columns of one matrix are summed in two ways:
  more upper-triangle tiles than workgroup slots (2 per CU), and 16 k-tiles of 16."""
  lib = _lib.load()
  name, arch = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128)
  cus, mem = ctypes.c_int(0), ctypes.c_int64(0)
  assert lib.sc_device_info(0, name, 128, arch, 128, ctypes.byref(cus), ctypes.byref(mem)) == 0
  slots = 2 * cus.value
  d = 256  # 16 k-tiles: two chunks of the 8 a split needs
  for tm in range(1, 64):
    tiles = tm * (tm + 1) // 2
    full = tiles // slots * slots
    rem = tiles - full
    if full > 0 and rem > 0 and min(slots // rem, (d // 16) // 8) >= 2:
      return (tm - 1) * 128 + 1, d
  raise AssertionError("no such shape")


def check_distance_routes(handle, x, pairs):
  for route in (0, 1):
    dist = device_distances(handle, route, x)
    assert np.isfinite(dist).all()
    assert same_bits(dist, dist.T.copy()), route
    # the whole column, bitwise -- with the two rows of the pair itself exchanged: a row's
    # distance to itself is the stored 0, its distance to its copy the computed 1 - x.x (so it
    # is in scipy's squareform(pdist(.)) as well)
    for copy, original in pairs:
      other = dist[:, original].copy()
      other[[copy, original]] = other[[original, copy]]
      assert same_bits(dist[:, copy], other), (route, copy, original)
    assert np.all(np.diag(dist) == 0.0)


@pytest.mark.parametrize("n,d", [(65, 24), (300, 24)])
def test_equal_rows_equal_distances(handle, n, d):
  x, pairs = lr.duplicates(n, d)
  check_distance_routes(handle, x, pairs)


def test_equal_rows_equal_distances_split_k_tail(handle):
  n, d = split_tail_shape()
  assert n < 4096  # (both routes: the batch hands 4096 rows and more to the single call)
  x, pairs = lr.duplicates(n, d)
  check_distance_routes(handle, x, pairs)


def test_distance_diagonal_within_one_ulp(handle):
  """The diagonal: zeros or values of at most one ulp of 1 (2^-52).

  1 - x.x of a unit row does not meet that: a row is divided by its rounded norm and multiplied
  with itself over d terms, about (d / 2 + 2) roundings of 2^-53.  Measured on an MI355X before
  the distance kernels wrote the self-distance as the zero it is, largest diagonal value of D:
    n = 65, d = 24     single call 4.44e-16 (2.0 ulp)   batch 4.44e-16 (2.0 ulp)
    n = 300, d = 24    single call 4.44e-16 (2.0 ulp)   batch 4.44e-16 (2.0 ulp)
    n = 3969, d = 256  single call 1.44e-15 (6.5 ulp)
  The kernels now store 0 at row == column, as scipy's squareform(pdist(.)) has it; no scan or
  update reads the diagonal, so every merge list is the same as before."""
  worst = 0.0
  for n, d in ((65, 24), (300, 24)):
    x, _ = lr.duplicates(n, d)
    for route in (0, 1):
      diag = np.diag(device_distances(handle, route, x))
      print("route %d n %d d %d: largest diagonal value %.3g = %.1f ulp" %
            (route, n, d, diag.max(), diag.max() / 2.0 ** -52))
      assert diag.min() >= 0.0
      worst = max(worst, diag.max())
  assert worst <= 2.0 ** -52, worst


def numbering_is_settled(x, linkage, how):
  """Does the data settle sklearn's label NUMBERING at this cut?  Label i is the i-th node id of
  the cut's heap, and a node's id is n + its rank among the merge heights.  Two equal rows merge
  at a height that is rounding noise (some 1e-16, in scipy's pdist as in the device's normalised
  product, and not the same noise), so the rank of such a pair among the other pairs -- its id --
  is noise as well: where one of them is a cluster of the cut, only the partition is settled."""
  n = x.shape[0]
  tree = scipy_linkage(pdist(x, "cosine"), linkage)
  _, nodes = lr.cut_tree(tree, n, how.get("n_clusters", 0), how.get("distance_threshold", 0.0))
  return all(v < n or tree[v - n, 2] > 1e-9 for v in nodes)


def same_partition(a, b):
  pairs = set(zip(a.tolist(), b.tolist()))
  return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


@pytest.mark.parametrize("linkage", ("complete", "average"))
@pytest.mark.parametrize("n,d", [(65, 24), (300, 24)])
def test_public_clustering_on_duplicate_rows(n, d, linkage):
  x, _ = lr.duplicates(n, d)
  y, _ = lr.duplicates(n + 7, d, seed=4)
  settled = 0
  for how in ({"n_clusters": 2}, {"n_clusters": 4}, {"n_clusters": 10},
              {"distance_threshold": 0.5}):
    want = [so.agglomerative(a, linkage=linkage, **how) for a in (x, y)]
    got = [utils.cosine_agglomerative_clustering(a, linkage=linkage, **how) for a in (x, y)]
    batch = utils.cosine_agglomerative_clustering_batch([x, y], linkage=linkage, **how)
    for a, w, g, b in zip((x, y), want, got, batch):
      assert np.array_equal(g, b), how  # the two routes agree in any case
      assert same_partition(g, w), how
      if numbering_is_settled(a, linkage, how):
        settled += 1
        assert np.array_equal(g, w), how
  assert settled >= 4
