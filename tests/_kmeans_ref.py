"""The k-means stage (reference custom_distance_kmeans.py:13-141, custom_dist="cosine") written as
a TRACE in plain NumPy: every intermediate quantity the device kernels of csrc/kmeans_chain.hip and
csrc/kmeans.hip compute, and next to each discrete decision how far it was from going the other
way.  Also the inputs of tests/test_gpu_kmeans_kernels.py and the tolerance rule those tests use.

Shared by tests/test_kmeans_trace_reference_host.py (CPU: the trace against sklearn, against
spectral_oracle.run_kmeans and the kmeans.npz goldens; the margin, cap and pass-count conditions
of every committed input) and by the GPU tests, so that what the kernels are compared with is
itself tested.

`trace(e, k, max_iter, dtype)`: dtype = np.longdouble is the reference of every quantity compared
with a tolerance; dtype = np.float64 is the plain NumPy oracle (the statements of
spectral_oracle.kmeanspp_seeds / lloyd_one_step / cosine_cdist / custom_kmeans_cosine), whose
deviation from the longdouble trace is the yardstick of the tolerances (`tolerances`).

Margins (all relative, a decision with nothing to decide has margin inf):
  candidate row   distance of rand * pot to the two neighbouring cumulative sums, over pot
  winner          (second-best - best trial potential) / best, over trials with another row
  assignment      second-smallest minus smallest distance of the row (absolute: distances are
                  O(1) in the cosine loop; relative to the largest |distance| in the Lloyd step)
  stop rule       slack of `mean_d <= prev` and `mean_d >= 0.999 prev`, over max(prev, 1) (relative
                  to prev, and no smaller in absolute terms: distances are 1 - cos): the smaller
                  one when the rule fired, the larger violation when it did not; inf at the
                  fixed point (the assignment of the two passes before was the same one, so this
                  pass repeats the last one's arithmetic on the same numbers) and for k = 1
"""

import functools
import math

import numpy as np

import spectral_oracle as so

LD = np.longdouble
MARGIN = 1e-9   # condition on every seeding, Lloyd-assignment and stop-rule margin of an input
LABEL_CAP = 0.01  # share of a case's rows that may sit closer to a tie than the tolerance


def _row_sum(a, order, mask=None):
  """Sum over the rows of `a`, added in the order `order` (members of `mask` only)."""
  idx = order if mask is None else order[mask[order]]
  return a[idx].sum(axis=0)


def _sq_dists(xc, xsq, rows):
  # sklearn _euclidean_distances(X[rows], X, squared=True), as spectral_oracle._sq_dists_to
  c = xc[rows]
  csq = np.einsum("ij,ij->i", c, c)
  d = -2.0 * (c @ xc.T)
  d += csq[:, None]
  d += xsq[None, :]
  np.maximum(d, 0, out=d)
  return d


def _cosine_cdist(x, c):
  # scipy cdist(metric="cosine"), as spectral_oracle.cosine_cdist
  nu = np.sqrt(np.einsum("ij,ij->i", x, x))
  nv = np.sqrt(np.einsum("ij,ij->i", c, c))
  cos = (x @ c.T) / (nu[:, None] * nv[None, :])
  cos = np.where(np.abs(cos) > 1.0, np.copysign(1.0, cos), cos)
  return 1.0 - cos


def _two_smallest_gap(d):
  if d.shape[1] < 2:
    return np.full(d.shape[0], np.inf)
  p = np.partition(d, 1, axis=1)
  return (p[:, 1] - p[:, 0]).astype(np.float64)


def trace(e, k, max_iter=300, dtype=LD, row_order=None):
  """The whole stage on the (n, k) array e.  row_order: the order in which every sum over rows
  is added (the cumulative sum of k-means++ stays in row order: it is a sequence, not a sum)."""
  e = np.ascontiguousarray(e, dtype=np.float64)
  n = e.shape[0]
  assert e.shape[1] == k and n >= k and max_iter > 0
  order = np.arange(n) if row_order is None else np.asarray(row_order)
  x = e.astype(dtype)
  t = {}
  mean = _row_sum(x, order) / dtype(n)
  t["col_means"] = mean
  xc = x - mean
  xsq = np.einsum("ij,ij->i", xc, xc)

  # ---- k-means++ (sklearn 1.7.2 _kmeans_plusplus, unit weights, RandomState(0))
  rng = so.Mt19937(0)
  trials = 2 + int(math.log(k))
  cdf = np.cumsum(np.ones(n) / float(n))
  cdf /= cdf[-1]
  first = int(np.searchsorted(cdf, rng.next_double(), side="right"))
  seeds = [first]
  closest = _sq_dists(xc, xsq, np.array([first]))[0]
  pot = _row_sum(closest, order)
  rounds = []
  for _ in range(1, k):
    u = np.array([rng.next_double() for _ in range(trials)])
    r = u.astype(dtype) * pot
    cum = np.cumsum(closest)
    cand = np.searchsorted(cum, r)
    np.clip(cand, None, n - 1, out=cand)
    cand_margin = np.full(trials, np.inf)
    if pot > 0:
      for i in range(trials):
        c = int(cand[i])
        up = (cum[c] - r[i]) if r[i] <= cum[c] else (r[i] - cum[c])  # (the clip decided)
        lo = (r[i] - cum[c - 1]) if c > 0 else np.inf
        cand_margin[i] = float(min(up, lo) / pot)
    d = _sq_dists(xc, xsq, cand)
    np.minimum(closest, d, out=d)
    pots = np.array([_row_sum(d[i], order) for i in range(trials)], dtype=dtype)
    b = int(np.argmin(pots))
    others = [float((pots[i] - pots[b]) / pots[b]) if pots[b] > 0 else np.inf
              for i in range(trials) if cand[i] != cand[b]]
    rounds.append({"pot": pot, "rand": r, "candidates": cand.astype(np.int64),
                   "candidate_margin": cand_margin, "trial_potentials": pots, "winner": b,
                   "winner_margin": min(others) if others else np.inf})
    pot, closest = pots[b], d[b]
    seeds.append(int(cand[b]))
  t["rounds"] = rounds
  t["seeds"] = np.array(seeds, dtype=np.int64)
  t["trials"] = trials

  # ---- one sklearn Lloyd step on the centred data (an empty cluster keeps its seed)
  centers = xc[t["seeds"]].copy()
  dl = np.einsum("ij,ij->i", centers, centers)[None, :] - 2.0 * (xc @ centers.T)
  lab = np.argmin(dl, axis=1)
  scale = float(np.max(np.abs(dl))) if dl.size else 1.0
  t["lloyd_labels"] = lab.astype(np.int64)
  t["lloyd_margin"] = _two_smallest_gap(dl) / (scale if scale > 0 else 1.0)
  new = centers.copy()
  for c in range(k):
    m = lab == c
    if m.any():
      new[c] = _row_sum(xc, order, m) / dtype(int(m.sum()))
  cent = new + mean
  t["lloyd_centroids"] = cent.copy()

  # ---- CustomKMeans.predict (:85-141), cosine
  prev = dtype(0)
  passes = []
  row0_alone = empty_in_loop = False
  for it in range(max_iter + 1):
    dist = _cosine_cdist(x, cent)
    labels = dist.argmin(axis=1)
    mean_d = _row_sum(dist[np.arange(n), labels], order) / dtype(n)
    fired = bool(mean_d <= prev and mean_d >= (1 - 0.001) * prev)
    if it == max_iter and not fired:
      stop_margin = np.inf
    elif k == 1 or (it >= 2 and np.array_equal(passes[it - 1]["labels"],
                                               passes[it - 2]["labels"])):
      # nothing to decide.  Two passes from the same assignment compute the same centroids and
      # so the same distances, bit for bit, in any arithmetic: mean_d == prev.  k = 1: every
      # cosine is exactly +-1, every distance exactly 0 or 2, the mean distances exact.
      assert fired or k == 1
      stop_margin = np.inf
    elif prev == 0:
      stop_margin = float(mean_d)  # (the rule fires at pass 0 only for mean_d == 0)
    else:
      s1, s2 = float(prev - mean_d), float(mean_d - (1 - 0.001) * prev)
      # relative to prev, and absolute as well: a cosine distance is 1 - cos, known to an
      # absolute 1e-16, so a prev of rounding size decides nothing
      stop_margin = (min(s1, s2) if fired else max(-s1, -s2)) / max(float(prev), 1.0)
    passes.append({"labels": labels.astype(np.int64), "mean_dist": mean_d,
                   "assign_margin": _two_smallest_gap(dist), "stop_margin": stop_margin,
                   "centroids": cent.copy()})
    if fired or it == max_iter:
      break
    prev = mean_d
    for c in range(k):
      members = np.where(labels == c)[0]
      if members.size == 0:
        empty_in_loop = True
      if members.size == 1 and members[0] == 0 and float(np.max(np.abs(cent[c] - x[0]))) > 1e-3:
        row0_alone = True  # (a centroid that is not row 0 itself: keeping it shows)
      if members.any():  # reference quirk (:137-138): truthiness of the member INDICES
        cent[c] = _row_sum(x, order, labels == c) / dtype(members.size)
  t["passes"] = passes
  t["first_labels"] = passes[0]["labels"]
  t["mean_dist"] = np.array([p["mean_dist"] for p in passes], dtype=dtype)
  t["iterations"] = len(passes)
  t["centroids"] = passes[-1]["centroids"]
  t["labels"] = passes[-1]["labels"]
  t["row0_alone"] = row0_alone      # an update kept the centroid of a cluster that had shrunk to row 0
  t["empty_in_loop"] = empty_in_loop  # ... or a cluster without members
  return t


def decision_margin(t):
  """The smallest seeding, Lloyd-assignment and stop-rule margin of a trace."""
  m = [np.inf]
  for r in t["rounds"]:
    m += [float(np.min(r["candidate_margin"])), float(r["winner_margin"])]
  m.append(float(np.min(t["lloyd_margin"])))
  m += [float(p["stop_margin"]) for p in t["passes"]]
  return min(m)


# ------------------------------------------------------------------------------ tolerances
CONTINUOUS = ("col_means", "lloyd_centroids", "mean_dist", "centroids")


def tolerances(ref, plain):
  """Per continuous quantity: (tolerance, yardstick).  yardstick = the deviation of the plain
  float64 NumPy oracle from the longdouble trace; the device, which adds in another order in the
  same precision, gets 8 x that, and never less than 4 ulp of the quantity's largest magnitude."""
  out = {}
  for name in CONTINUOUS:
    a, b = np.asarray(ref[name]), np.asarray(plain[name], dtype=LD)
    assert a.shape == b.shape, name
    yard = float(np.max(np.abs(a - b))) if a.size else 0.0
    floor = 4.0 * float(np.spacing(np.float64(np.max(np.abs(a))))) if a.size else 0.0
    out[name] = (max(8.0 * yard, floor), yard)
  return out


def uncertain_rows(ref, tol):
  """Per pass the rows whose assignment margin in the reference is below tol."""
  return [p["assign_margin"] < tol for p in ref["passes"]]


# ------------------------------------------------------------------------------ inputs
def overlapping(n, k, noise, seed):
  """n rows around k centres ~ N(0, I_k), noise `noise`: overlapping clusters, many passes."""
  rng = np.random.default_rng(seed)
  centres = rng.standard_normal((k, k))
  member = rng.integers(0, k, size=n)
  return centres[member] + noise * rng.standard_normal((n, k))


def exact_pairs(n, k, seed, span=6):
  """Small integers in +- row pairs (an odd n gets one zero row... which the cosine distance
  cannot take, so the last THREE rows are a, b, -(a + b)): every column sums to 0, and every
  sum through the Lloyd step is an exact integer in any order."""
  rng = np.random.default_rng(seed)
  def rows(m):
    r = rng.integers(-span, span + 1, size=(m, k))
    r[np.all(r == 0, axis=1), 0] = 1
    return r
  if n % 2 == 0:
    half = rows(n // 2)
    out = np.empty((n, k), dtype=np.int64)
    out[0::2], out[1::2] = half, -half
  else:
    half = rows((n - 3) // 2)
    out = np.empty((n, k), dtype=np.int64)
    out[0:n - 3:2], out[1:n - 3:2] = half, -half
    a, b = rows(1)[0], rows(1)[0]
    if np.all(a + b == 0):
      b = b.copy()
      b[0] += 1
    out[n - 3], out[n - 2], out[n - 1] = a, b, -(a + b)
  return out.astype(np.float64)


def exact_duplicates(n, k, distinct, seed, dup_first=0, dup_last=0):
  """+- pairs of only `distinct` different directions (mean exactly 0).  distinct < k: after
  `distinct` seeds the k-means++ potential is exactly 0 (the r == 0 clause of the searchsorted,
  flat cumulative sums, an empty cluster that keeps its seed).  dup_first / dup_last: that many
  further +- pairs of copies of row 0 / row n - 1 placed in the middle."""
  rng = np.random.default_rng(seed)
  if distinct == 3:  # a, b, -(a + b) in turn
    assert n % 3 == 0 and dup_first == 0 and dup_last == 0
    a = rng.integers(1, 6, size=k)
    b = -rng.integers(1, 6, size=k)
    b[0] = 7
    return np.tile(np.stack([a, b, -(a + b)]), (n // 3, 1)).astype(np.float64)
  assert n % 2 == 0 and distinct % 2 == 0
  base = rng.integers(1, 6, size=(distinct // 2, k)) * rng.choice([-1, 1], size=(distinct // 2, k))
  pick = rng.integers(0, distinct // 2, size=n // 2)
  pick[:distinct // 2] = np.arange(distinct // 2)
  out = np.empty((n, k), dtype=np.int64)
  out[0::2], out[1::2] = base[pick], -base[pick]
  mid = (n // 4) * 2
  for j in range(dup_first):
    out[mid + 2 * j], out[mid + 2 * j + 1] = out[0], -out[0]
  for j in range(dup_last):
    out[mid + 2 * (dup_first + j)], out[mid + 2 * (dup_first + j) + 1] = -out[n - 1], out[n - 1]
  return out.astype(np.float64)


# name -> (builder, args).  Exact-arithmetic cases: compared bit for bit through the Lloyd step.
EXACT_CASES = {
    "zero_potential_60x4": (exact_duplicates, (60, 4, 3, 11)),
    "zero_potential_64x4": (exact_duplicates, (64, 4, 2, 11)),
    "zero_potential_260x9": (exact_duplicates, (260, 9, 6, 12)),
    "dup_row0_rowlast_200x5": (exact_duplicates, (200, 5, 40, 13, 6, 6)),
    "pairs_4x4": (exact_pairs, (4, 4, 31)),
    "pairs_16x16": (exact_pairs, (16, 16, 32)),
    "pairs_32x32": (exact_pairs, (32, 32, 33)),
    "pairs_127x3": (exact_pairs, (127, 3, 21)),
    "pairs_128x3": (exact_pairs, (128, 3, 22)),
    "pairs_129x3": (exact_pairs, (129, 3, 23)),
    "pairs_2048x8": (exact_pairs, (2048, 8, 24)),
    "pairs_2049x8": (exact_pairs, (2049, 8, 25)),
    "pairs_300x17": (exact_pairs, (300, 17, 26)),
    "pairs_700x32": (exact_pairs, (700, 32, 27)),
}

# (n, k, noise, generator seed); the seeds were searched on the CPU so that decision_margin of
# the longdouble trace is >= MARGIN (tests/test_kmeans_trace_reference_host.py asserts it).
# n = k with k >= 2 cannot meet it: every row is its own cluster, every distance is rounding
# noise around 0 and the stop rule compares noise with noise; the smallest n (and the first
# generator seed) whose trace has all its margins stands in, and n = k itself is among the
# exact-arithmetic inputs, where seeds and Lloyd step are compared bit for bit.
OVERLAP_CASES = [
    (1, 1, 1.0, 1), (129, 1, 3.0, 1),
    (3, 2, 1.0, 9), (129, 2, 1.0, 1), (2049, 2, 3.0, 1),
    (4, 3, 3.0, 17), (129, 3, 1.0, 1), (129, 3, 3.0, 1), (2049, 3, 3.0, 1),
    (8, 7, 1.0, 77), (300, 7, 3.0, 1),
    (9, 8, 3.0, 47), (700, 8, 1.0, 1), (2049, 8, 3.0, 1),
    (11, 9, 1.0, 13), (300, 9, 1.0, 1), (300, 9, 3.0, 1),
    (18, 16, 3.0, 116), (700, 16, 1.0, 1),
    (20, 17, 1.0, 11), (300, 17, 3.0, 1), (2049, 17, 1.0, 1),
    (23, 20, 3.0, 32), (129, 20, 1.0, 1),
    (26, 21, 1.0, 34), (700, 21, 1.0, 1), (700, 21, 3.0, 1),
    (39, 32, 1.0, 167), (300, 32, 3.0, 1), (2049, 32, 1.0, 1),
]
BOUNDARY_CASES = [(7680, 32, 1.0, 1), (7681, 32, 1.0, 1)]   # chain's last n at k = 32 / beyond
SINGLE_CASES = [(300, 33, 1.0, 1), (700, 64, 3.0, 1), (300, 9, 3.0, 1)]  # single-workgroup form
BIG_CASES = [(300, 65, 1.0, 1)]                              # its large-k form
GROUP_MEMBERS = [(100, 2, 3.0, 1), (129, 9, 1.0, 1), (300, 17, 3.0, 1), (2049, 3, 3.0, 1),
                 (700, 21, 1.0, 1)]
MAX_ITER_CASE = (300, 7, 3.0, 1)   # 13 passes; cut at max_iter in {1, 2, 3, 4, 5, 8}
# n <= 200: found on the CPU with `trace`: an update that sees a cluster whose only member is
# row 0 (its centroid stays put), and one that sees a cluster without members
ROW0_ALONE_CASE = (16, 6, 3.0, 1420)
EMPTY_CLUSTER_CASE = (5, 3, 3.0, 528)


def all_overlap_cases():
  seen, out = set(), []
  for c in (OVERLAP_CASES + BOUNDARY_CASES + SINGLE_CASES + BIG_CASES + GROUP_MEMBERS +
            [MAX_ITER_CASE, ROW0_ALONE_CASE, EMPTY_CLUSTER_CASE]):
    if c not in seen:
      seen.add(c)
      out.append(c)
  return out


@functools.lru_cache(maxsize=None)
def exact_input(name):
  fn, args = EXACT_CASES[name]
  e = fn(*args)
  e.setflags(write=False)
  return e


@functools.lru_cache(maxsize=None)
def overlap_input(case):
  e = overlapping(*case)
  e.setflags(write=False)
  return e


@functools.lru_cache(maxsize=None)
def overlap_reference(case, max_iter=300):
  """(longdouble trace, plain float64 trace, tolerances) of one overlapping case, computed once."""
  e = overlap_input(case)
  ref = trace(e, case[1], max_iter, LD)
  plain = trace(e, case[1], max_iter, np.float64)
  return ref, plain, tolerances(ref, plain)
