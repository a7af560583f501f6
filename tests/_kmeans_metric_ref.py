"""The k-means stage under a `custom_dist` other than cosine, as a TRACE in plain NumPy:
`_kmeans_ref.trace` with the distance of its loop replaced.  Seeding and the Lloyd step do not
read the metric (reference custom_distance_kmeans.py:39-43), so they are `_kmeans_ref.trace`'s own;
only the loop (:118-141) is restated here, statement for statement, around `metric_cdist`.

Distances are scipy's definitions (scipy/spatial/src/distance_impl.h), as csrc/kmeans_common.h
lists them:
  euclidean    sqrt(sum (u - v)^2)            sqeuclidean  sum (u - v)^2
  cityblock    sum |u - v|                    chebyshev    max |u - v|
  braycurtis   sum |u - v| / sum |u + v|      canberra     sum |u - v| / (|u| + |v|), 0 / 0 = 0
  correlation  the cosine distance of the operands centred by their own means (rows and centroids)

Shared by tests/test_kmeans_metric_trace_reference_host.py (CPU: the trace against
spectral_oracle.run_kmeans_metric, scipy's cdist and the kmeans_metrics.npz goldens; the margin
and cap conditions of every input) and tests/test_gpu_kmeans_metric_chain.py.
"""

import functools

import numpy as np

import _kmeans_ref as kr

LD = kr.LD
METRICS = ("euclidean", "sqeuclidean", "cityblock", "chebyshev", "correlation", "braycurtis",
           "canberra")

# `_kmeans_ref.overlapping` arguments: G = 1 / 2 / 3 / 6 workgroups of 128 rows with a ragged last
# one, every register width of the chain (k <= 8, <= 16, <= 32)
CASES = [(129, 2, 1.0, 1), (100, 2, 3.0, 1), (129, 3, 1.0, 1), (300, 9, 1.0, 1),
         (300, 17, 3.0, 1), (129, 20, 1.0, 1), (300, 32, 3.0, 1), (700, 21, 1.0, 1)]
SINGLE_CASE = (300, 9, 1.0, 1)      # the single-workgroup kernel, held to the same reference
GROUP_MEMBERS = [(100, 2, 3.0, 1), (129, 9, 1.0, 1), (300, 17, 3.0, 1), (700, 21, 1.0, 1)]
GROUP_METRICS = ("euclidean", "cityblock", "correlation")  # no / no / centred per-row work
MAX_ITER_CASE = (300, 7, 3.0, 1)
K1_CASE = (129, 1, 3.0, 1)


def cases_of(metric):
  """correlation with k = 2: a centred pair is (a, -a), so every distance is 0 or 2 up to
  rounding and nothing is decided by more than that -- left out."""
  return [c for c in CASES if not (metric == "correlation" and c[1] == 2)]


def group_members_of(metric):
  return [c for c in GROUP_MEMBERS if not (metric == "correlation" and c[1] == 2)]


def metric_cdist(x, c, metric):
  """scipy cdist(x, c, metric) in the dtype of x (longdouble or float64)."""
  if metric == "correlation":
    x = x - x.mean(axis=1, keepdims=True)
    c = c - c.mean(axis=1, keepdims=True)
    return kr._cosine_cdist(x, c)
  u, v = x[:, None, :], c[None, :, :]
  d = np.abs(u - v)
  if metric == "euclidean":
    return np.sqrt((d * d).sum(axis=2))
  if metric == "sqeuclidean":
    return (d * d).sum(axis=2)
  if metric == "cityblock":
    return d.sum(axis=2)
  if metric == "chebyshev":
    return d.max(axis=2)
  if metric == "braycurtis":
    return d.sum(axis=2) / np.abs(u + v).sum(axis=2)
  if metric == "canberra":
    den = np.abs(u) + np.abs(v)
    return np.where(den > 0, d / np.where(den > 0, den, 1), 0).sum(axis=2)
  raise ValueError(metric)


def trace_metric(e, k, metric, max_iter=300, dtype=LD):
  """`_kmeans_ref.trace(e, k, max_iter, dtype)` with `metric` in the loop; the same keys."""
  e = np.ascontiguousarray(e, dtype=np.float64)
  n = e.shape[0]
  # everything through the Lloyd step (the cosine passes of this call are dropped)
  t = {key: val for key, val in kr.trace(e, k, 1, dtype).items()
       if key in ("col_means", "rounds", "seeds", "trials", "lloyd_labels", "lloyd_margin",
                  "lloyd_centroids")}
  x = e.astype(dtype)
  order = np.arange(n)
  cent = t["lloyd_centroids"].copy()
  prev = dtype(0)
  passes = []
  for it in range(max_iter + 1):
    dist = metric_cdist(x, cent, metric)
    labels = dist.argmin(axis=1)
    mean_d = kr._row_sum(dist[np.arange(n), labels], order) / dtype(n)
    fired = bool(mean_d <= prev and mean_d >= (1 - 0.001) * prev)
    if it == max_iter and not fired:
      stop_margin = np.inf
    elif k == 1 or (it >= 2 and np.array_equal(passes[it - 1]["labels"],
                                               passes[it - 2]["labels"])):
      # the fixed point: the same assignment twice gives the same centroids and distances, bit
      # for bit, in any arithmetic (k = 1: nothing to assign; its pass count is not compared
      # with this trace)
      stop_margin = np.inf
    elif prev == 0:
      stop_margin = float(mean_d)
    else:
      s1, s2 = float(prev - mean_d), float(mean_d - (1 - 0.001) * prev)
      stop_margin = (min(s1, s2) if fired else max(-s1, -s2)) / max(float(prev), 1.0)
    passes.append({"labels": labels.astype(np.int64), "mean_dist": mean_d,
                   "assign_margin": kr._two_smallest_gap(dist), "stop_margin": stop_margin,
                   "centroids": cent.copy()})
    if fired or it == max_iter:
      break
    prev = mean_d
    for c in range(k):
      members = np.where(labels == c)[0]
      if members.any():  # reference quirk (:137-138): truthiness of the member INDICES
        cent[c] = kr._row_sum(x, order, labels == c) / dtype(members.size)
  t["passes"] = passes
  t["first_labels"] = passes[0]["labels"]
  t["mean_dist"] = np.array([p["mean_dist"] for p in passes], dtype=dtype)
  t["iterations"] = len(passes)
  t["centroids"] = passes[-1]["centroids"]
  t["labels"] = passes[-1]["labels"]
  return t


@functools.lru_cache(maxsize=None)
def metric_reference(case, metric, max_iter=300):
  """(longdouble trace, plain float64 trace, `_kmeans_ref.tolerances`) of one case, once."""
  e = kr.overlap_input(case)
  ref = trace_metric(e, case[1], metric, max_iter, LD)
  plain = trace_metric(e, case[1], metric, max_iter, np.float64)
  return ref, plain, kr.tolerances(ref, plain)
