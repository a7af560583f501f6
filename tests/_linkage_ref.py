"""The reference of the agglomerative linkage kernels (csrc/ahc.hip), in plain NumPy: scipy's
nearest-neighbour-chain loop for complete and average linkage, emitting the RAW merge list the
kernels write -- (x, y, height, size) with x < y slot indices, in chain order -- and counting what
an input exercises (tied scans, ties the previous chain element won, the longest chain, chain
restarts).  `label` is scipy's stable sort by height + union-find relabelling, `cut` sklearn's heap
cut; tests/test_linkage_reference_host.py checks all three against scipy and sklearn.

The arithmetic is the kernels' expression by expression -- d = 1 - clip(c), max(dx, dy),
(float(nx) * dx + float(ny) * dy) / float(nx + ny) -- so in float64 the expectation is bit
equality.  `dtype=np.longdouble` runs the same loop in extended precision (the yardstick of the
continuous inputs).  The three rule arguments are the mutants the host test uses to show that an
input can tell the rules apart: tie="last" (last index of the minimum), prefer_prev=False (`<=`
against the previous chain element), start="last" (a chain restarts at the last live slot).
"""

import functools
import heapq

import numpy as np

COMPLETE, AVERAGE = 1, 2
METHOD_NAMES = {COMPLETE: "complete", AVERAGE: "average"}


def distances(c, dtype=np.float64):
  """d = 1 - clip(c, -1, 1): k_cosine_distance's expression."""
  c = np.asarray(c, dtype=np.float64)
  return (1.0 - np.clip(c, -1.0, 1.0)).astype(dtype)


def nn_chain(d, method, tie="first", prefer_prev=True, start="first", dtype=np.float64):
  """(Z, stats) of the n x n symmetric distance matrix d; Z is (n - 1) x 4 float64."""
  d = np.array(d, dtype=dtype)
  n = d.shape[0]
  inf = dtype(np.inf)
  size = np.ones(n, dtype=np.int64)
  live = np.ones(n, dtype=bool)
  chain = []
  z = np.zeros((max(n - 1, 0), 4), dtype=dtype)
  stats = {"ties": 0, "prev_ties": 0, "max_chain": 0, "restarts": 0, "scans": 0}
  for k in range(n - 1):
    if not chain:
      slots = np.flatnonzero(live)
      chain.append(int(slots[0] if start == "first" else slots[-1]))
      stats["restarts"] += 1
      stats["max_chain"] = max(stats["max_chain"], 1)
    while True:
      x = chain[-1]
      y0 = chain[-2] if len(chain) > 1 else -1
      cur = d[x, y0] if y0 >= 0 else inf
      row = np.where(live, d[x], inf)
      row[x] = inf
      best = row.min()
      cands = np.flatnonzero(row == best)
      stats["scans"] += 1
      if len(cands) > 1:
        stats["ties"] += 1
      besti = int(cands[0] if tie == "first" else cands[-1])
      if y0 >= 0 and best == cur and besti != y0:
        stats["prev_ties"] += 1
      y = y0
      if (best < cur) if prefer_prev else (best <= cur):
        cur, y = best, besti
      if len(chain) > 1 and y == y0:
        break
      chain.append(y)
      stats["max_chain"] = max(stats["max_chain"], len(chain))
    del chain[-2:]
    if x > y:
      x, y = y, x
    nx, ny = int(size[x]), int(size[y])
    z[k] = (x, y, cur, nx + ny)
    size[x], size[y] = 0, nx + ny
    live[x] = False
    m = live.copy()
    m[y] = False
    dx, dy = d[x, m], d[y, m]
    if method == COMPLETE:
      nv = np.maximum(dx, dy)
    else:
      nv = (dtype(nx) * dx + dtype(ny) * dy) / dtype(nx + ny)
    d[y, m] = nv
    d[m, y] = nv
  return z, stats


def label(z, n):
  """scipy's linkage matrix of a raw merge list: stable sort by height, union-find node ids."""
  z = np.asarray(z)
  z = z[np.argsort(z[:, 2], kind="stable")]
  parent = list(range(2 * n - 1))

  def find(v):
    root = v
    while parent[root] != root:
      root = parent[root]
    while parent[v] != root:
      parent[v], v = root, parent[v]
    return root

  out = np.zeros((n - 1, 4))
  for i in range(n - 1):
    xr, yr = find(int(z[i, 0])), find(int(z[i, 1]))
    out[i] = (min(xr, yr), max(xr, yr), z[i, 2], z[i, 3])
    parent[xr] = parent[yr] = n + i
  return out


def cut(z, n, n_clusters=0, distance_threshold=0.0):
  """sklearn's labels of a raw merge list (AgglomerativeClustering: _hc_cut on label(z)):
  n_clusters > 0, or as many clusters as the merges at or above the threshold leave."""
  return cut_tree(label(z, n), n, n_clusters, distance_threshold)[0]


def cut_tree(tree, n, n_clusters=0, distance_threshold=0.0):
  """(labels, nodes) of a scipy linkage matrix: sklearn's heap of node ids (_hc_cut); label i is
  the cluster under nodes[i], so the numbering is the heap array's order of the node ids."""
  children = tree[:, :2].astype(np.int64)
  if n_clusters <= 0:
    n_clusters = int(np.count_nonzero(tree[:, 2] >= distance_threshold)) + 1
  nodes = [-(int(children[-1].max()) + 1)]
  for _ in range(n_clusters - 1):
    a, b = children[-nodes[0] - n]
    heapq.heappush(nodes, -int(a))
    heapq.heappushpop(nodes, -int(b))
  out = np.zeros(n, dtype=np.int64)
  for i, node in enumerate(nodes):
    stack = [-node]
    while stack:
      v = stack.pop()
      if v < n:
        out[v] = i
      else:
        stack.extend(int(c) for c in children[v - n])
  return out, [-node for node in nodes]


# ---- inputs: every builder returns the COSINE matrix c (what the GEMM leaves), float64 -------

def quantised(n, levels, seed=None):
  """Symmetric d with entries j / 8, j uniform in 1 .. levels, zero diagonal; c = 1 - d exact."""
  rng = np.random.default_rng(1000 * n + levels if seed is None else seed)
  a = rng.integers(1, levels + 1, size=(n, n)).astype(np.float64) / 8.0
  d = np.triu(a, 1)
  return 1.0 - (d + d.T)


def long_chain(n):
  """Points on a line with gaps n - 1, n - 2, ..., 1 (over 2^20; 2^22 above n = 1025, so that
  the largest distance stays below 1), d = |p_i - p_j|: every value exact, and the chain grows to
  n elements before the first merge."""
  gaps = np.arange(n - 1, 0, -1, dtype=np.float64)
  p = np.concatenate([[0.0], np.cumsum(gaps)]) / (2.0 ** 20 if n <= 1025 else 2.0 ** 22)
  return 1.0 - np.abs(p[:, None] - p[None, :])


def clip_case(n):
  """A quantised matrix (8 levels) with about a tenth of the cosines replaced by 1 + 2^-40
  (distance 0 after the clip) and as many by -1.5 (distance 2)."""
  c = quantised(n, 8, seed=77000 + n)
  rng = np.random.default_rng(78000 + n)
  iu, ju = np.triu_indices(n, 1)
  pick = rng.random(len(iu))
  for lo, hi, value in ((0.0, 0.1, 1.0 + 2.0 ** -40), (0.1, 0.2, -1.5)):
    sel = (pick >= lo) & (pick < hi)
    c[iu[sel], ju[sel]] = value
    c[ju[sel], iu[sel]] = value
  return c


def continuous(n, d=16):
  """Cosines of real unit rows: two to four loose clusters, no ties, full mantissas."""
  rng = np.random.default_rng(5000 + n)
  k = 2 + n % 3
  centres = rng.standard_normal((k, d))
  x = centres[rng.integers(0, k, size=n)] + 0.7 * rng.standard_normal((n, d))
  x /= np.linalg.norm(x, axis=1, keepdims=True)
  c = np.triu(x @ x.T, 1)
  c = c + c.T
  np.fill_diagonal(c, 1.0)
  return c


def duplicates(n, d, seed=None):
  """(x, pairs): an (n, d) embedding array in which about a third of the rows are exact copies of
  other rows -- of a row in another 128-row tile wherever n has more than one -- and the list of
  (copy, original) index pairs."""
  rng = np.random.default_rng(9000 + n + d if seed is None else seed)
  k = 4
  centres = rng.standard_normal((k, d))
  x = centres[rng.integers(0, k, size=n)] + 0.5 * rng.standard_normal((n, d))
  copies = np.flatnonzero(rng.random(n) < 1.0 / 3.0)
  originals = np.setdiff1d(np.arange(n), copies)
  pairs = []
  for j in copies:
    far = originals[originals // 128 != j // 128]
    src = int(rng.choice(far if len(far) else originals))
    x[j] = x[src]
    pairs.append((int(j), src))
  return np.ascontiguousarray(x), pairs


BUILDERS = {
    "q1": lambda n: quantised(n, 1),
    "q3": lambda n: quantised(n, 3),
    "q8": lambda n: quantised(n, 8),
    "chain": long_chain,
    "clip": clip_case,
    "cont": continuous,
}
EXACT_KINDS = ("q1", "q3", "q8", "chain", "clip")


@functools.lru_cache(maxsize=None)
def cosines(kind, n):
  c = BUILDERS[kind](n)
  c.setflags(write=False)
  return c


@functools.lru_cache(maxsize=None)
def reference(kind, n, method):
  """(Z, stats) of the port on the named input, computed once per process and never changed."""
  z, stats = nn_chain(distances(cosines(kind, n)), method)
  z.setflags(write=False)
  return z, stats


def verdict_record(z, threshold):
  """The two-double record of the verdict kernels for the raw merge list z: the first height in
  chain order that is >= threshold with verdict 0, else the largest height with verdict 1."""
  heights = np.asarray(z)[:, 2]
  hit = np.flatnonzero(heights >= threshold)
  if len(hit):
    return np.array([heights[hit[0]], 0.0])
  return np.array([heights.max(), 1.0])
