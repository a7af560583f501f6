"""Multi-stage streaming clustering (mirror of reference
`spectralcluster/multi_stage_clusterer.py`; Wang et al., "Highly efficient real-time
streaming and fully on-device speaker diarization with multi-stage clustering",
arXiv:2210.13690).

Stage by size of the stream: fewer than L embeddings -> the agglomerative fallback; up to U1
-> the main spectral clusterer; beyond U1 -> a complete-linkage cosine AHC pre-clusterer
compresses the cache to U1 centroids which the main clusterer then clusters; at U2 cached
rows the cache is replaced by those centroids ("dynamic compression").  Every clustering
step runs on the device (AHC: `ahc.hip`; spectral: the hot path); this class is the host
bookkeeping around them, plus the label de-flickering.
"""

from __future__ import annotations

import ctypes
import enum
import typing

import numpy as np

from spectralcluster_amd import _dlpack
from spectralcluster_amd import _lib
from spectralcluster_amd import fallback_clusterer
from spectralcluster_amd import spectral_clusterer
from spectralcluster_amd import utils


class Deflicker(enum.Enum):
  """How the streaming output labels are kept stable (reference :19-28)."""
  NoDeflicker = 1
  OrderBased = 2    # enforce order-based labels
  Hungarian = 3     # match the previous output by an assignment problem


def linear_sum_assignment(cost: np.ndarray, maximize: bool = False):
  """Rectangular linear sum assignment, shortest augmenting paths (D. F. Crouse, "On
  implementing 2D rectangular assignment algorithms", IEEE T-AES 2016) -- the algorithm
  behind `scipy.optimize.linear_sum_assignment`, which the reference calls (:51).  Host
  code: the matrices here are (speakers x speakers).  Returns (row_ind, col_ind), rows
  ascending."""
  c = np.array(cost, dtype=np.float64)
  if c.ndim != 2:
    raise ValueError("expected a matrix (2-D array)")
  if maximize:
    c = -c
  transposed = c.shape[1] < c.shape[0]
  if transposed:
    c = c.T.copy()
  nr, nc = c.shape
  if nr == 0:
    return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
  c = c - c.min()                       # non-negative costs for the dual updates
  u = np.zeros(nr)
  v = np.zeros(nc)
  col4row = -np.ones(nr, dtype=np.int64)
  row4col = -np.ones(nc, dtype=np.int64)
  for cur_row in range(nr):
    shortest = np.full(nc, np.inf)
    path = -np.ones(nc, dtype=np.int64)
    in_rows = np.zeros(nr, dtype=bool)
    in_cols = np.zeros(nc, dtype=bool)
    remaining = list(range(nc - 1, -1, -1))   # columns still open, scanned in this order
    min_val = 0.0
    i = cur_row
    sink = -1
    while sink == -1:
      index = -1
      lowest = np.inf
      in_rows[i] = True
      for it, j in enumerate(remaining):
        reduced = min_val + c[i, j] - u[i] - v[j]
        if reduced < shortest[j]:
          path[j] = i
          shortest[j] = reduced
        # among equally short paths prefer an unassigned column: it ends the search
        if shortest[j] < lowest or (shortest[j] == lowest and row4col[j] == -1):
          lowest = shortest[j]
          index = it
      min_val = lowest
      if not np.isfinite(min_val):
        raise ValueError("cost matrix is infeasible")
      j = remaining[index]
      if row4col[j] == -1:
        sink = j
      else:
        i = row4col[j]
      in_cols[j] = True
      remaining[index] = remaining[-1]
      remaining.pop()
    u[cur_row] += min_val
    for r in range(nr):
      if in_rows[r] and r != cur_row:
        u[r] += min_val - shortest[col4row[r]]
    for col in range(nc):
      if in_cols[col]:
        v[col] -= min_val - shortest[col]
    j = sink
    while True:                          # augment along the path back to cur_row
      r = path[j]
      row4col[j] = r
      col4row[r], j = j, col4row[r]
      if r == cur_row:
        break
  if transposed:
    order = np.argsort(col4row)
    return col4row[order], order.astype(np.int64)
  return np.arange(nr, dtype=np.int64), col4row


def match_labels(current: np.ndarray, previous: np.ndarray) -> np.ndarray:
  """Rename the labels of `current` (one element longer) so that they agree with
  `previous` as much as possible (reference :31-63)."""
  current = utils.enforce_ordered_labels(np.asarray(current)).astype(np.int32)
  previous = np.asarray(previous).astype(np.int32)
  cropped = current[:-1]
  if cropped.shape != previous.shape:
    raise ValueError("current must have one more element than previous .")
  num_current = max(cropped) + 1
  num_previous = max(max(previous) + 1, num_current)
  # overlap[i, j]: how often label i now coincides with label j before
  overlap = np.zeros((num_current, num_previous), dtype=np.int32)
  np.add.at(overlap, (cropped, previous), 1)
  rows, cols = linear_sum_assignment(overlap, maximize=True)
  renamed = dict(zip(rows.tolist(), cols.tolist()))
  out = current.copy()
  for label in range(max(current) + 1):
    if label in renamed:
      out[current == label] = renamed[label]
  return out


class MultiStageClusterer:
  """reference multi_stage_clusterer.py:66-180"""

  def __init__(self,
               main_clusterer: spectral_clusterer.SpectralClusterer,
               fallback_threshold: float = 0.5,
               L: int = 50,
               U1: int = 100,
               U2: int = 600,
               deflicker: Deflicker = Deflicker.NoDeflicker):
    self.deflicker = deflicker
    self.main = main_clusterer
    if self.main.max_spectral_size:
      raise ValueError(
          "Do not set max_spectral_size for SpectralClusterer when"
          "using MultiStageClusterer.")
    options = self.main.fallback_options
    options.spectral_min_embeddings = L            # lower bound of the main clusterer
    self.U1 = U1                                   # upper bound of the main clusterer
    self.U2 = U2                                   # upper bound of the pre-clusterer
    options.agglomerative_threshold = fallback_threshold
    options.single_cluster_condition = (
        fallback_clusterer.SingleClusterCondition.FallbackClusterer)
    options.fallback_clusterer_type = (
        fallback_clusterer.FallbackClustererType.Agglomerative)
    self.cache = None                  # all cached embeddings / centroids
    self.num_embeddings = 0
    self.compression_labels = None     # original embedding -> compressed centroid
    self.previous_output = None

  def _pre_cluster(self, rows: np.ndarray) -> np.ndarray:
    """AgglomerativeClustering(n_clusters=U1, metric="cosine", linkage="complete")."""
    return utils.cosine_agglomerative_clustering(rows, n_clusters=self.U1,
                                                 linkage="complete")

  def streaming_predict(self, embedding: np.ndarray) -> np.ndarray:
    """Label the next embedding and re-label all earlier ones (reference :128-180)."""
    self.num_embeddings += 1
    if self.num_embeddings == 1:
      self.cache = embedding
      labels = np.array([0])
      self.previous_output = labels
      return labels
    self.cache = np.vstack([self.cache, embedding])

    if self.num_embeddings <= self.U1:             # fallback or main clusterer only
      labels = self.main.predict(self.cache)
      self.previous_output = labels
      return labels

    pre_labels = self._pre_cluster(self.cache)
    pre_centroids = utils.get_cluster_centroids(self.cache, pre_labels)
    main_labels = self.main.predict(pre_centroids)
    compress = self.cache.shape[0] == self.U2      # dynamic compression
    if compress:
      self.cache = pre_centroids
    return finish_stream_step(self, self.deflicker, pre_labels, main_labels, compress)


def finish_stream_step(state, deflicker: Deflicker, pre_labels: np.ndarray,
                       main_labels: np.ndarray, compress: bool) -> np.ndarray:
  """The host bookkeeping of one step beyond U1, after its two clustering calls (reference
  :150-180): the labels of every embedding of the stream from the pre-cluster labels of the
  cache and the main labels of its centroids, chained through `state.compression_labels`
  (original embedding -> cache row); that map extended by the new row and, when the cache is
  being replaced by its centroids (`compress`), rewritten to point at them; the de-flickering
  against `state.previous_output`.  `state`: a MultiStageClusterer or a session of a
  MultiStageStreamPool -- both streams go through this one function."""
  if state.compression_labels is not None:
    state.compression_labels = np.append(state.compression_labels,
                                         max(state.compression_labels) + 1)
  labels = utils.chain_labels(state.compression_labels,
                              utils.chain_labels(pre_labels, main_labels))
  if compress:
    state.compression_labels = utils.chain_labels(state.compression_labels, pre_labels)
  if deflicker == Deflicker.OrderBased:
    labels = utils.enforce_ordered_labels(labels)
  elif deflicker == Deflicker.Hungarian and state.previous_output is not None:
    labels = match_labels(labels, state.previous_output)
  state.previous_output = labels
  return labels


class _PoolSession:
  """Host state of one session of a MultiStageStreamPool (the cache itself is on the device)."""

  def __init__(self):
    self.num_embeddings = 0
    # host copy of the cache while it has at most U1 rows (none with pool_early_stage)
    self.mirror = None
    self.compression_labels = None
    self.previous_output = None


(ROUTE_MAIN_ONLY, ROUTE_POOLED_GROUPED, ROUTE_POOLED_SINGLE, ROUTE_EARLY_FALLBACK,
 ROUTE_EARLY_MAIN) = range(5)


class MultiStageStreamPool:
  """Up to `capacity` independent MultiStageClusterer streams advanced together.

  The caches live on the device (`sc_pool_*`).  One `streaming_predict(sessions, embeddings)`
  call appends one embedding to each listed session and returns, per session, exactly what
  that session's own `MultiStageClusterer.streaming_predict` would have returned.  Sessions
  beyond U1 rows share their launches: one append, one distance pass, one nearest-neighbour-
  chain launch with a workgroup per session, one centroid launch, and -- when the main
  clusterer is one the library batch covers -- one grouped call over the resident centroid
  buffers.  Constructor arguments as MultiStageClusterer's, plus `capacity` and `device`
  (default: the main clusterer's).  The embedding width is fixed by the first rows a pool sees.

  `pool_early_stage` (keyword only, default False): sessions of at most U1 rows share their
  launches too, when the main clusterer is one the library batch covers.  Fewer than L rows: one
  `sc_pool_fallback` call per step, the average-linkage fallback of all such sessions on their
  resident caches.  L to U1 rows: the cache itself (`sc_pool_cache`) joins the step's one
  grouped main call next to the centroid buffers of the sessions beyond U1.  No host copy of a
  cache is kept then and no embedding is downloaded.  Without the flag, or with a main clusterer
  outside the library batch, each such session runs `main.predict` on a host mirror of its
  cache, one after the other.

  `pool_fallback_condition` (keyword only, default False): a `min_clusters=1` main clusterer that
  carries the single-cluster condition this constructor sets (FallbackClusterer, agglomerative)
  counts as one the library batch covers.  The step's grouped main call is then ONE
  `sc_predict_batch_single_fallback` call: the verdicts of all its centroid buffers (and, with
  `pool_early_stage`, of the caches of L .. U1 rows) on the device, then the grouped batch of
  those that hold several clusters.  Without the flag such a pool runs `main.predict` per
  session (routes 0 and 2), as before.
  """

  def __init__(self,
               main_clusterer: spectral_clusterer.SpectralClusterer,
               fallback_threshold: float = 0.5,
               L: int = 50,
               U1: int = 100,
               U2: int = 600,
               deflicker: Deflicker = Deflicker.NoDeflicker,
               capacity: int = 64,
               device: typing.Optional[int] = None,
               d: typing.Optional[int] = None,
               *,
               pool_early_stage: bool = False,
               pool_fallback_condition: bool = False):
    # (the option changes and the max_spectral_size check of the per-stream class)
    MultiStageClusterer(main_clusterer, fallback_threshold, L, U1, U2, deflicker)
    self.main = main_clusterer
    self.deflicker = deflicker
    self.L, self.U1, self.U2 = int(L), int(U1), int(U2)
    self.capacity = int(capacity)
    self.pool_early_stage = bool(pool_early_stage)
    self.pool_fallback_condition = bool(pool_fallback_condition)
    self.device = device if device is not None else main_clusterer.device
    self.d = None
    self._pool = None
    self._sessions = {}                # id -> _PoolSession
    self.last_routes = []
    # All device memory is taken up front.  With `d` that is now; without it the slabs are
    # taken when the first rows show their width, and the constructor only takes (and gives
    # back) those of d = 1 -- the distance matrices, which do not depend on d, are most of
    # them -- so a capacity that cannot fit raises its MemoryError here, not mid-stream.
    with _lib.use_device(self.device):
      self._ensure_pool(1 if d is None else int(d))
    if d is None:
      self._free()
      self.d = None

  # ---------------------------------------------------------------- plumbing
  def _handle(self) -> _lib.Handle:
    return _lib.default_handle(self.device)

  def _ensure_pool(self, d: int) -> None:
    if self._pool is not None:
      if d != self.d:
        raise ValueError("embeddings have %d features, the pool holds %d" % (d, self.d))
      return
    handle = self._handle()
    pool = ctypes.c_void_p()
    handle.check(handle.lib.sc_pool_create(handle.raw, self.capacity, int(d), self.U1, self.U2,
                                           ctypes.byref(pool)))
    self._pool, self._pool_handle, self.d = pool, handle, int(d)

  def _free(self):
    pool, self._pool = getattr(self, "_pool", None), None
    if pool is not None and getattr(self._pool_handle, "raw", None):
      self._pool_handle.lib.sc_pool_destroy(pool)

  def __del__(self):
    try:
      self._free()
    except Exception:  # interpreter shutdown
      pass

  def _session(self, session) -> _PoolSession:
    state = self._sessions.get(session) if isinstance(session, (int, np.integer)) else None
    if state is None:
      raise ValueError("session %r is not open" % (session,))
    return state

  def _append(self, sessions, counts, source) -> None:
    handle, n = self._pool_handle, len(sessions)
    handle.check(handle.lib.sc_pool_append(
        self._pool, (ctypes.c_int32 * n)(*[int(s) for s in sessions]),
        (ctypes.c_int32 * n)(*counts), n, ctypes.byref(source.array)))

  # ---------------------------------------------------------------- sessions
  def open(self) -> int:
    for slot in range(self.capacity):
      if slot not in self._sessions:
        self._sessions[slot] = _PoolSession()
        if self._pool is not None:
          self._pool_handle.check(self._pool_handle.lib.sc_pool_reset(self._pool, slot))
        return slot
    raise RuntimeError("all %d sessions of the pool are open" % self.capacity)

  def close(self, session) -> None:
    self._session(session)
    del self._sessions[int(session)]

  def reset(self, session) -> None:
    self._session(session)
    self._sessions[int(session)] = _PoolSession()
    if self._pool is not None:
      self._pool_handle.check(self._pool_handle.lib.sc_pool_reset(self._pool, int(session)))

  def load(self, session, rows) -> None:
    """Append `rows` (anything streaming_predict takes, (k, d)) to the session's cache without
    clustering them: resumes a stream.  Only while the cache stays within U2 rows and has not
    been compressed yet (ValueError otherwise); the next step has no previous output to
    de-flicker against."""
    state = self._session(session)
    with _lib.use_device(self.device):
      with _dlpack.describe(rows, self._handle) as source:
        k, d = source.shape
        if state.compression_labels is not None or state.num_embeddings + k > self.U2:
          raise ValueError("load() needs an uncompressed cache that stays within U2 = %d rows"
                           % self.U2)
        self._ensure_pool(d)
        self._append([session], [k], source)
        total = state.num_embeddings + k
        mirrored = 0 if state.mirror is None else state.mirror.shape[0]
        if total <= self.U1 and mirrored == state.num_embeddings and not self._early_pooled():
          host = np.asarray(source.host_f64(self._pool_handle), dtype=np.float64)
          state.mirror = host.copy() if state.mirror is None else np.vstack([state.mirror, host])
        else:   # (a step that needs the mirror after all fetches the cache: _step)
          state.mirror = None
        state.num_embeddings = total
        state.previous_output = None

  # -------------------------------------------------------------------- step
  def streaming_predict(self, sessions: typing.Sequence[int],
                        embeddings) -> typing.List[np.ndarray]:
    """One step of every listed session (distinct ids): row i of `embeddings`
    ((len(sessions), d); NumPy or DLPack, float64 / float32 / float16 / bfloat16, host or
    device) is the next embedding of sessions[i].  Element i of the result is what that
    stream's MultiStageClusterer.streaming_predict would return, values and dtype.
    `last_routes`: per session, 0 main.predict on its own (at most U1 rows; with
    `pool_early_stage` only a session's first row, which runs nothing), 1 pooled pre-cluster +
    the grouped main call, 2 pooled pre-cluster + a main.predict of its own, and with
    `pool_early_stage` 3 the pooled fallback (2 .. L - 1 rows), 4 the cache in the grouped main
    call (L .. U1 rows)."""
    sessions = [int(s) if isinstance(s, (int, np.integer)) else s for s in sessions]
    states = [self._session(s) for s in sessions]
    if len(set(sessions)) != len(sessions):
      raise ValueError("a session is listed twice")
    if not sessions:
      self.last_routes = []
      return []
    with _lib.use_device(self.device):
      with _dlpack.describe(embeddings, self._handle) as source:
        if source.shape[0] != len(sessions):
          raise ValueError("embeddings must be (len(sessions), d)")
        self._ensure_pool(source.shape[1])
        self._append(sessions, [1] * len(sessions), source)
        early = self._early_pooled()
        host = None
        if not early and any(st.num_embeddings < self.U1 for st in states):
          host = np.asarray(source.host_f64(self._pool_handle), dtype=np.float64)
      return self._step(sessions, states, host, early)

  def _mirror_row(self, session, st, row) -> None:
    """The host mirror of a cache of at most U1 rows after its append: the mirror plus the new
    row, or -- when the mirror is missing or behind, after steps or a load() that kept none --
    the cache as the device holds it."""
    mirrored = 0 if st.mirror is None else st.mirror.shape[0]
    if mirrored == st.num_embeddings - 1:
      st.mirror = row.copy() if st.mirror is None else np.vstack([st.mirror, row])
    else:
      st.mirror = np.empty((st.num_embeddings, self.d), dtype=np.float64)
      self._pool_handle.check(self._pool_handle.lib.sc_pool_get(
          self._pool, session, _lib.SC_POOL_CACHE, _lib.as_double_p(st.mirror)))

  def _step(self, sessions, states, host, early) -> typing.List[np.ndarray]:
    handle = self._pool_handle
    out = [None] * len(sessions)
    routes = [ROUTE_MAIN_ONLY] * len(sessions)
    pooled, early_fallback, early_main = [], [], []
    for i, st in enumerate(states):
      st.num_embeddings += 1
      if st.num_embeddings > self.U1:
        st.mirror = None
        pooled.append(i)
      elif early:                                 # the cache stays where it is
        st.mirror = None
        if st.num_embeddings == 1:
          out[i] = np.array([0])
          st.previous_output = out[i]
        elif st.num_embeddings < self.L:
          early_fallback.append(i)
        else:
          early_main.append(i)
      else:
        self._mirror_row(sessions[i], st, host[i:i + 1])
        if st.num_embeddings == 1:
          out[i] = np.array([0])
        else:
          out[i] = self.main.predict(st.mirror)   # fallback or main clusterer only
        st.previous_output = out[i]
    if early_fallback:                            # main.predict below L rows, for all of them
      count = len(early_fallback)
      labels = [np.empty(states[i].num_embeddings, dtype=np.int64) for i in early_fallback]
      handle.check(handle.lib.sc_pool_fallback(
          self._pool, (ctypes.c_int32 * count)(*[sessions[i] for i in early_fallback]), count,
          float(self.main.fallback_options.agglomerative_threshold),
          (ctypes.POINTER(ctypes.c_int64) * count)(*[_lib.as_int64_p(l) for l in labels])))
      for i, fallback_labels in zip(early_fallback, labels):
        out[i] = fallback_labels
        states[i].previous_output = out[i]
        routes[i] = ROUTE_EARLY_FALLBACK
    if pooled or early_main:
      count = len(pooled)
      pre = [np.empty(handle.lib.sc_pool_rows(self._pool, sessions[i]), dtype=np.int64)
             for i in pooled]
      if pooled:
        slots = (ctypes.c_int32 * count)(*[sessions[i] for i in pooled])
        handle.check(handle.lib.sc_pool_precluster(
            self._pool, slots, count,
            (ctypes.POINTER(ctypes.c_int64) * count)(*[_lib.as_int64_p(l) for l in pre])))
      if early or self._main_is_batchable():
        # one grouped call per step: the caches of L .. U1 rows and the centroids beyond U1
        arrays = []
        for i in early_main:
          arrays.append(_lib.ScArray())
          handle.check(handle.lib.sc_pool_cache(self._pool, sessions[i],
                                                ctypes.byref(arrays[-1])))
        for i in pooled:
          arrays.append(_lib.ScArray())
          handle.check(handle.lib.sc_pool_centroids(self._pool, sessions[i],
                                                    ctypes.byref(arrays[-1])))
        if getattr(self, "pool_fallback_condition", False):
          main = self.main.predict_device_batch(arrays, batch_fallback_condition=True)
        else:
          main = self.main.predict_device_batch(arrays)
        for i, main_labels in zip(early_main, main):
          out[i] = main_labels
          states[i].previous_output = out[i]
          routes[i] = ROUTE_EARLY_MAIN
        main = main[len(early_main):]
        route = ROUTE_POOLED_GROUPED
      else:
        main = []
        for i in pooled:
          centroids = np.empty((self.U1, self.d), dtype=np.float64)
          handle.check(handle.lib.sc_pool_get(self._pool, sessions[i], _lib.SC_POOL_CENTROIDS,
                                              _lib.as_double_p(centroids)))
          main.append(self.main.predict(centroids))
        route = ROUTE_POOLED_SINGLE
      for i, pre_labels, main_labels in zip(pooled, pre, main):
        compress = pre_labels.shape[0] == self.U2   # dynamic compression, on the device
        if compress:
          handle.check(handle.lib.sc_pool_compress(self._pool, sessions[i]))
        out[i] = finish_stream_step(states[i], self.deflicker, pre_labels, main_labels, compress)
        routes[i] = route
    self.last_routes = routes
    return out

  def _early_pooled(self) -> bool:
    """Do sessions of at most U1 rows take the pooled routes 3 and 4?  (The fallback of the
    per-stream class is the agglomerative one: its constructor sets it on the main clusterer.)"""
    return (self.pool_early_stage and self._main_is_batchable() and
            self.main.fallback_options.fallback_clusterer_type ==
            fallback_clusterer.FallbackClustererType.Agglomerative)

  def _main_is_batchable(self) -> bool:
    """predict_batch's conditions; spectral_min_embeddings (= L) is met by the U1 centroids, and
    a min_clusters = 1 main clusterer is covered when its single-cluster test reads the affinity
    (predict_device_batch then carries the test inside the grouped call).  With
    `pool_fallback_condition` the FallbackClusterer condition is covered as well (it checks the
    metric itself)."""
    if (getattr(self, "pool_fallback_condition", False) and
        self.main._fallback_condition_covers(min_embeddings_met=self.L <= self.U1)):
      return True
    if not self.main._library_batch_covers(min_embeddings_met=self.L <= self.U1,
                                           single_check_covered=True):
      return False
    try:
      _lib.kmeans_metric_code(self.main.custom_dist)
    except (ValueError, NotImplementedError):
      return False   # main.predict raises what it raises today
    return True
