"""Utility functions (mirror of reference `spectralcluster/utils.py`)."""

from __future__ import annotations

import contextlib
import ctypes
import enum
import typing

import numpy as np

from spectralcluster_amd import _lib

EPS = 1e-10


class EigenGapType(enum.Enum):
  """Ratio of, or max-normalised difference between, consecutive eigenvalues
  (reference utils.py:10-17)."""
  Ratio = 1
  NormalizedDiff = 2


def _stage_on_arrays(inputs, out_specs, call):
  """A building block on described arrays: `inputs` are read where they are (`_dlpack.describe`'s
  sources), every `(out, shape, what)` of `out_specs` is written where it is -- or, for an `out`
  of None, into a new host float64 array -- and `call(handle, sources, outs)` makes the library
  call.  Returns the list of results (each `out` object itself, or the new array)."""
  from spectralcluster_amd import _dlpack  # (it imports this module's siblings)
  handle = _lib.default_handle()
  with contextlib.ExitStack() as held:
    sources = [held.enter_context(_dlpack.describe_input(x, lambda: handle)) for x in inputs]
    results, outs = [], []
    for out, shape, what in out_specs:
      shape = shape(sources) if callable(shape) else shape
      if out is None:
        out = np.empty(shape, dtype=np.float64)
      results.append(out)
      outs.append(held.enter_context(_dlpack.describe_out(out, lambda: handle, shape, what)))
    call(handle, sources, outs)
  return results


def compute_affinity_matrix(embeddings, out=None):
  """(cos(x_i, x_j) + 1) / 2 on the fp64 MFMA GEMM (reference utils.py:20-41).

  `embeddings` is whatever predict() takes: a NumPy array, or an object with `__dlpack__` in host
  memory or on the GPU, float64 / float32 / float16 / bfloat16, any non-negative strides; a device
  tensor is read in place.  `out`, when given, receives the (n, n) result and is returned: a
  writeable ndarray (float64 / float32 / float16) or a DLPack object (also bfloat16), host or
  device, of exactly that shape, with non-negative strides under which no two indices share an
  address.  The result is the float64 one rounded to nearest even into float32 and from there
  into float16 / bfloat16.  `out` may be `embeddings`, a view of it or overlap it: the input is
  completely inside the library's buffers before the first byte of `out` is written.  Without
  `out` the result is a new host float64 array."""
  from spectralcluster_amd import _dlpack  # (it imports this module's siblings)
  if out is not None or _dlpack.is_described(embeddings):
    def call(handle, sources, outs):
      handle.check(handle.lib.sc_stage_affinity_array(
          handle.raw, ctypes.byref(sources[0].array), ctypes.byref(outs[0].array)))
    return _stage_on_arrays([embeddings], [(out, lambda s: (s[0].shape[0],) * 2, "out")], call)[0]
  x = np.ascontiguousarray(embeddings, dtype=np.float64)
  if x.ndim != 2:
    raise ValueError("embeddings must be 2-dimensional")
  n = x.shape[0]
  out = np.empty((n, n), dtype=np.float64)
  handle = _lib.default_handle()
  handle.check(handle.lib.sc_stage_affinity(
      handle.raw, _lib.as_double_p(x), n, x.shape[1], _lib.as_double_p(out)))
  return out


def compute_sorted_eigenvectors(
    input_matrix, descend: bool = True,
    count: typing.Optional[int] = None, out=None) -> typing.Tuple:
  """Sorted eigenpairs (reference utils.py:44-71): `np.linalg.eig`, real parts,
  argsort by eigenvalue.

  A symmetric input runs on the symmetric solver (dense Jacobi for n <= 128 -- every
  eigenpair, as the reference returns -- else block Lanczos for the `count` (default
  extreme ones; more than 64 come from the dense tridiagonal path).  Anything else runs on
  the general solver (Hessenberg + complex QR for n <= 64, else block Arnoldi for `count` <= 64
  extreme ones, default 32; more than 64 -- up to all n -- take the dense Hessenberg route:
  reduction on the device, QR iteration + inverse iteration on the host); eigenvectors of
  complex pairs carry LAPACK's normalisation before `.real`.

  `input_matrix` and `out` are what `compute_affinity_matrix` takes; `out` is a pair (values,
  vectors) of shapes (count,) and (n, count), and the pair is returned.  With `out` given and
  `count` None, `count = out[0].shape[0]`; given both, they must agree.  For an input that is read
  where it is (a DLPack object, or any input when `out` is given) the symmetric / general decision
  is made on the device, by the rule above on the widened float64 values -- a matrix with a NaN is
  not symmetric -- from three numbers: the matrix is not downloaded.  `out` may overlap the input.
  """
  from spectralcluster_amd import _dlpack  # (it imports this module's siblings)
  if out is not None or _dlpack.is_described(input_matrix):
    return _sorted_eigenvectors_on_arrays(input_matrix, descend, count, out)
  m = np.ascontiguousarray(input_matrix, dtype=np.float64)
  if m.ndim != 2 or m.shape[0] != m.shape[1]:
    raise ValueError("input_matrix must be square")
  n = m.shape[0]
  scale = float(np.max(np.abs(m))) if m.size else 0.0
  symmetric = np.allclose(m, m.T, rtol=0.0, atol=1e-12 * max(scale, 1e-300))
  if count is None:
    if symmetric:
      count = n if n <= 128 else 64
    else:
      count = n if n <= 64 else 32
  values = np.empty(count, dtype=np.float64)
  vectors = np.empty((n, count), dtype=np.float64)
  handle = _lib.default_handle()
  entry = handle.lib.sc_stage_sym_eig if symmetric else handle.lib.sc_stage_eig
  handle.check(entry(
      handle.raw, _lib.as_double_p(m), n, count, int(bool(descend)),
      _lib.as_double_p(values), _lib.as_double_p(vectors), None))
  return values, vectors


def _sorted_eigenvectors_on_arrays(input_matrix, descend, count, out):
  """compute_sorted_eigenvectors through `sc_stage_eig_array`."""
  from spectralcluster_amd import _dlpack  # (it imports this module's siblings)
  if out is not None:
    if not isinstance(out, (tuple, list)) or len(out) != 2:
      raise TypeError("out must be a pair (values, vectors)")
    shape = getattr(out[0], "shape", None)
    if shape is None or len(shape) != 1:
      raise ValueError("out values must be 1-dimensional, (count,)")
    if count is None:
      count = int(shape[0])
    elif int(count) != int(shape[0]):
      raise ValueError("out values hold %d entries, count is %d" % (int(shape[0]), int(count)))
  if not hasattr(input_matrix, "shape"):
    input_matrix = np.asarray(input_matrix)
  shape = input_matrix.shape
  if len(shape) != 2 or shape[0] != shape[1]:
    raise ValueError("input_matrix must be square")
  n = int(shape[0])
  symmetric = ctypes.c_int(0)
  # count None (only without `out`): the default count follows the decision, which the library
  # makes -- it is given room for the larger default and says which one it took
  room = (n if n <= 128 else 64) if count is None else int(count)
  request = -1 if count is None else room
  values, vectors = out if out is not None else (None, None)

  def call(handle, sources, outs):
    handle.check(handle.lib.sc_stage_eig_array(
        handle.raw, ctypes.byref(sources[0].array), request, int(bool(descend)),
        ctypes.byref(outs[0].array), ctypes.byref(outs[1].array), ctypes.byref(symmetric)))
  values, vectors = _stage_on_arrays(
      [input_matrix], [(values, (room,), "out values"), (vectors, (n, room), "out vectors")],
      call)
  if count is None and not symmetric.value:
    count = n if n <= 64 else 32
    values, vectors = values[:count].copy(), np.ascontiguousarray(vectors[:, :count])
  return values, vectors


def compute_number_of_clusters(eigenvalues: np.ndarray,
                               max_clusters: typing.Optional[int] = None,
                               stop_eigenvalue: float = 1e-2,
                               eigengap_type: EigenGapType = EigenGapType.Ratio,
                               descend: bool = True,
                               eps: float = EPS) -> typing.Tuple[int, float]:
  """Maximum-eigengap cluster count (reference utils.py:74-130); the scalar loop
  runs in the native library (`sc_eigengap`)."""
  if not isinstance(eigengap_type, EigenGapType):
    raise TypeError("eigengap_type must be a EigenGapType")
  if eps != EPS:
    raise _lib.UnsupportedOnDeviceError("eps is fixed at 1e-10 in the native library")
  w = np.ascontiguousarray(eigenvalues, dtype=np.float64)
  k = ctypes.c_int(0)
  delta = ctypes.c_double(0.0)
  rc = _lib.load().sc_eigengap(_lib.as_double_p(w), w.size, int(max_clusters or 0),
                               float(stop_eigenvalue), eigengap_type.value,
                               int(bool(descend)), ctypes.byref(k),
                               ctypes.byref(delta))
  if rc != _lib.SC_OK:
    raise ValueError("Unsupported eigengap_type")
  return k.value, delta.value


def enforce_ordered_labels(labels: np.ndarray) -> np.ndarray:
  """Relabel so that labels appear in increasing order of first occurrence
  (reference utils.py:133-156)."""
  out = np.empty_like(labels)
  order = {}
  for pos, value in enumerate(labels.tolist()):
    out[pos] = order.setdefault(value, len(order))
  return out


def get_cluster_centroids(embeddings, labels, out=None):
  """Mean embedding of every cluster, (max(labels) + 1, n_features) (reference
  utils.py:159-176); the segmented mean runs on the device and adds the members in index
  order, as `np.mean(axis=0)` does.

  `embeddings` is whatever predict() takes and `labels` a 1-D array of n entries, each a NumPy
  array or an object with `__dlpack__` in host memory or on the GPU (labels: int64 / int32, or
  float64 / float32 holding integral values, any non-negative stride); device tensors are read
  where they are.  `out`, when given, is a (rows >= k, n_features) array as
  `compute_affinity_matrix` takes it: rows 0 .. k - 1 are written, nothing else, and `out[:k]` is
  returned -- a caller who knows `max_clusters` preallocates and never waits to learn k.  `out`
  in device memory must not overlap a device `embeddings` or `labels`.  The values are, bit for
  bit, `np.mean(x64[labels == c], axis=0)` narrowed to `out`'s dtype: a label in range(k) that no
  row carries gives a row of NaN, rows with a negative label belong to no cluster.  Without `out`
  the result is a new host float64 array (for labels on the device that takes a second library
  call, which returns k first).  NumPy `embeddings` and `labels` (or lists) with `out=None` run
  `sc_cluster_centroids`, as they always have."""
  from spectralcluster_amd import _dlpack  # (it imports this module's siblings)
  if out is not None or _dlpack.is_described(embeddings) or _dlpack.is_described(labels):
    return get_cluster_centroids_batch([embeddings], [labels],
                                       None if out is None else [out])[0]
  x = np.ascontiguousarray(embeddings, dtype=np.float64)
  lab = np.ascontiguousarray(labels, dtype=np.int64)
  if x.ndim != 2 or lab.shape != (x.shape[0],):
    raise ValueError("embeddings must be (n_samples, n_features), labels (n_samples,)")
  k = int(lab.max()) + 1
  out = np.empty((k, x.shape[1]), dtype=np.float64)
  handle = _lib.default_handle()
  handle.check(handle.lib.sc_cluster_centroids(
      handle.raw, _lib.as_double_p(x), x.shape[0], x.shape[1], _lib.as_int64_p(lab), k,
      _lib.as_double_p(out)))
  return out


def get_cluster_centroids_batch(embeddings_list: typing.Sequence, labels_list: typing.Sequence,
                                out: typing.Optional[typing.Sequence] = None) -> typing.List:
  """`get_cluster_centroids(e, l, out=o)` for every member of the lists in ONE
  `sc_cluster_centroids_arrays` call: members of any n, dtype and location may be mixed, all with
  the same number of columns (as `cosine_agglomerative_clustering_batch`).  `out` is None or a
  list of the same length; returns the list of `out[i][:k_i]` (new host float64 arrays without
  `out`).  The library walks all labels once (validation and every k_i), sorts each member's rows
  by cluster on the device and takes the means from each cluster's own rows: a fixed number of
  launches and two synchronisations for the whole list.  Every argument is checked before
  anything is launched; an error names the member's index and leaves every `out` untouched."""
  from spectralcluster_amd import _dlpack  # (it imports this module's siblings)
  count = len(embeddings_list)
  if len(labels_list) != count:
    raise ValueError("labels_list must be as long as embeddings_list")
  if out is not None and len(out) != count:
    raise ValueError("out must be as long as embeddings_list")
  if count == 0:
    return []
  handle = _lib.default_handle()
  with contextlib.ExitStack() as held:
    xs = [held.enter_context(_dlpack.describe_input(e, lambda: handle)) for e in embeddings_list]
    d = xs[0].shape[1]
    for i, x in enumerate(xs):
      if x.shape[1] != d:
        raise ValueError("member %d: all embeddings must be (n_i, d) with the same d" % i)
    labs = []
    for i, (x, l) in enumerate(zip(xs, labels_list)):
      labs.append(held.enter_context(
          _dlpack.describe_labels(l, lambda: handle, x.shape[0], "labels of member %d" % i)))
    # k where the host can tell: a host label array has been checked and is read here
    ks = [None if l.numpy is None else (int(l.numpy.max()) + 1 if l.numpy.size else 0)
          for l in labs]
    ks = [None if k is None else max(k, 0) for k in ks]
    x_arr = (_lib.ScArray * count)(*[x.array for x in xs])
    l_arr = (_lib.ScArray * count)(*[l.array for l in labs])
    k_arr = (ctypes.c_int32 * count)()
    if out is None:
      if any(k is None for k in ks):  # labels on the device: the library says how many clusters
        handle.check(handle.lib.sc_cluster_centroids_arrays(handle.raw, x_arr, l_arr, count, None,
                                                            k_arr))
        ks = [int(k) for k in k_arr]
      results = [np.empty((k, d), dtype=np.float64) for k in ks]
    else:
      results = list(out)
    outs = []
    for i, (o, k) in enumerate(zip(results, ks)):
      what = "out of member %d" % i
      shape = tuple(int(e) for e in np.shape(o))
      if len(shape) != 2 or shape[1] != d:
        raise ValueError("%s must be (rows >= k, %d), not %s" % (what, d, shape))
      if k is not None and shape[0] < k:
        raise ValueError("%s has %d rows, the labels make %d clusters" % (what, shape[0], k))
      if shape[0] == 0:  # room for no cluster (every label negative): nothing is written
        outs.append(_dlpack.Source(_lib.ScArray(None, _lib.SC_DTYPE_F64, _lib.SC_MEM_HOST, 0, d,
                                                d, 1), o))
      else:
        outs.append(held.enter_context(_dlpack.describe_out(o, lambda: handle, shape, what)))
    clash = _dlpack.device_overlap(outs, xs + labs)
    if clash is not None:
      raise ValueError("out of member %d overlaps embeddings or labels of the call in device "
                       "memory: they are read in place" % clash)
    o_arr = (_lib.ScArray * count)(*[o.array for o in outs])
    handle.check(handle.lib.sc_cluster_centroids_arrays(handle.raw, x_arr, l_arr, count, o_arr,
                                                        k_arr))
  return [o[:int(k)] for o, k in zip(results, k_arr)]


def chain_labels(pre_labels: typing.Optional[np.ndarray],
                 main_labels: np.ndarray) -> np.ndarray:
  """Labels of the samples given the labels of their pre-clusters (reference
  utils.py:179-206).  Like the reference the result is float64 (it fills `np.zeros`)."""
  if pre_labels is None:
    return main_labels
  count = int(max(pre_labels) + 1)
  if count != main_labels.shape[0]:
    raise ValueError("pre_labels has {} values while main_labels has {} rows.".format(
        count, main_labels.shape[0]))
  return np.asarray(main_labels, dtype=np.float64)[np.asarray(pre_labels, dtype=np.int64)]


LINKAGE_CODES = {"complete": 1, "average": 2}


def cosine_agglomerative_clustering(embeddings: np.ndarray,
                                    n_clusters: typing.Optional[int] = None,
                                    linkage: str = "complete",
                                    distance_threshold: typing.Optional[float] = None
                                    ) -> np.ndarray:
  """`sklearn.cluster.AgglomerativeClustering(n_clusters=..., metric="cosine",
  linkage=..., distance_threshold=...).fit_predict(embeddings)` on the device -- the
  pre-clusterer of the reference (spectral_clusterer.py:170-199,
  multi_stage_clusterer.py:109-112) and its agglomerative fallback
  (fallback_clusterer.py:108-113).  Labels are numbered exactly as sklearn numbers them
  (its heap-ordered tree cut); the downstream GaussianBlur depends on that order."""
  if linkage not in LINKAGE_CODES:
    raise _lib.UnsupportedOnDeviceError("linkage must be 'complete' or 'average'")
  if (n_clusters is None) == (distance_threshold is None):
    raise ValueError("Exactly one of n_clusters and distance_threshold has to be set, "
                     "and the other needs to be None.")
  x = np.ascontiguousarray(embeddings, dtype=np.float64)
  if x.ndim != 2:
    raise ValueError("embeddings must be 2-dimensional")
  labels = np.empty(x.shape[0], dtype=np.int64)
  found = ctypes.c_int(0)
  handle = _lib.default_handle()
  handle.check(handle.lib.sc_ahc(
      handle.raw, _lib.as_double_p(x), x.shape[0], x.shape[1], LINKAGE_CODES[linkage],
      int(n_clusters or 0), float(distance_threshold or 0.0), _lib.as_int64_p(labels),
      ctypes.byref(found)))
  return labels


def cosine_agglomerative_clustering_batch(embeddings_list: typing.Sequence,
                                          n_clusters: typing.Optional[int] = None,
                                          linkage: str = "complete",
                                          distance_threshold: typing.Optional[float] = None,
                                          return_centroids: bool = False):
  """`cosine_agglomerative_clustering` of every entry of `embeddings_list` (each anything
  predict() takes: NumPy arrays and DLPack objects, float64 / float32 / float16 / bfloat16, host
  or device memory, mixed freely; all with the same number of columns) in ONE `sc_batch_ahc`
  call: entries of any size share the launches, a workgroup per entry in the chain.  Returns the
  list of label arrays; with `return_centroids` also the list of `get_cluster_centroids` of each
  entry (bit for bit).  An entry with a zero or non-finite row raises a ValueError that names its
  index."""
  from spectralcluster_amd import _dlpack  # (it imports this module's siblings)
  if linkage not in LINKAGE_CODES:
    raise _lib.UnsupportedOnDeviceError("linkage must be 'complete' or 'average'")
  if (n_clusters is None) == (distance_threshold is None):
    raise ValueError("Exactly one of n_clusters and distance_threshold has to be set, "
                     "and the other needs to be None.")
  for e in embeddings_list:
    if isinstance(e, np.ndarray) and e.ndim != 2:
      raise ValueError("embeddings must be 2-dimensional")
  count = len(embeddings_list)
  if count == 0:
    return ([], []) if return_centroids else []
  handle = _lib.default_handle()
  with contextlib.ExitStack() as held:
    sources = [held.enter_context(_dlpack.describe(e, lambda: handle)) for e in embeddings_list]
    d = sources[0].shape[1]
    if any(src.shape[1] != d for src in sources):
      raise ValueError("all utterances must be (n_i, d) with the same d")
    labels = [np.empty(src.shape[0], dtype=np.int64) for src in sources]
    lp = (ctypes.POINTER(ctypes.c_int64) * count)(*[_lib.as_int64_p(l) for l in labels])
    centroids, cp = None, None
    if return_centroids:
      centroids = [np.empty((min(int(n_clusters), src.shape[0]) if n_clusters else src.shape[0], d),
                            dtype=np.float64) for src in sources]
      cp = (ctypes.POINTER(ctypes.c_double) * count)(*[_lib.as_double_p(c) for c in centroids])
    handle.check(handle.lib.sc_batch_ahc(
        handle.raw, (_lib.ScArray * count)(*[src.array for src in sources]), count,
        LINKAGE_CODES[linkage], int(n_clusters or 0), float(distance_threshold or 0.0), lp, cp))
  if not return_centroids:
    return labels
  return labels, [c[:int(l.max()) + 1] for c, l in zip(centroids, labels)]


def cosine_single_cluster_check_batch(embeddings_list: typing.Sequence,
                                      distance_threshold: float):
  """Does `cosine_agglomerative_clustering(e, linkage="average", distance_threshold=...)` leave
  ONE cluster? -- for every entry of `embeddings_list` (what `cosine_agglomerative_clustering_batch`
  takes) in one `sc_batch_fallback_check` call: the FallbackClusterer single-cluster condition
  with the agglomerative fallback (`fallback_clusterer.check_single_cluster`), decided on the
  device without a merge list.  Returns (single, heights): a bool array, and per entry the merge
  height that decided it -- the largest of the tree for an entry of one cluster, otherwise the
  first one found at or above the threshold.  An entry with a zero or non-finite row raises a
  ValueError that names its index; neither output exists then."""
  from spectralcluster_amd import _dlpack  # (it imports this module's siblings)
  for e in embeddings_list:
    if isinstance(e, np.ndarray) and e.ndim != 2:
      raise ValueError("embeddings must be 2-dimensional")
  count = len(embeddings_list)
  heights = np.full(count, np.nan, dtype=np.float64)
  single = np.full(count, -1, dtype=np.int32)
  if count == 0:
    return single.astype(bool), heights
  handle = _lib.default_handle()
  with contextlib.ExitStack() as held:
    sources = [held.enter_context(_dlpack.describe(e, lambda: handle)) for e in embeddings_list]
    d = sources[0].shape[1]
    if any(src.shape[1] != d for src in sources):
      raise ValueError("all utterances must be (n_i, d) with the same d")
    handle.check(handle.lib.sc_batch_fallback_check(
        handle.raw, (_lib.ScArray * count)(*[src.array for src in sources]), count,
        float(distance_threshold), _lib.as_double_p(heights),
        single.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
  return single.astype(bool), heights
