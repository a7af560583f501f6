"""How a batch chooses its library call, and the one marshalling path of those calls.

`SpectralClusterer.predict_batch`, `predict_affinity_batch` and `predict_device_batch` each make
a `Form`, ask for a `Plan` and `execute` it:

  plan()       reads the clusterer, the form, the flags and the constraints and names the call
               family (`Family`) -- it touches no handle and launches nothing;
  described()  is the marshalling preamble of every family: the inputs described as `sc_array`s,
               the label, pointer and diagnostics arrays allocated, every source released on exit;
  execute()    runs the family's executor: what predict() would raise for an utterance, the ONE
               library call with its arguments, the report, predict()'s result dtypes;
  labels_into() is the way out of every entry that was given `out=`: the destinations validated
               before the executor runs, one `sc_labels_egress` call after it.

Everything goes through `c._handle()`, `c.build_config()` and `c.predict(...)` on the instance.
`tests/golden/batch_dispatch.json` records what each call of a grid of them does.
"""

from __future__ import annotations

import contextlib
import copy
import ctypes
import enum
import typing

import numpy as np

from spectralcluster_amd import _dlpack
from spectralcluster_amd import _lib
from spectralcluster_amd import constraint as constraint_lib
from spectralcluster_amd import custom_distance_kmeans
from spectralcluster_amd import fallback_clusterer
from spectralcluster_amd import refinement
from spectralcluster_amd import utils

# the constraint forms that travel inside a library batch call
BATCH_CONSTRAINTS = (constraint_lib.ConstraintMatrix, constraint_lib.PairwiseConstraints,
                     constraint_lib.DenseConstraints)


class Form(typing.NamedTuple):
  """(group, streams) of a batch call, read once.  `grouped`: the library-batch form -- no
  `streams`, `group` not 1; `group_arg` / `streams_arg`: what the library is given."""
  grouped: bool
  group_arg: int
  streams_arg: int

  @classmethod
  def make(cls, group: typing.Optional[int], streams: typing.Optional[int]) -> "Form":
    grouped = streams is None and (group is None or int(group) > 1)
    if group is None:
      group = 16 if streams is None else 0
    return cls(grouped, int(group), 1 if streams is None else max(1, int(streams)))


class Flags(typing.NamedTuple):
  """The opt-in keywords of predict_batch."""
  entry_state: bool = False
  fallback_condition: bool = False
  naive_fallback: bool = False
  multi_stage: bool = False
  any_metric: bool = False


class Family(enum.Enum):
  """One member per distinct library route, and the three loops."""
  AUTOTUNE = "sc_predict_batch_autotune"
  MULTI_STAGE = "sc_predict_batch_multi_stage"
  SINGLE_FALLBACK = "sc_predict_batch_single_fallback / _single_naive"
  SINGLE = "sc_predict_batch_single"
  CONSTRAINED = "sc_predict_batch_constrained / _constraints / _constraint_arrays"
  REDUCED = "sc_predict_batch_reduced / _reduced_naive"
  PLAIN = "sc_predict_batch_grouped / _streams / _arrays"
  AFFINITIES = "sc_predict_batch_affinities / _constraint_arrays"
  LOOP = "predict() per utterance"
  LOOP_ENTRY_STATE = "predict() per utterance on a copy of the AutoTune object"
  LOOP_AFFINITY = "predict_affinity() per matrix"


class Plan(typing.NamedTuple):
  """What `execute` needs.  `constraints`: the list that travels (or goes to the loop), None
  when none was given or the family drops it; `naive`: the `_naive` variant of the call;
  `single_check`: the `sc_single_check` of `Family.SINGLE`."""
  family: Family
  constraints: typing.Optional[typing.List] = None
  naive: bool = False
  single_check: typing.Optional[_lib.ScSingleCheck] = None


# ---------------------------------------------------------------- the clauses
def no_autotune(c) -> bool:
  return c.autotune is None


def default_affinity(c) -> bool:
  return c.affinity_function is utils.compute_affinity_matrix


def default_kmeans(c) -> bool:
  return c.post_eigen_cluster_function is custom_distance_kmeans.run_kmeans


def kmeans_ok(c) -> bool:
  """Is this clusterer's k-means one the grouped batch runs?  The cosine one; under
  `batch_any_metric` every metric that is on the device.  False for a metric that is not
  (predict() raises what it raises today)."""
  try:
    metric = _lib.kmeans_metric_code(c.custom_dist)
  except (ValueError, _lib.UnsupportedOnDeviceError):
    return False
  return metric == _lib.KMEANS_METRICS["cosine"] or c._batch_any_metric


def _by_fallback(c, naive: bool) -> bool:
  """min_clusters == 1 decided by the FallbackClusterer condition, with a fallback type the
  batch takes: the agglomerative one, with `naive` the Naive one as well."""
  options = c.fallback_options
  return (c.min_clusters == 1 and options.single_cluster_condition ==
          fallback_clusterer.SingleClusterCondition.FallbackClusterer and
          (options.fallback_clusterer_type == fallback_clusterer.FallbackClustererType.Agglomerative
           or (naive and c._naive_fallback())))


def _sizes_nest(c) -> bool:
  """The centroids of a size-reduced utterance are no fallback members themselves."""
  return (c.max_spectral_size is None or
          c.max_spectral_size >= c.fallback_options.spectral_min_embeddings)


def _multi_stage_options(c) -> bool:
  return c.max_spectral_size is not None or c.fallback_options.spectral_min_embeddings > 1


def library_covers(c, min_embeddings_met=False, single_check_covered=False, affinity_input=False,
                   autotune_ok=False) -> bool:
  """`SpectralClusterer._library_batch_covers`; `autotune_ok`: the caller carries the search."""
  embeddings_read = not affinity_input
  return ((autotune_ok or no_autotune(c)) and default_kmeans(c) and
          not (embeddings_read and c.max_spectral_size is not None) and
          (c.min_clusters != 1 or
           (single_check_covered and c._single_check_struct() is not None)) and
          not (embeddings_read and c.fallback_options.spectral_min_embeddings > 1 and
               not min_embeddings_met) and
          (default_affinity(c) or affinity_input))


def fallback_condition_covers(c, min_embeddings_met=False, naive=False) -> bool:
  """`SpectralClusterer._fallback_condition_covers`."""
  return (_by_fallback(c, naive) and no_autotune(c) and c.max_spectral_size is None and
          (c.fallback_options.spectral_min_embeddings <= 1 or min_embeddings_met) and
          default_affinity(c) and default_kmeans(c) and c._batch_kmeans_ok())


def reduced_covers(c, utterances, grouped: bool, naive=False) -> bool:
  """`SpectralClusterer._reduced_batch_covers` for a batch that is `grouped` or not."""
  if not (_multi_stage_options(c) and no_autotune(c) and c.min_clusters != 1 and
          default_affinity(c) and default_kmeans(c) and grouped and c._batch_kmeans_ok() and
          _sizes_nest(c)):
    return False
  try:
    kinds = [c._batch_kind(int(np.shape(u)[0])) for u in utterances]
  except (IndexError, TypeError):
    return False  # (not (n, d): predict() says what is wrong with it)
  return (_lib.BATCH_KIND_FALLBACK not in kinds or c.fallback_options.fallback_clusterer_type ==
          fallback_clusterer.FallbackClustererType.Agglomerative or
          (naive and c._naive_fallback()))


def multi_stage_covers(c) -> bool:
  """`SpectralClusterer._multi_stage_batch_covers`."""
  options = c.fallback_options
  return (c.min_clusters == 1 and _multi_stage_options(c) and no_autotune(c) and
          default_affinity(c) and default_kmeans(c) and _sizes_nest(c) and
          # (predict() says what is wrong with an option that is no member of its enum)
          isinstance(options.single_cluster_condition, fallback_clusterer.SingleClusterCondition)
          and isinstance(options.fallback_clusterer_type, fallback_clusterer.FallbackClustererType)
          and c._batch_kmeans_ok())


# ---------------------------------------------------- per-utterance ValueErrors
def _at(index: typing.Optional[int]) -> str:
  return "" if index is None else " (utterance %d)" % index


def too_few_samples(n: int, index: typing.Optional[int] = None) -> ValueError:
  return ValueError("Found array with %d sample(s) while a minimum of 2 is required by "
                    "AgglomerativeClustering.%s" % (n, _at(index)))


def spectral_size_too_small(c) -> bool:
  """predict()'s test of `max_spectral_size` (reference spectral_clusterer.py:240-244)."""
  return bool(c.max_spectral_size < 2 or
              (c.max_clusters and c.max_spectral_size <= c.max_clusters) or
              (c.min_clusters and c.max_spectral_size <= c.min_clusters))


def small_spectral_size(index: typing.Optional[int] = None) -> ValueError:
  return ValueError("max_spectral_size should be a relatively big number%s" % _at(index))


def check_rows(c, rows: typing.Sequence[int], condition: int = 0, offset: int = 0,
               index: bool = True, kinds: bool = True) -> None:
  """What predict() raises for an utterance, before anything is launched (the library checks the
  same).  `condition` / `offset`: the single-cluster test the call carries (`SC_SINGLE_*`, 0
  none); `index`: name the utterance; `kinds`: the utterances are classified (`_batch_kind`) --
  a fallback utterance is not tested, of a size-reduced one the centroids are."""
  agglomerative = not c._naive_fallback()
  for i, n in enumerate(rows):
    at = i if index else None
    kind = c._batch_kind(n) if kinds else _lib.BATCH_KIND_SPECTRAL
    if kind == _lib.BATCH_KIND_FALLBACK:
      if n < 2 and agglomerative:
        raise too_few_samples(n, at)
      continue
    if kind == _lib.BATCH_KIND_REDUCED:
      if spectral_size_too_small(c):
        raise small_spectral_size(at)
      n = c.max_spectral_size  # what is tested: the centroids
    if condition == _lib.SC_SINGLE_GMM_BIC and (offset < 0 or offset >= n - 1):
      raise ValueError("single_cluster_affinity_diagonal_offset must be significantly smaller "
                       "than affinity matrix dimension%s" % _at(at))
    if condition == _lib.SC_SINGLE_BY_FALLBACK and agglomerative and n < 2:
      raise too_few_samples(n, at)


def check_length(constraint_matrices, count: int) -> None:
  if constraint_matrices is not None and len(constraint_matrices) != count:
    raise ValueError("constraint_matrices must be as long as the batch")


def check_constraint(c, n: int, constraint_matrix) -> None:
  """predict()'s check and message (`_set_constraint`) against an (n, n) affinity: only its
  shape is read."""
  c.constraint_options.constraint_operator.check_input(
      np.lib.stride_tricks.as_strided(np.zeros(1, dtype=bool), (n, n), (0, 0)), constraint_matrix)


def check_autotune_sequence(c) -> None:
  if refinement.RefinementName.RowWiseThreshold not in (
      c.refinement_options.refinement_sequence or []):
    raise ValueError(
        "AutoTune is only effective when the refinement sequence"
        "contains RowWiseThreshold")


# ------------------------------------------------------------------- the plan
def wants_permission(c, form: Form, flags: Flags) -> bool:
  """Is the any-metric permission to be held around plan and execution?  `batch_any_metric`,
  the library-batch form, a device metric other than cosine -- and no entry-state AutoTune
  batch, which ignores the flag."""
  return (flags.any_metric and form.grouped and
          not (flags.entry_state and c.autotune is not None) and c._metric_needs_permission())


def plan(c, form: Form, flags: Flags, constraint_matrices, utterances) -> Plan:
  """The call family of predict_batch, in today's precedence: entry-state AutoTune, multi-stage,
  fallback condition, affinity single check, constrained or the loop, reduced, the loop, plain.
  Raises the length mismatch, and what the entry-state batch raises before it launches."""
  check_length(constraint_matrices, len(utterances))
  if flags.entry_state and c.autotune is not None:
    return _plan_entry_state(c, form, constraint_matrices, utterances)
  travels = constraint_matrices is not None and c.constraint_options is not None
  if (flags.multi_stage and form.grouped and constraint_matrices is None and
      c._multi_stage_batch_covers()):
    return Plan(Family.MULTI_STAGE)
  if (flags.fallback_condition and form.grouped and not travels and
      c._fallback_condition_covers(naive=flags.naive_fallback)):
    return Plan(Family.SINGLE_FALLBACK, naive=c._naive_fallback())
  covered = c._library_batch_covers()
  if (not covered and c.min_clusters == 1 and not travels and form.grouped and
      c._library_batch_covers(single_check_covered=True) and c._batch_kmeans_ok()):
    # the test travels inside the call; constraints without constraint_options are dropped
    return Plan(Family.SINGLE, single_check=c._single_check_struct())
  if travels:
    # (a metric that is not on the device raises in predict(), as it does today)
    if (covered and c._batch_kmeans_ok() and form.grouped and
        all(m is None or isinstance(m, BATCH_CONSTRAINTS) for m in constraint_matrices)):
      return Plan(Family.CONSTRAINED, list(constraint_matrices))
    return Plan(Family.LOOP, list(constraint_matrices))
  if not covered and reduced_covers(c, utterances, form.grouped, naive=flags.naive_fallback):
    return Plan(Family.REDUCED)
  if not covered:
    # anything the library batch does not cover (user-supplied affinity / clustering functions,
    # AutoTune, size reduction, fallback decisions) goes through predict().  A batch never
    # carries a constraint matrix without constraint_options -- same as predict(u) without one.
    return Plan(Family.LOOP)
  return Plan(Family.PLAIN)


def _plan_entry_state(c, form: Form, constraint_matrices, utterances) -> Plan:
  """predict_batch(autotune_from_entry_state=True) on a clusterer with AutoTune: ONE
  `sc_predict_batch_autotune` call where the library batch covers the clusterer, else predict()
  per utterance on a copy of the object."""
  count = len(utterances)
  if constraint_matrices is None:
    constraint_matrices = [None] * count
  check_autotune_sequence(c)
  if c.constraint_options is not None:
    for u, cm in zip(utterances, constraint_matrices):
      if isinstance(cm, (constraint_lib.ConstraintMatrix, constraint_lib.DenseConstraints)):
        check_constraint(c, int(np.shape(u)[0]), cm)
  try:  # (a metric that is not on the device raises in predict(), as it does today)
    cosine = _lib.kmeans_metric_code(c.custom_dist) == _lib.KMEANS_METRICS["cosine"]
  except (ValueError, _lib.UnsupportedOnDeviceError):
    cosine = False
  if (library_covers(c, autotune_ok=True) and cosine and form.grouped and count and
      all(m is None or isinstance(m, constraint_lib.ConstraintMatrix)
          for m in constraint_matrices)):
    return Plan(Family.AUTOTUNE, list(constraint_matrices))
  return Plan(Family.LOOP_ENTRY_STATE, list(constraint_matrices))


def plan_affinity(c, form: Form, constraint_matrices: typing.Sequence, count: int) -> Plan:
  """The call family of predict_affinity_batch (its checks have passed)."""
  constrained = c.constraint_options is not None and any(
      m is not None for m in constraint_matrices)
  try:  # (a metric that is not on the device raises in predict_affinity, as in predict())
    _lib.kmeans_metric_code(c.custom_dist)
    metric_ok = not constrained or c._batch_kmeans_ok()
  except (ValueError, _lib.UnsupportedOnDeviceError):
    metric_ok = False
  if (count and metric_ok and c._library_batch_covers(affinity_input=True) and form.grouped and
      all(m is None or isinstance(m, BATCH_CONSTRAINTS) for m in constraint_matrices)):
    return Plan(Family.AFFINITIES, list(constraint_matrices) if constrained else None)
  return Plan(Family.LOOP_AFFINITY, list(constraint_matrices))


def plan_device(c, fallback_condition: bool) -> Plan:
  """The call family of predict_device_batch."""
  if fallback_condition and c._fallback_condition_covers(min_embeddings_met=True):
    return Plan(Family.SINGLE_FALLBACK)
  if c.min_clusters == 1:
    # (the caller's predicate: _library_batch_covers(single_check_covered=True))
    return Plan(Family.SINGLE, single_check=c._single_check_struct())
  return Plan(Family.PLAIN)


# ------------------------------------------------------------ the marshalling
class Described:
  """The inputs of a batch as the library takes them: `rows` per input, the label arrays with
  their pointer array `lp`, `diags`, and `arrays` -- the `sc_array`s of `sources`, or the ones
  the caller gave."""

  def __init__(self, sources: typing.List[_dlpack.Source], dense_sources: typing.List,
               given: typing.Optional[typing.Sequence[_lib.ScArray]] = None):
    self.sources, self.dense_sources, self._given = sources, dense_sources, given
    self.rows = ([src.shape[0] for src in sources] if given is None
                 else [int(a.rows) for a in given])
    self.count = count = len(self.rows)
    self.labels = [np.empty(n, dtype=np.int64) for n in self.rows]
    self.lp = (ctypes.POINTER(ctypes.c_int64) * count)(*[_lib.as_int64_p(l) for l in self.labels])
    self.diags = (_lib.ScDiag * count)()

  @property
  def arrays(self):
    given = [src.array for src in self.sources] if self._given is None else self._given
    return (_lib.ScArray * self.count)(*given)

  @property
  def host_f64(self) -> bool:
    """Compact float64 host rows throughout: what the `double*` forms take."""
    return self._given is None and all(src.is_host_f64 for src in self.sources)

  def int32s(self):
    return (ctypes.c_int32 * self.count)()


@contextlib.contextmanager
def described(c, inputs: typing.Sequence = (), strided: bool = False, arrays=None):
  """`inputs` described under the clusterer's device (`strided`: affinities, which keep their
  strides and have been checked) -- or `arrays`, `sc_array`s the caller holds -- as a
  `Described`; every source, the dense constraints' included, is released on exit."""
  sources, dense_sources = [], []
  try:
    if arrays is None:
      same_d = "all utterances must be (n_i, d) with the same d"
      if not strided and any(isinstance(u, np.ndarray) and u.ndim != 2 for u in inputs):
        raise ValueError(same_d)
      with _lib.use_device(c.device):
        for u in inputs:
          sources.append(_dlpack.describe(u, c._handle, strided=strided))
      d = sources[0].shape[1] if sources else 0
      if not strided and any(src.shape[1] != d for src in sources):
        raise ValueError(same_d)
    yield Described(sources, dense_sources, arrays)
  finally:
    for src in sources + dense_sources:
      src.release()


def band_buffer(constraint_matrix, n: int) -> np.ndarray:
  band = np.zeros(max(n - 1, 1), dtype=np.float64)  # (n = 1: no values, a valid pointer)
  band[:n - 1] = constraint_matrix.band()
  return band


def band_pointers(constraint_matrices: typing.Sequence, rows: typing.Sequence[int]):
  """The `bands` argument of the band-only calls: NULL where there is no constraint.  Returns
  (pointer array, the buffers to keep alive)."""
  bands = [None if cm is None else band_buffer(cm, n) for cm, n in zip(constraint_matrices, rows)]
  return (ctypes.POINTER(ctypes.c_double) * len(bands))(
      *[None if b is None else _lib.as_double_p(b) for b in bands]), bands


def constraint_descriptors(constraint_matrices: typing.Sequence, rows: typing.Sequence[int]):
  """One `sc_constraint_desc` per utterance: kind 2 a band, 3 an entry list, 0 none or a dense
  matrix (which travels in `dense`).  Returns (array, the buffers to keep alive)."""
  cons, keep = (_lib.ScConstraintDesc * len(rows))(), []
  for desc, n, cm in zip(cons, rows, constraint_matrices):
    if cm is None or isinstance(cm, constraint_lib.DenseConstraints):
      continue
    if isinstance(cm, constraint_lib.PairwiseConstraints):
      entries = cm.entries()  # (rows, cols, vals)
      keep.append(entries)
      desc.kind, desc.count = 3, len(entries[2])
      desc.rows, desc.cols = _lib.as_int32_p(entries[0]), _lib.as_int32_p(entries[1])
      desc.vals = _lib.as_double_p(entries[2])
    else:
      keep.append(band_buffer(cm, n))
      desc.kind, desc.band = 2, _lib.as_double_p(keep[-1])
  return cons, keep


def describe_dense(c, constraint_matrices: typing.Sequence, sources: typing.List):
  """The `dense` list of `sc_predict_batch_constraint_arrays` -- one `sc_array` per utterance,
  `data` NULL where its constraint is no `DenseConstraints` -- or None when the batch holds
  none.  The described matrices are appended to `sources` (`Described.dense_sources`)."""
  if not any(isinstance(m, constraint_lib.DenseConstraints) for m in constraint_matrices):
    return None
  dense = (_lib.ScArray * len(constraint_matrices))()
  with _lib.use_device(c.device):
    for i, cm in enumerate(constraint_matrices):
      if isinstance(cm, constraint_lib.DenseConstraints):
        sources.append(cm.describe(c._handle))
        dense[i] = sources[-1].array
  return dense


def results(c, labels: typing.Sequence[np.ndarray], kinds=None, single=None):
  """Raw labels -> predict()'s results: float64 for a size-reduced utterance (utils.chain_labels
  fills np.zeros), `np.array([0] * n)` for one found single, int64 otherwise.  Sets
  `last_batch_reduced` from `kinds` and `last_batch_single` from `single` (negative: a fallback
  utterance, not tested: None) when the call reported them."""
  count = len(labels)
  if kinds is not None:
    c.last_batch_reduced = [int(k) for k in kinds]
  if single is not None:
    c.last_batch_single = [None if v < 0 else bool(v) for v in single]
  if kinds is None and single is None:
    return labels
  out = []
  for l, k, one in zip(labels, kinds if kinds is not None else [0] * count,
                       single if single is not None else [0] * count):
    if k == _lib.BATCH_KIND_REDUCED:
      out.append(l.astype(np.float64))
    else:
      out.append(np.array([0] * l.shape[0]) if one > 0 else l)
  return out


# -------------------------------------------------- one executor per library symbol
def _double_rows(batch: Described):
  """Compact float64 host rows as the `double*` forms take them: (x pointers, n per utterance,
  d).  (`sc_predict_batch_arrays` runs the same code on the descriptors of exactly these.)"""
  xp = (ctypes.POINTER(ctypes.c_double) * batch.count)(
      *[_lib.as_double_p(src.keep) for src in batch.sources])
  return xp, (ctypes.c_int * batch.count)(*batch.rows), batch.sources[0].shape[1]


def _grouped(c, handle, batch: Described, form: Form):
  xp, ns, d = _double_rows(batch)
  handle.check(handle.lib.sc_predict_batch_grouped(
      handle.raw, xp, ns, d, batch.count, c.build_config(), batch.lp, batch.diags,
      form.group_arg), TypeError)


def _streams(c, handle, batch: Described, form: Form):
  xp, ns, d = _double_rows(batch)
  handle.check(handle.lib.sc_predict_batch_streams(
      handle.raw, xp, ns, d, batch.count, c.build_config(), batch.lp, batch.diags,
      form.streams_arg), TypeError)


def _arrays(c, handle, batch: Described, form: Form):
  handle.check(handle.lib.sc_predict_batch_arrays(
      handle.raw, batch.arrays, batch.count, c.build_config(), batch.lp, batch.diags,
      form.group_arg, form.streams_arg), TypeError)


def _constrained(c, handle, batch: Described, form: Form, constraint_matrices, dense):
  """Bands alone: `sc_predict_batch_constrained`; an entry list or a dense matrix among them:
  one descriptor per utterance."""
  if dense is None and not any(isinstance(m, constraint_lib.PairwiseConstraints)
                               for m in constraint_matrices):
    bp, keep = band_pointers(constraint_matrices, batch.rows)
    handle.check(handle.lib.sc_predict_batch_constrained(
        handle.raw, batch.arrays, bp, batch.count, c.build_config(), batch.lp, batch.diags,
        form.group_arg), TypeError)
    return
  _described_constraints(c, handle, batch, form, constraint_matrices, dense, 0)


def _described_constraints(c, handle, batch: Described, form: Form, constraint_matrices, dense,
                           affinity_input: int):
  """`sc_predict_batch_constraint_arrays` when a dense matrix travels, else the descriptor call
  of the input kind: `_constraints` for embeddings, `_affinities` for affinities."""
  cons, keep = (None, None) if constraint_matrices is None else constraint_descriptors(
      constraint_matrices, batch.rows)
  if dense is not None:
    handle.check(handle.lib.sc_predict_batch_constraint_arrays(
        handle.raw, batch.arrays, cons, dense, batch.count, c.build_config(), batch.lp,
        batch.diags, form.group_arg, affinity_input), TypeError)
    return
  call = (handle.lib.sc_predict_batch_affinities if affinity_input
          else handle.lib.sc_predict_batch_constraints)
  handle.check(call(handle.raw, batch.arrays, cons, batch.count, c.build_config(), batch.lp,
                    batch.diags, form.group_arg), TypeError)


def _single(c, handle, batch: Described, form: Form, plan: Plan):
  single_check = plan.single_check
  # (predict()'s ValueError, before anything is launched; the library checks it as well)
  check_rows(c, batch.rows, single_check.condition, single_check.diagonal_offset, kinds=False)
  single = batch.int32s()
  handle.check(handle.lib.sc_predict_batch_single(
      handle.raw, batch.arrays, batch.count, c.build_config(), ctypes.byref(single_check),
      batch.lp, batch.diags, form.group_arg, single), TypeError)
  return None, single


def _single_fallback(c, handle, batch: Described, form: Form, plan: Plan):
  """`sc_predict_batch_single_fallback` (`plan.naive`: `sc_predict_batch_single_naive`)."""
  naive = plan.naive
  if naive:
    thresholds = c._naive_thresholds()  # (NaiveClusterer's ValueError, before any launch)
  else:
    check_rows(c, batch.rows, _lib.SC_SINGLE_BY_FALLBACK, index=False, kinds=False)
  single = batch.int32s()
  if naive:
    handle.check(handle.lib.sc_predict_batch_single_naive(
        handle.raw, batch.arrays, batch.count, c.build_config(), thresholds[0], thresholds[1],
        batch.lp, batch.diags, form.group_arg, single), ValueError)
  else:
    handle.check(handle.lib.sc_predict_batch_single_fallback(
        handle.raw, batch.arrays, batch.count, c.build_config(),
        float(c.fallback_options.agglomerative_threshold), batch.lp, batch.diags, form.group_arg,
        single), ValueError)
  return None, single


def _reduced(c, handle, batch: Described, form: Form, plan: Plan):
  """`sc_predict_batch_reduced`; `_reduced_naive` when a fallback utterance meets the Naive type
  (`reduced_covers(naive=True)` let it through)."""
  naive = c._naive_fallback() and any(
      c._batch_kind(n) == _lib.BATCH_KIND_FALLBACK for n in batch.rows)
  if naive:
    thresholds = c._naive_thresholds()  # (NaiveClusterer's ValueError)
  check_rows(c, batch.rows, index=False)
  kinds = batch.int32s()
  sizes = (int(c.max_spectral_size or 0), int(c.fallback_options.spectral_min_embeddings))
  if naive:
    handle.check(handle.lib.sc_predict_batch_reduced_naive(
        handle.raw, batch.arrays, batch.count, c.build_config(), sizes[0], sizes[1],
        thresholds[0], thresholds[1], batch.lp, batch.diags, form.group_arg, kinds), ValueError)
  else:
    handle.check(handle.lib.sc_predict_batch_reduced(
        handle.raw, batch.arrays, batch.count, c.build_config(), sizes[0], sizes[1],
        float(c.fallback_options.agglomerative_threshold), batch.lp, batch.diags, form.group_arg,
        kinds), ValueError)
  return kinds, None


def _multi_stage(c, handle, batch: Described, form: Form, plan: Plan):
  stage = c._multi_stage_struct()
  check_rows(c, batch.rows, stage.single_condition, stage.diagonal_offset)
  kinds, single = batch.int32s(), batch.int32s()
  handle.check(handle.lib.sc_predict_batch_multi_stage(
      handle.raw, batch.arrays, batch.count, c.build_config(), ctypes.byref(stage), batch.lp,
      batch.diags, form.group_arg, kinds, single), ValueError)
  return kinds, single


def autotune_call(c, utterances, constraint_matrices, group: int):
  """`SpectralClusterer._autotune_library_batch`: ONE `sc_predict_batch_autotune` call."""
  with described(c, utterances) as batch:
    if c.constraint_options is None:
      constraint_matrices = [None] * batch.count
    bp, keep = band_pointers(constraint_matrices, batch.rows)
    handle = c._handle()
    best_p = np.zeros(batch.count, dtype=np.float64)
    last_p = np.zeros(batch.count, dtype=np.float64)
    state = c.autotune.to_struct()
    handle.check(handle.lib.sc_predict_batch_autotune(
        handle.raw, batch.arrays, bp, batch.count, c.build_config(), ctypes.byref(state),
        batch.lp, batch.diags, _lib.as_double_p(best_p), int(group), _lib.as_double_p(last_p)),
        TypeError)
  c._batch_report(handle, batch.diags, batch.count)
  c.last_batch_best_p = [float(p) for p in best_p]
  # reference closure: p_percentile stays at the last value evaluated (spectral_clusterer.py:277)
  c.refinement_options.p_percentile = float(last_p[-1])
  c.last_best_p = float(best_p[-1])
  c.last_diag = batch.diags[batch.count - 1]
  return batch.labels


# ------------------------------------------------------- one executor per family
def _empty(c, *reports: str):
  """An empty batch is no call at all: the family's reports are empty lists."""
  for name in ("last_batch_routes",) + reports:
    setattr(c, name, [])
  return []


def _run_library(c, plan: Plan, form: Form, utterances):
  """The plain, constrained and single-check families: a batch carries no resident constraint."""
  _lib.kmeans_metric_code(c.custom_dist)  # raises for metrics that are not on the device
  if not utterances:
    return _empty(c)
  kinds = single = None
  with described(c, utterances) as batch:
    dense = None
    if plan.family is Family.CONSTRAINED:
      for n, cm in zip(batch.rows, plan.constraints):
        if cm is not None:
          check_constraint(c, n, cm)
      dense = describe_dense(c, plan.constraints, batch.dense_sources)
    handle = c._handle()
    handle.check(handle.lib.sc_clear_constraint(handle.raw))  # a batch carries none
    if plan.family is Family.SINGLE:
      kinds, single = _single(c, handle, batch, form, plan)
    elif plan.family is Family.CONSTRAINED:
      _constrained(c, handle, batch, form, plan.constraints, dense)
    elif batch.host_f64:
      (_grouped if form.group_arg > 1 else _streams)(c, handle, batch, form)
    else:
      _arrays(c, handle, batch, form)
  c._batch_report(handle, batch.diags, batch.count)
  return results(c, batch.labels, kinds, single)


# family -> (its call, the reports an empty batch leaves empty besides the routes)
_STAGED = {
    Family.SINGLE_FALLBACK: (_single_fallback, ("last_batch_single", "last_batch_diags")),
    Family.REDUCED: (_reduced, ("last_batch_reduced", "last_batch_diags")),
    Family.MULTI_STAGE: (_multi_stage, ("last_batch_reduced", "last_batch_diags",
                                        "last_batch_single")),
}


def _run_staged(c, plan: Plan, form: Form, utterances):
  """The families that classify or test utterances before the grouped batch: fallback
  condition, reduced, multi-stage."""
  call, reports = _STAGED[plan.family]
  if not utterances:
    return _empty(c, *reports)
  with described(c, utterances) as batch:
    handle = c._handle()
    kinds, single = call(c, handle, batch, form, plan)
  c._batch_report(handle, batch.diags, batch.count)
  return results(c, batch.labels, kinds, single)


def _run_affinities(c, plan: Plan, form: Form, affinities):
  with described(c, affinities, strided=True) as batch:
    handle = c._handle()
    handle.check(handle.lib.sc_clear_constraint(handle.raw))
    dense = None
    if plan.constraints is not None:
      dense = describe_dense(c, plan.constraints, batch.dense_sources)
    _described_constraints(c, handle, batch, form, plan.constraints, dense, 1)
  c._batch_report(handle, batch.diags, batch.count)
  return batch.labels


def _run_loop(c, plan: Plan, form: Form, utterances):
  c.last_batch_routes = [_lib.BATCH_ROUTE_SINGLE] * len(utterances)
  if plan.constraints is None:
    return [c.predict(u) for u in utterances]
  return [c.predict(u, cm) for u, cm in zip(utterances, plan.constraints)]


def _run_loop_entry_state(c, plan: Plan, form: Form, utterances):
  entry = c.autotune
  labels, best_p, diags = [], [], []
  try:
    for u, cm in zip(utterances, plan.constraints):
      c.autotune = copy.deepcopy(entry)
      c.last_best_p = None
      labels.append(c.predict(u, cm))
      # (None: the utterance left predict() before the search -- fallback, size reduction)
      best_p.append(c.last_best_p)
      diags.append(c.last_diag)
  finally:
    c.autotune = entry
  c.last_batch_best_p = best_p
  c.last_batch_diags = diags
  c.last_batch_routes = [_lib.BATCH_ROUTE_SINGLE] * len(utterances)
  return labels


def _run_loop_affinity(c, plan: Plan, form: Form, affinities):
  labels, diags = [], []
  for a, cm in zip(affinities, plan.constraints):
    labels.append(c.predict_affinity(a, cm))
    diags.append(c.last_diag)
  c.last_batch_routes = [_lib.BATCH_ROUTE_SINGLE] * len(affinities)
  c.last_batch_diags = diags
  return labels


_EXECUTORS = {
    # (through the instance: a caller may have replaced the method)
    Family.AUTOTUNE: lambda c, plan, form, utterances: c._autotune_library_batch(
        utterances, plan.constraints, form.group_arg),
    Family.MULTI_STAGE: _run_staged,
    Family.SINGLE_FALLBACK: _run_staged,
    Family.REDUCED: _run_staged,
    Family.SINGLE: _run_library,
    Family.CONSTRAINED: _run_library,
    Family.PLAIN: _run_library,
    Family.AFFINITIES: _run_affinities,
    Family.LOOP: _run_loop,
    Family.LOOP_ENTRY_STATE: _run_loop_entry_state,
    Family.LOOP_AFFINITY: _run_loop_affinity,
}


def execute(c, plan: Plan, form: Form, inputs, out=None) -> typing.List:
  """`out` (a list with one label destination per input, or None): every one is validated before
  the executor runs, and receives its input's labels after it -- whatever the family."""
  if out is None:
    return _EXECUTORS[plan.family](c, plan, form, inputs)
  if len(out) != len(inputs):
    raise ValueError("out must be as long as the batch")
  return labels_into(c, out, [rows_of(c, u) for u in inputs],
                     lambda: _EXECUTORS[plan.family](c, plan, form, inputs))


# ----------------------------------------------------------------- labels out
def rows_of(c, array) -> int:
  """n of an input of a predict entry: its `shape` where it has one (an ndarray, a tensor);
  an object that only speaks DLPack is described, as the entry will describe it, and says n
  that way; anything else is what predict() refuses."""
  shape = getattr(array, "shape", None)
  if shape is None and _dlpack.is_described(array):
    with _lib.use_device(c.device):
      src = _dlpack.describe(array, c._handle, strided=True)
    with src:
      return src.shape[0]
  if shape is None or len(shape) == 0:
    raise TypeError("embeddings must be a numpy array")
  return int(shape[0])


def exact_int64(labels) -> np.ndarray:
  """The labels a predict entry returned, as contiguous int64: the float64 labels of a
  size-reduced utterance (utils.chain_labels) are converted exactly."""
  a = np.asarray(labels)
  as_int = np.ascontiguousarray(a, dtype=np.int64)
  if a.dtype.kind == "f" and not np.array_equal(as_int, a):
    raise ValueError("labels are not integral")
  return as_int


def labels_into(c, outs: typing.Sequence, rows: typing.Sequence[int], run) -> typing.List:
  """The label egress of every predict entry: `outs[i]` -- a 1-D int64 / int32 array of exactly
  `rows[i]` entries, NumPy or DLPack, host or the clusterer's device, any stride >= 1 -- is
  described (`_dlpack.describe_labels_out`: type, dtype, length, writeability, stride, device)
  before `run()` launches anything, and receives the labels `run()` returns in ONE
  `sc_labels_egress` call.  Returns `outs` as a list."""
  with contextlib.ExitStack() as held:
    with _lib.use_device(c.device):
      described_outs = [held.enter_context(_dlpack.describe_labels_out(
          o, c._handle, n, "out" if len(outs) == 1 else "out %d" % i))
                        for i, (o, n) in enumerate(zip(outs, rows))]
    labels = [exact_int64(l) for l in run()]
    count = len(described_outs)
    if count:
      handle = c._handle()
      lp = (ctypes.POINTER(ctypes.c_int64) * count)(*[_lib.as_int64_p(l) for l in labels])
      handle.check(handle.lib.sc_labels_egress(
          handle.raw, lp, count, (_lib.ScArray * count)(*[src.array for src in described_outs])))
  return list(outs)


def execute_device(c, plan: Plan, form: Form, arrays: typing.Sequence[_lib.ScArray]):
  """predict_device_batch: the caller's `sc_array`s; the grouped calls get a group of 2 at the
  least."""
  grouped = form._replace(group_arg=max(2, form.group_arg))
  kinds = single = None
  with described(c, arrays=arrays) as batch:
    handle = c._handle()
    handle.check(handle.lib.sc_clear_constraint(handle.raw))  # a batch carries none
    if plan.family is Family.SINGLE_FALLBACK:
      kinds, single = _single_fallback(c, handle, batch, grouped, plan)
    elif plan.family is Family.SINGLE:
      if plan.single_check is None:
        raise ValueError("predict_device_batch: min_clusters=1 needs a single-cluster condition "
                         "that reads the affinity")
      kinds, single = _single(c, handle, batch, grouped, plan)
    else:
      _arrays(c, handle, batch, form)
  c._batch_report(handle, batch.diags, batch.count)
  return results(c, batch.labels, kinds, single)
