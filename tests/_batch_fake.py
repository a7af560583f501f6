"""One stand-in library for every batch symbol predict_batch, predict_affinity_batch and
predict_device_batch can call, the stand-in handle that carries it, and `wire`, which puts a
clusterer on them -- so that the dispatch of a batch can be driven, and recorded, without a device.

The outputs are deterministic: kinds are classified as the library does, a tested member of an
odd number of rows is "single" (label 0), label 1 is written elsewhere.  Every call is one event,
a short string: the symbol without its `sc_predict_batch_` prefix, the rows per utterance, every
scalar argument, the fields of a struct argument, kind:count per constraint descriptor, and
`any=` the value of the clusterer's `_batch_any_metric` during the call.  A looped utterance
(predict / predict_affinity on the instance) is an event too: `p<rows>`, `+c` when a constraint
came along."""

import ctypes

import numpy as np

from spectralcluster_amd import _lib

PREFIX = "sc_predict_batch_"
BATCH_SYMBOLS = tuple(PREFIX + name for name in (
    "grouped", "streams", "arrays", "constrained", "constraints", "constraint_arrays",
    "affinities", "single", "single_fallback", "single_naive", "reduced", "reduced_naive",
    "multi_stage", "autotune"))


def _fields(struct, cls):
  s = ctypes.cast(struct, ctypes.POINTER(cls)).contents
  return "/".join("%g" % getattr(s, name) for name, _ in cls._fields_)


class FakeLib:
  """See the module's docstring.  `fail`: the name of a symbol that raises RuntimeError."""

  def __init__(self):
    self.events = []
    self.clusterer = None
    self.fail = None
    self._routes = []

  # ------------------------------------------------------------------ helpers
  def _event(self, symbol, rows, **scalars):
    text = "%s rows=%s" % (symbol[len(PREFIX):], ",".join(str(n) for n in rows))
    for key, value in scalars.items():
      text += " %s=%s" % (key, value if isinstance(value, str) else "%g" % value)
    text += " any=%d" % bool(getattr(self.clusterer, "_batch_any_metric", False))
    self.events.append(text)
    if symbol == self.fail:
      raise RuntimeError("the library call failed")

  def _write(self, rows, lp, single=None, kinds=None):
    """Label 0 for a member found single, 1 elsewhere; route 3 for a fallback member."""
    self._routes = []
    for i, n in enumerate(rows):
      one = single is not None and single[i] == 1
      for r in range(n):
        lp[i][r] = 0 if one else 1
      self._routes.append(3 if kinds is not None and kinds[i] == 2 else (2 if n <= 128 else 1))
    return 0

  @staticmethod
  def _rows(arrays, count):
    return [int(arrays[i].rows) for i in range(count)]

  @staticmethod
  def _classify(rows, mss, low, kinds):
    for i, n in enumerate(rows):
      kinds[i] = 2 if n < low else (1 if mss > 0 and n > mss else 0)

  @staticmethod
  def _descriptors(cons, count):
    return "-" if cons is None else ",".join(
        "%d:%d" % (cons[i].kind, cons[i].count) for i in range(count))

  # ------------------------------------------------------------- small symbols
  def sc_clear_constraint(self, raw):
    self.events.append("clear")
    return 0

  def sc_set_batch_any_metric(self, raw, value):
    self.events.append("permit=%d" % value)
    return 0

  def sc_last_batch_routes(self, raw, routes, count):
    for i in range(count):
      routes[i] = self._routes[i] if i < len(self._routes) else 0
    return 0

  # ------------------------------------------------------------- batch symbols
  def sc_predict_batch_grouped(self, raw, xp, ns, d, count, cfg, lp, diags, group):
    rows = [int(ns[i]) for i in range(count)]
    self._event(PREFIX + "grouped", rows, d=d, group=group)
    return self._write(rows, lp)

  def sc_predict_batch_streams(self, raw, xp, ns, d, count, cfg, lp, diags, streams):
    rows = [int(ns[i]) for i in range(count)]
    self._event(PREFIX + "streams", rows, d=d, streams=streams)
    return self._write(rows, lp)

  def sc_predict_batch_arrays(self, raw, arrays, count, cfg, lp, diags, group, streams):
    rows = self._rows(arrays, count)
    dtypes = ",".join(str(arrays[i].dtype) for i in range(count))
    self._event(PREFIX + "arrays", rows, dtypes=dtypes, group=group, streams=streams)
    return self._write(rows, lp)

  def sc_predict_batch_constrained(self, raw, arrays, bp, count, cfg, lp, diags, group):
    rows = self._rows(arrays, count)
    bands = ",".join("1" if bp[i] else "0" for i in range(count))
    self._event(PREFIX + "constrained", rows, bands=bands, group=group)
    return self._write(rows, lp)

  def sc_predict_batch_constraints(self, raw, arrays, cons, count, cfg, lp, diags, group):
    rows = self._rows(arrays, count)
    self._event(PREFIX + "constraints", rows, cons=self._descriptors(cons, count), group=group)
    return self._write(rows, lp)

  def sc_predict_batch_constraint_arrays(self, raw, arrays, cons, dense, count, cfg, lp, diags,
                                         group, affinity_input):
    rows = self._rows(arrays, count)
    held = ",".join(str(int(dense[i].rows)) if dense[i].data else "0" for i in range(count))
    self._event(PREFIX + "constraint_arrays", rows, cons=self._descriptors(cons, count),
                dense=held, group=group, affinity_input=affinity_input)
    return self._write(rows, lp)

  def sc_predict_batch_affinities(self, raw, arrays, cons, count, cfg, lp, diags, group):
    rows = self._rows(arrays, count)
    self._event(PREFIX + "affinities", rows, cons=self._descriptors(cons, count), group=group)
    return self._write(rows, lp)

  def sc_predict_batch_single(self, raw, arrays, count, cfg, check, lp, diags, group, single):
    rows = self._rows(arrays, count)
    for i, n in enumerate(rows):
      single[i] = n % 2
    self._event(PREFIX + "single", rows, check=_fields(check, _lib.ScSingleCheck), group=group)
    return self._write(rows, lp, single)

  def _single_by_fallback(self, name, arrays, count, lp, single, **scalars):
    rows = self._rows(arrays, count)
    kinds = [2 * (n % 2) for n in rows]   # (a single member reports route 3)
    for i, n in enumerate(rows):
      single[i] = n % 2
    self._event(PREFIX + name, rows, **scalars)
    return self._write(rows, lp, single, kinds)

  def sc_predict_batch_single_fallback(self, raw, arrays, count, cfg, threshold, lp, diags, group,
                                       single):
    return self._single_by_fallback("single_fallback", arrays, count, lp, single,
                                    threshold=threshold, group=group)

  def sc_predict_batch_single_naive(self, raw, arrays, count, cfg, threshold, adaptation, lp,
                                    diags, group, single):
    return self._single_by_fallback("single_naive", arrays, count, lp, single,
                                    threshold=threshold, adaptation=adaptation, group=group)

  def _reduced(self, name, arrays, count, mss, low, lp, kinds, **scalars):
    rows = self._rows(arrays, count)
    self._classify(rows, mss, low, kinds)
    self._event(PREFIX + name, rows, mss=mss, low=low, **scalars)
    return self._write(rows, lp, None, kinds)

  def sc_predict_batch_reduced(self, raw, arrays, count, cfg, mss, low, threshold, lp, diags,
                               group, kinds):
    return self._reduced("reduced", arrays, count, mss, low, lp, kinds, threshold=threshold,
                         group=group)

  def sc_predict_batch_reduced_naive(self, raw, arrays, count, cfg, mss, low, threshold,
                                     adaptation, lp, diags, group, kinds):
    return self._reduced("reduced_naive", arrays, count, mss, low, lp, kinds,
                         threshold=threshold, adaptation=adaptation, group=group)

  def sc_predict_batch_multi_stage(self, raw, arrays, count, cfg, stage, lp, diags, group, kinds,
                                   single):
    rows = self._rows(arrays, count)
    s = ctypes.cast(stage, ctypes.POINTER(_lib.ScMultiStage)).contents
    self._classify(rows, s.max_spectral_size, s.spectral_min_embeddings, kinds)
    for i, n in enumerate(rows):
      single[i] = -1 if kinds[i] == 2 else n % 2
    self._event(PREFIX + "multi_stage", rows, stage=_fields(stage, _lib.ScMultiStage),
                group=group)
    return self._write(rows, lp, single, kinds)

  def sc_predict_batch_autotune(self, raw, arrays, bp, count, cfg, state, lp, diags, best_p,
                                group, last_p):
    rows = self._rows(arrays, count)
    for i in range(count):
      best_p[i] = 0.5 + 0.01 * i
      last_p[i] = 0.75 + 0.01 * i
    bands = ",".join("1" if bp[i] else "0" for i in range(count))
    self._event(PREFIX + "autotune", rows, bands=bands, state=_fields(state, _lib.ScAutoTune),
                group=group)
    return self._write(rows, lp)


class FakeHandle:
  """The stand-in handle: `lib` is a `FakeLib` unless the caller brings one of its own."""
  raw = None

  def __init__(self, lib=None):
    self.lib = FakeLib() if lib is None else lib

  def check(self, rc, *a):
    assert rc == 0


def wire(monkeypatch, c, lib=None, marker=7, keep_config=False):
  """`c` on a stand-in handle: `_handle`, `build_config` (unless `keep_config`), `predict` and
  `predict_affinity` replaced on the instance -- through `monkeypatch`, or for good when that is
  None.  The looped utterances are recorded (their rows in the returned list, an event each in a
  `FakeLib`) and answered with `marker`.  Returns (handle, looped)."""
  handle = FakeHandle(lib)
  looped = []
  events = getattr(handle.lib, "events", None)
  if isinstance(handle.lib, FakeLib):
    handle.lib.clusterer = c

  def looped_call(dtype):
    def call(u, constraint_matrix=None):
      n = int(np.shape(u)[0])
      looped.append(n)
      if events is not None and isinstance(handle.lib, FakeLib):
        events.append("p%d%s" % (n, "" if constraint_matrix is None else "+c"))
      return np.full(n, marker, dtype=dtype)
    return call

  replaced = [("_handle", lambda: handle), ("predict", looped_call(np.int64)),
              ("predict_affinity", looped_call(np.int64))]
  if not keep_config:
    replaced.append(("build_config", lambda *a: None))
  for name, value in replaced:
    if monkeypatch is None:
      setattr(c, name, value)
    else:
      monkeypatch.setattr(c, name, value)
  return handle, looped
