"""A grid of batch calls and what each of them does: which library symbols it calls with which
arguments, which utterances it loops, what it raises or returns and what it leaves in
`last_batch_*`.  `run(case)` drives one case on a fresh clusterer wired to the stand-in library of
`_batch_fake.py` (host NumPy inputs, no device, no library) and returns the outcome as one compact
JSON line; `tests/golden/batch_dispatch.json` holds the outcome of every case and
`test_batch_dispatch_host.py` replays them.

    python tests/_batch_grid.py --write     record the table from the code as it is
"""

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import spectralcluster_amd as sca  # noqa: E402
from spectralcluster_amd import _lib  # noqa: E402
from spectralcluster_amd import fallback_clusterer as fb  # noqa: E402

import _batch_fake  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "batch_dispatch.json")
CONDITIONS = ("AffinityGmmBic", "AllAffinity", "NeighborAffinity", "AffinityStd",
              "FallbackClusterer")
FALLBACK_TYPES = ("Agglomerative", "Naive")


# ------------------------------------------------------------------ clusterers
def _band_options():
  return sca.ConstraintOptions(constraint_name=sca.ConstraintName.AffinityIntegration,
                               apply_before_refinement=False,
                               integration_type=sca.IntegrationType.Max)


def _fallback(condition="AffinityGmmBic", kind="Agglomerative", low=1, offset=2, adaptation=None):
  return fb.FallbackOptions(
      spectral_min_embeddings=low,
      single_cluster_condition=getattr(fb.SingleClusterCondition, condition),
      single_cluster_affinity_threshold=0.6, single_cluster_affinity_diagonal_offset=offset,
      fallback_clusterer_type=getattr(fb.FallbackClustererType, kind),
      agglomerative_threshold=0.4, naive_threshold=0.3, naive_adaptation_threshold=adaptation)


def _autotune(threshold=True, **kwargs):
  sequence = [sca.RefinementName.RowWiseThreshold if threshold else sca.RefinementName.Symmetrize]
  return dict(autotune=sca.AutoTune(p_percentile_min=0.5, p_percentile_max=0.9,
                                    init_search_step=0.1, search_level=1),
              refinement_options=sca.RefinementOptions(refinement_sequence=sequence,
                                                       p_percentile=0.9), **kwargs)


def _clusterers():
  """name -> keyword arguments of a SpectralClusterer (built anew for every case)."""
  made = {
      "plain": lambda: {},
      "at": _autotune,
      "at_norwt": lambda: _autotune(threshold=False),
      "mss": lambda: dict(max_spectral_size=12, fallback_options=_fallback()),
      "low": lambda: dict(fallback_options=_fallback(low=5)),
      "both": lambda: dict(max_spectral_size=12, fallback_options=_fallback(low=5)),
      "both_naive": lambda: dict(max_spectral_size=12,
                                 fallback_options=_fallback(kind="Naive", low=5)),
      "both_lt": lambda: dict(max_clusters=2, max_spectral_size=4,
                              fallback_options=_fallback(low=5)),
      "m1_mss": lambda: dict(min_clusters=1, max_spectral_size=12,
                             fallback_options=_fallback("AllAffinity")),
      "m1_low": lambda: dict(min_clusters=1, fallback_options=_fallback("AllAffinity", low=5)),
      "m1_both": lambda: dict(min_clusters=1, max_spectral_size=12,
                              fallback_options=_fallback("AllAffinity", low=5)),
      "m1_both_fb": lambda: dict(min_clusters=1, max_spectral_size=12,
                                 fallback_options=_fallback("FallbackClusterer", "Naive", low=5)),
      "m1_both_gmm": lambda: dict(min_clusters=1, max_spectral_size=12,
                                  fallback_options=_fallback("AffinityGmmBic", low=2, offset=10)),
      "aff_fn": lambda: dict(affinity_function=lambda x: x),
      "km_fn": lambda: dict(post_eigen_cluster_function=lambda **kw: None),
      "euclid": lambda: dict(custom_dist="euclidean"),
      "mahal": lambda: dict(custom_dist="mahalanobis"),
      "s_euclid": lambda: dict(min_clusters=1, custom_dist="euclidean",
                               fallback_options=_fallback("AllAffinity")),
      "both_euclid": lambda: dict(max_spectral_size=12, custom_dist="euclidean",
                                  fallback_options=_fallback(low=5)),
      "c_plain": lambda: dict(constraint_options=_band_options()),
      "c_euclid": lambda: dict(constraint_options=_band_options(), custom_dist="euclidean"),
      "c_m1": lambda: dict(min_clusters=1, constraint_options=_band_options(),
                           fallback_options=_fallback("AllAffinity")),
      "c_m1_fb": lambda: dict(min_clusters=1, constraint_options=_band_options(),
                              fallback_options=_fallback("FallbackClusterer")),
      "c_at": lambda: _autotune(constraint_options=_band_options()),
      "c_both": lambda: dict(max_spectral_size=12, constraint_options=_band_options(),
                             fallback_options=_fallback(low=5)),
      # what predict() raises for an utterance
      "naive_bad": lambda: dict(max_spectral_size=12, fallback_options=_fallback(
          kind="Naive", low=5, adaptation=0.1)),
      "s_naive_bad": lambda: dict(min_clusters=1, fallback_options=_fallback(
          "FallbackClusterer", "Naive", adaptation=0.1)),
      "m1_naive_bad": lambda: dict(min_clusters=1, max_spectral_size=12, fallback_options=_fallback(
          "AllAffinity", "Naive", low=5, adaptation=0.1)),
      "mss_small": lambda: dict(max_spectral_size=4, fallback_options=_fallback()),
      "m1_mss_small": lambda: dict(min_clusters=1, max_spectral_size=4,
                                   fallback_options=_fallback("AllAffinity", low=2)),
      "gmm_off": lambda: dict(min_clusters=1, fallback_options=_fallback(offset=10)),
  }
  for condition in CONDITIONS:
    for kind in FALLBACK_TYPES:
      made["s_%s_%s" % (condition, kind)] = (
          lambda condition=condition, kind=kind: dict(
              min_clusters=1, fallback_options=_fallback(condition, kind)))
  return made


CLUSTERERS = _clusterers()


def make_clusterer(name):
  kwargs = dict(min_clusters=2, max_clusters=4)
  kwargs.update(CLUSTERERS[name]())
  return sca.SpectralClusterer(**kwargs)


# ------------------------------------------------------------------------ axes
FORMS = tuple((g, s) for g in (None, 1, 8) for s in (None, 2))
FLAG_NAMES = ("autotune_from_entry_state", "batch_fallback_condition", "batch_naive_fallback",
              "batch_multi_stage", "batch_any_metric")
FLAGS = {"none": (), "ate": FLAG_NAMES[:1], "bfc": FLAG_NAMES[1:2], "bnf": FLAG_NAMES[2:3],
         "bms": FLAG_NAMES[3:4], "bam": FLAG_NAMES[4:5], "bfc+bnf": FLAG_NAMES[1:3],
         "all": FLAG_NAMES}
CONSTRAINTS = ("none", "cm", "mix", "pair", "dense", "raw", "short", "badlen")
INPUTS = ("f64", "f32", "1d", "twod", "empty", "one", "row1")


def make_inputs(name):
  """Utterances of 4, 9 and 13 rows meet the three `BATCH_KIND_*` of a clusterer with
  max_spectral_size=12 and spectral_min_embeddings=5; 9 and 13 are "single" to the stand-in."""
  if name == "f64":
    return [np.ones((n, 3)) for n in (4, 9, 13)]
  if name == "f32":
    return [np.ones((4, 3)), np.ones((9, 3), dtype=np.float32), np.ones((13, 3))]
  if name == "1d":
    return [np.ones((4, 3)), np.ones(9)]
  if name == "twod":
    return [np.ones((4, 3)), np.ones((9, 2))]
  if name == "empty":
    return []
  if name == "one":
    return [np.ones((9, 3))]
  if name == "row1":
    return [np.ones((n, 3)) for n in (1, 9, 13)]
  raise ValueError(name)


def make_constraints(name, rows):
  if name == "none":
    return None
  band = lambda n: sca.ConstraintMatrix([0.0] * n, 1)
  other = {"mix": lambda n: None, "pair": lambda n: sca.PairwiseConstraints(n, [(0, 1)]),
           "dense": lambda n: sca.DenseConstraints(np.zeros((n, n))),
           "raw": lambda n: np.zeros((n, n))}
  out = [band(n) for n in rows]
  if name in other and len(out) > 1:
    out[1] = other[name](rows[1])
    if len(out) > 2 and name != "mix":
      out[2] = None
  if name == "short":
    out = out[:-1]
  if name == "badlen" and out:
    out[0] = band(rows[0] + 1)
  return out


def _form_id(form):
  return "g%ss%s" % tuple("-" if v is None else v for v in form)


def cases():
  """Every case: (id, method, clusterer, form, flags, constraints, inputs)."""
  out = []

  def add(method, clusterer, form=(None, None), flags="none", cons="none", inputs="f64"):
    case = (method, clusterer, form, flags, cons, inputs)
    cid = "/".join((method, clusterer, _form_id(form), flags, cons, inputs))
    if cid not in seen:
      seen.add(cid)
      out.append((cid,) + case)

  seen = set()
  names = sorted(CLUSTERERS)
  concerned = {   # the flag alone, on the clusterers whose route it decides
      "ate": ("plain", "at", "at_norwt", "c_at"),
      "bfc": ("plain", "s_FallbackClusterer_Agglomerative", "s_FallbackClusterer_Naive",
              "s_AllAffinity_Agglomerative", "s_naive_bad", "c_m1_fb"),
      "bnf": ("plain", "both_naive", "naive_bad", "both", "s_FallbackClusterer_Naive"),
      "bfc+bnf": ("s_FallbackClusterer_Agglomerative", "s_FallbackClusterer_Naive", "s_naive_bad"),
      "bms": ("plain", "both") + tuple(c for c in names if c.startswith("m1_")),
      "bam": ("plain", "euclid", "mahal", "s_euclid", "both_euclid", "c_euclid", "aff_fn"),
  }
  for c in names:                      # every clusterer without flags and under all of them
    add("batch", c)
    add("batch", c, flags="all")
  for flags, chosen in concerned.items():
    for c in chosen:
      add("batch", c, flags=flags)
  routed = ("plain", "at", "s_AllAffinity_Agglomerative", "s_FallbackClusterer_Agglomerative",
            "both", "m1_both", "euclid", "c_plain")
  for c in routed:                     # every form, every kind of input
    for form in FORMS[1:]:
      add("batch", c, form, "all")
    for inputs in INPUTS[1:]:
      add("batch", c, flags="all", inputs=inputs)
  for c in ("plain", "both", "euclid", "s_AllAffinity_Agglomerative"):
    for form in FORMS[1:]:
      add("batch", c, form)
  for inputs in INPUTS[1:]:
    add("batch", "plain", inputs=inputs)
  for c in ("both_naive", "m1_both_fb", "m1_both_gmm", "gmm_off", "mss_small", "m1_mss_small",
            "s_FallbackClusterer_Naive"):
    add("batch", c, flags="all", inputs="row1")
  for c in ("plain", "c_plain", "c_euclid", "c_m1", "c_at", "c_both"):
    for cons in CONSTRAINTS[1:]:       # every kind of constraint list
      add("batch", c, cons=cons)
      if c in ("c_plain", "c_euclid", "c_at"):
        add("batch", c, flags="all", cons=cons)
  for c in ("s_AllAffinity_Agglomerative", "s_FallbackClusterer_Agglomerative", "m1_both", "at"):
    for cons in ("cm", "short"):       # (a list without constraint_options)
      add("batch", c, flags="all", cons=cons)
  for form in ((1, None), (None, 2)):
    add("batch", "c_plain", form, cons="cm")
  add("batch", "c_plain", flags="all", cons="cm", inputs="row1")
  for c in ("plain", "c_plain", "c_euclid"):   # predict_affinity_batch
    for flags in ("none", "bam"):
      for group in (None, 1, 8):
        for cons in ("none", "cm"):
          add("affinity", c, (group, None), flags, cons)
      for cons in CONSTRAINTS[2:]:
        add("affinity", c, flags=flags, cons=cons)
  for c in ("at", "c_at", "c_m1", "euclid", "mahal", "km_fn", "aff_fn",
            "s_AllAffinity_Agglomerative", "s_FallbackClusterer_Agglomerative", "low", "mss"):
    add("affinity", c)
    add("affinity", c, flags="bam", cons="cm")
  add("affinity", "plain", inputs="empty")
  add("affinity", "plain", (0, None))
  for c in ("plain", "euclid", "mahal", "s_AllAffinity_Agglomerative", "gmm_off",
            "s_FallbackClusterer_Agglomerative", "s_FallbackClusterer_Naive", "s_naive_bad"):
    for flags in ("none", "bfc"):      # predict_device_batch
      add("device", c, (8, None), flags)
    add("device", c, (1, None), "bfc", inputs="row1")
  add("device", "plain", (16, None), inputs="f32")
  add("device", "plain", (16, None), inputs="empty")
  return out


# --------------------------------------------------------------------- running
def _runs(values):
  """[1, 1, 1, 0] -> "1*3,0" (nothing is lost: values and their order)."""
  out, values = [], list(values)
  while values:
    k = 1
    while k < len(values) and values[k] == values[0] and type(values[k]) is type(values[0]):
      k += 1
    out.append("%r*%d" % (values[0], k) if k > 1 else repr(values[0]))
    values = values[k:]
  return ",".join(out)


def _square(u):
  n = u.shape[0]
  return np.ones((n, n), dtype=u.dtype) if u.ndim == 2 else np.ones(n)


def run(case):
  """One case on a fresh clusterer -> its outcome, a JSON line with sorted keys."""
  _, method, name, form, flags, cons, inputs = case
  c = make_clusterer(name)
  handle, _ = _batch_fake.wire(None, c)
  utterances = make_inputs(inputs)
  rows = [u.shape[0] for u in utterances]
  group, streams = form
  keywords = {flag: True for flag in FLAGS[flags]}
  outcome = {}
  try:
    if method == "batch":
      got = c.predict_batch(utterances, streams, group, make_constraints(cons, rows), **keywords)
    elif method == "affinity":
      got = c.predict_affinity_batch([_square(u) for u in utterances],
                                     make_constraints(cons, rows), group, **keywords)
    else:
      utterances = [np.ascontiguousarray(u) for u in utterances]
      arrays = [_lib.ScArray(u.ctypes.data, _lib.SC_DTYPE_F64 if u.dtype == np.float64
                             else _lib.SC_DTYPE_F32, _lib.SC_MEM_HOST, u.shape[0], 3, 3, 1)
                for u in utterances]
      got = c.predict_device_batch(arrays, group, **keywords)
    outcome["res"] = ["%s:%s" % (g.dtype.str, _runs(g.tolist())) for g in got]
    outcome["routes"] = c.last_batch_routes
    outcome["single"] = c.last_batch_single
    outcome["reduced"] = c.last_batch_reduced
    diags = getattr(c, "last_batch_diags", None)
    outcome["diags"] = None if diags is None else len(diags)
    if hasattr(c, "last_batch_best_p"):
      outcome["best_p"] = c.last_batch_best_p
  except Exception as e:  # the outcome IS the exception
    outcome["exc"] = "%s: %s" % (type(e).__name__, e)
  outcome["ev"] = handle.lib.events
  if c.autotune is not None:
    outcome["p"] = c.refinement_options.p_percentile
  # (an attribute that is None is left out: a key that is absent reads "None")
  outcome = {key: value for key, value in outcome.items() if value is not None}
  return json.dumps(outcome, sort_keys=True, separators=(",", ":"))


def load_table():
  with open(TABLE) as f:
    return {cid: json.dumps(outcome, sort_keys=True, separators=(",", ":"))
            for cid, outcome in json.load(f).items()}


def write_table():
  """One case per line, sorted keys: a change of dispatch is a readable diff."""
  lines = ["%s:%s" % (json.dumps(case[0]), run(case)) for case in cases()]
  with open(TABLE, "w") as f:
    f.write("{\n" + ",\n".join(lines) + "\n}\n")
  print("%d cases, %d distinct outcomes, %d bytes" % (
      len(lines), len({l.split(":", 1)[1] for l in lines}), os.path.getsize(TABLE)))


if __name__ == "__main__":
  if "--write" in sys.argv:
    write_table()
  else:
    for case in cases():
      print(case[0], run(case))
