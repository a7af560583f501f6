"""GPU: predict_batch(batch_multi_stage=True) -- `fallback_options.spectral_min_embeddings`,
`max_spectral_size` and `min_clusters=1` together as ONE `sc_predict_batch_multi_stage` call --
against per-utterance predict() on the same clusterer, for the five single-cluster conditions and
both fallback types: labels and their dtypes, kinds, verdicts, routes, diags; the input forms; a
batch of one; a size-reduced member of 4096 rows; at least three waves per stage; and the call
against its sibling calls where they cover the same batch.

The batch, d = 16, spectral_min_embeddings = 40: 100 utterances of n in {1, 2, 20, 39} (fallback),
{40, 64, 128} (66 of them), {129, 200}, {201, 260, 700}, of one noisy speaker, one tight speaker
and 2, 3 and 4 speakers (the one- and three-speaker classes are tests/_single_check_ref.py's).
With max_spectral_size = 200 the sub-batch holds 66 members of the short route and 25 of the
lockstep groups (waves of 64 and groups of 16 wrap) and the centroids take route 1; with 100 all
centroids take route 2."""

import ctypes

import numpy as np
import pytest
# (at module level on purpose: PyTorch has to be in the process before the library is loaded,
#  so that both use one HIP runtime -- INTEGRATION.md section 6)
import torch

import spectral_oracle as so
import _single_check_ref as ref_lib

import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import fallback_clusterer as fb

pytestmark = pytest.mark.gpu

MIN_EMBEDDINGS = 40
CONDITIONS = {   # single_cluster_affinity_threshold (tests/test_gpu_batch_single.py's)
    "AffinityGmmBic": 0.75,   # (not read)
    "AllAffinity": 0.75,
    "NeighborAffinity": 0.75,
    "AffinityStd": 0.1,
    "FallbackClusterer": 0.75,   # (not read)
}
FALLBACK_TYPES = ("Agglomerative", "Naive")
CONFIGS = [(c, t) for c in CONDITIONS for t in FALLBACK_TYPES]
CLASSES = ("a", "b", "c", "s2", "s4")


def embeddings(n, cls):
  if cls in ref_lib.CLASSES:
    return ref_lib.embeddings(n, cls)
  k = int(cls[1])
  return so.blobs(n, 16, k, 3000 + n + k, 0.2)


def batch_cases():
  def cycle(sizes, count, shift):
    return [(sizes[i % len(sizes)], CLASSES[(i // len(sizes) + shift) % 5]) for i in range(count)]
  cases = (cycle((2, 20, 39), 9, 0) + cycle((40, 64, 128), 66, 1) + cycle((129, 200), 10, 2) +
           cycle((201, 260, 700), 15, 0))
  order = np.random.default_rng(11).permutation(len(cases))
  return [cases[i] for i in order]


CASES = batch_cases()
UTTERANCES = [embeddings(n, cls) for n, cls in CASES]
ONE_ROW = embeddings(1, "a")   # a fallback utterance of one row: the Naive type alone takes it


def make_clusterer(condition, fallback_type, mss, min_embeddings=MIN_EMBEDDINGS):
  options = fb.FallbackOptions(
      spectral_min_embeddings=min_embeddings,
      single_cluster_condition=getattr(fb.SingleClusterCondition, condition),
      single_cluster_affinity_threshold=CONDITIONS[condition],
      single_cluster_affinity_diagonal_offset=1,
      fallback_clusterer_type=getattr(fb.FallbackClustererType, fallback_type),
      agglomerative_threshold=0.5, naive_threshold=0.5)
  refinement = sca.RefinementOptions(gaussian_blur_sigma=1, p_percentile=0.95,
                                     refinement_sequence=sca.ICASSP2018_REFINEMENT_SEQUENCE)
  return sca.SpectralClusterer(min_clusters=1, max_clusters=6, refinement_options=refinement,
                               fallback_options=options, max_spectral_size=mss)


def diag_is_zeroed(diag):
  return bytes(diag) == b"\0" * ctypes.sizeof(_lib.ScDiag)


def reference_verdict(clusterer, u):
  """predict()'s single-cluster decision for `u`, in its order: None for a fallback utterance;
  for a size-reduced one the test runs on the centroids."""
  kind = clusterer._batch_kind(u.shape[0])
  if kind == _lib.BATCH_KIND_FALLBACK:
    return None
  if kind == _lib.BATCH_KIND_REDUCED:
    pre = sca.utils.cosine_agglomerative_clustering(
        u, n_clusters=clusterer.max_spectral_size, linkage="complete")
    u = sca.utils.get_cluster_centroids(u, pre)
  options = clusterer.fallback_options
  if options.single_cluster_condition == fb.SingleClusterCondition.FallbackClusterer:
    return fb.check_single_cluster(options, u, None)
  return fb.check_single_cluster(options, None, so.affinity(u))


def expected_route(clusterer, n, one):
  kind = clusterer._batch_kind(n)
  if kind == _lib.BATCH_KIND_FALLBACK:
    return _lib.BATCH_ROUTE_FALLBACK
  by_fallback = (clusterer.fallback_options.single_cluster_condition ==
                 fb.SingleClusterCondition.FallbackClusterer)
  if one and by_fallback:
    return _lib.BATCH_ROUTE_FALLBACK
  rows = clusterer.max_spectral_size if kind == _lib.BATCH_KIND_REDUCED else n
  if rows >= 4096:
    return _lib.BATCH_ROUTE_SINGLE
  return _lib.BATCH_ROUTE_GROUP_JACOBI if rows <= 128 else _lib.BATCH_ROUTE_GROUP_LANCZOS


def check_against_predict(clusterer, cases, utterances, got):
  """Every report of the call, and the labels against predict() (computed once per case)."""
  assert len(got) == len(cases)
  want, verdict = {}, {}
  for case, u in zip(cases, utterances):
    if case not in want:
      want[case] = clusterer.predict(u)
      verdict[case] = reference_verdict(clusterer, u)
  assert clusterer.last_batch_reduced == [clusterer._batch_kind(n) for n, _ in cases]
  assert clusterer.last_batch_single == [verdict[c] for c in cases]
  assert clusterer.last_batch_routes == [
      expected_route(clusterer, n, one) for (n, _), one in zip(cases, clusterer.last_batch_single)]
  differ = []
  for case, labels, kind, one, diag in zip(cases, got, clusterer.last_batch_reduced,
                                           clusterer.last_batch_single,
                                           clusterer.last_batch_diags):
    w = want[case]
    assert diag_is_zeroed(diag) == (kind == _lib.BATCH_KIND_FALLBACK or bool(one)), case
    assert labels.dtype == w.dtype and labels.shape == w.shape, (case, labels.dtype, w.dtype)
    assert w.dtype == (np.float64 if kind == _lib.BATCH_KIND_REDUCED else np.int64), case
    if one:
      assert not labels.any(), case
    if not np.array_equal(labels, w):
      differ.append((case, so.adjusted_rand_index(labels, w)))
  print("labels that differ from predict(): (case, ARI)", differ)
  assert differ == []


@pytest.mark.parametrize("mss", [100, 200])
@pytest.mark.parametrize("condition,fallback_type", CONFIGS)
def test_batch_equals_predict(condition, fallback_type, mss):
  clusterer = make_clusterer(condition, fallback_type, mss)
  cases, utterances = list(CASES), list(UTTERANCES)
  if fallback_type == "Naive":
    cases.insert(5, (1, "a"))
    utterances.insert(5, ONE_ROW)
  got = clusterer.predict_batch(utterances, batch_multi_stage=True)
  check_against_predict(clusterer, cases, utterances, got)
  kinds, single = clusterer.last_batch_reduced, clusterer.last_batch_single
  # one-speaker and several-speaker members in each kind; both verdicts occur
  for kind in range(3):
    classes = {cls for (_, cls), k in zip(cases, kinds) if k == kind}
    assert classes >= {"a", "b", "c"}, (kind, classes)
    verdicts = {one for k, one in zip(kinds, single) if k == kind}
    assert verdicts == ({None} if kind == _lib.BATCH_KIND_FALLBACK else {True, False}), kind
  routes = [r for k, r in zip(kinds, clusterer.last_batch_routes) if k == _lib.BATCH_KIND_REDUCED]
  if condition != "FallbackClusterer":   # the centroids' route: 2 at 100, 1 at 200
    assert set(routes) == {2 if mss == 100 else 1}
  # without the flag: the loop, as before
  clusterer.predict_batch(utterances[:4])
  assert clusterer.last_batch_routes == [0] * 4 and clusterer.last_batch_single is None


SMALL = [(20, "c"), (39, "a"), (40, "b"), (64, "c"), (128, "a"), (129, "s2"), (200, "b"),
         (201, "c"), (260, "b"), (2, "b")]


@pytest.mark.parametrize("condition,fallback_type", CONFIGS)
def test_input_forms_and_a_batch_of_one(condition, fallback_type):
  """The same values (fp16-representable) as NumPy float64, NumPy float32, device float32, device
  float16 and a strided device view: the same labels, dtypes and reports.  Then utterances of each
  kind as batches of one against predict()."""
  clusterer = make_clusterer(condition, fallback_type, 200)
  half = [torch.tensor(embeddings(n, cls), dtype=torch.float16, device="cuda") for n, cls in SMALL]
  wide = [torch.zeros((2 * t.shape[0], 24), dtype=torch.float32, device="cuda") for t in half]
  for w, t in zip(wide, half):
    w[::2, 3:19] = t.float()
  forms = {
      "numpy float64": [t.cpu().numpy().astype(np.float64) for t in half],
      "numpy float32": [t.cpu().numpy().astype(np.float32) for t in half],
      "device float32": [t.float() for t in half],
      "device float16": half,
      "device strided view": [w[::2, 3:19] for w in wide],
  }
  assert not forms["device strided view"][0].is_contiguous()
  want = clusterer.predict_batch(forms["numpy float64"], batch_multi_stage=True)
  check_against_predict(clusterer, SMALL, forms["numpy float64"], want)
  report = (clusterer.last_batch_reduced, clusterer.last_batch_single,
            clusterer.last_batch_routes)
  for name, batch in forms.items():
    got = clusterer.predict_batch(batch, batch_multi_stage=True)
    assert (clusterer.last_batch_reduced, clusterer.last_batch_single,
            clusterer.last_batch_routes) == report, name
    for a, b in zip(got, want):
      assert a.dtype == b.dtype and np.array_equal(a, b), name
  for i in (0, 2, 5, 7):   # fallback, short route, lockstep group, size-reduced
    for batch in (forms["numpy float64"], forms["device float32"]):
      got = clusterer.predict_batch([batch[i]], batch_multi_stage=True)
      assert len(got) == 1 and got[0].dtype == want[i].dtype and np.array_equal(got[0], want[i])
      assert clusterer.last_batch_reduced == [report[0][i]]
      assert clusterer.last_batch_single == [report[1][i]]
      assert clusterer.last_batch_routes == [report[2][i]]


@pytest.mark.parametrize("condition,fallback_type", CONFIGS)
def test_a_size_reduced_member_of_4096_rows(condition, fallback_type):
  """n = 4096: the pre-clustering takes sc_ahc's own path inside the call; its 200 centroids are
  tested and clustered as any others."""
  clusterer = make_clusterer(condition, fallback_type, 200)
  for u in (so.blobs(4096, 16, 3, 7099, 0.2), so.blobs(4096, 16, 1, 6096, 0.02)):
    got = clusterer.predict_batch([u], batch_multi_stage=True)
    check_against_predict(clusterer, [(4096, "x")], [u], got)
    assert clusterer.last_batch_reduced == [_lib.BATCH_KIND_REDUCED]


@pytest.mark.parametrize("condition,fallback_type", CONFIGS)
def test_three_waves_and_more_per_stage(condition, fallback_type):
  """A wave budget of 1.5 MB.  Stage A: a 700-row member (3.9 MB of distances) alone exceeds it
  and takes sc_ahc's own path, the ten of 201 / 260 rows (0.4 / 0.65 MB each) go two or three to
  a wave, the fallback members share another.  The verdict stage of the FallbackClusterer
  condition: 91 members, those of 200 rows 0.4 MB each -- three to a wave.  Nothing changes."""
  clusterer = make_clusterer(condition, fallback_type, 200)
  want = clusterer.predict_batch(UTTERANCES, batch_multi_stage=True)
  report = (clusterer.last_batch_reduced, clusterer.last_batch_single,
            clusterer.last_batch_routes)
  handle = clusterer._handle()
  handle.check(handle.lib.sc_set_reduce_wave_bytes(handle.raw, 3 << 19))
  try:
    got = clusterer.predict_batch(UTTERANCES, batch_multi_stage=True)
  finally:
    handle.check(handle.lib.sc_set_reduce_wave_bytes(handle.raw, 0))
  assert (clusterer.last_batch_reduced, clusterer.last_batch_single,
          clusterer.last_batch_routes) == report
  for a, b in zip(got, want):
    assert a.dtype == b.dtype and np.array_equal(a, b)


# ---- the library call against its siblings ------------------------------------------------

def describe(batch):
  return (_lib.ScArray * len(batch))(*[
      _lib.ScArray(u.ctypes.data, _lib.SC_DTYPE_F64, _lib.SC_MEM_HOST, u.shape[0], 16, 16, 1)
      for u in batch])


class Outputs:
  def __init__(self, batch):
    count = len(batch)
    self.labels = [np.full(u.shape[0], -5, dtype=np.int64) for u in batch]
    self.lp = (ctypes.POINTER(ctypes.c_int64) * count)(*[_lib.as_int64_p(l) for l in self.labels])
    self.diags = (_lib.ScDiag * count)()
    self.kinds = (ctypes.c_int32 * count)()
    self.single = (ctypes.c_int32 * count)()
    self.routes = (ctypes.c_int32 * count)()

  def report(self, handle):
    handle.check(handle.lib.sc_last_batch_routes(handle.raw, self.routes, len(self.labels)))
    return self

  def same_as(self, other, single=True):
    assert all(a.tobytes() == b.tobytes() for a, b in zip(self.labels, other.labels))
    assert list(self.routes) == list(other.routes)
    if single:
      assert list(self.single) == list(other.single)
    for a, b in zip(self.diags, other.diags):
      assert (a.n, a.n_clusters_raw, a.n_clusters, a.eig_path, a.n_eigenvalues) == (
          b.n, b.n_clusters_raw, b.n_clusters, b.eig_path, b.n_eigenvalues)
      assert bytes(a.eigenvalues) == bytes(b.eigenvalues) and a.max_delta == b.max_delta


def stage_of(clusterer, **fields):
  stage = clusterer._multi_stage_struct()
  for name, value in fields.items():
    setattr(stage, name, value)
  return stage


@pytest.mark.parametrize("fallback_type", FALLBACK_TYPES)
def test_without_a_test_the_call_is_the_reduced_call(fallback_type):
  clusterer = make_clusterer("AffinityGmmBic", fallback_type, 200)
  handle, cfg = clusterer._handle(), clusterer.build_config()
  batch = UTTERANCES + ([ONE_ROW] if fallback_type == "Naive" else [])
  arrays, count = describe(batch), len(batch)
  a, b = Outputs(batch), Outputs(batch)
  stage = stage_of(clusterer, single_condition=0)
  handle.check(handle.lib.sc_predict_batch_multi_stage(
      handle.raw, arrays, count, cfg, ctypes.byref(stage), a.lp, a.diags, 16, a.kinds, a.single))
  a.report(handle)
  if fallback_type == "Naive":
    handle.check(handle.lib.sc_predict_batch_reduced_naive(
        handle.raw, arrays, count, cfg, 200, MIN_EMBEDDINGS, 0.5, 0.5, b.lp, b.diags, 16,
        b.kinds))
  else:
    handle.check(handle.lib.sc_predict_batch_reduced(
        handle.raw, arrays, count, cfg, 200, MIN_EMBEDDINGS, 0.5, b.lp, b.diags, 16, b.kinds))
  b.report(handle)
  a.same_as(b, single=False)
  assert list(a.kinds) == list(b.kinds) == [clusterer._batch_kind(u.shape[0]) for u in batch]
  assert list(a.single) == [-1 if k == _lib.BATCH_KIND_FALLBACK else 0 for k in a.kinds]


@pytest.mark.parametrize("condition,fallback_type", CONFIGS)
def test_with_neither_size_option_the_call_is_the_single_call(condition, fallback_type):
  clusterer = make_clusterer(condition, fallback_type, 200)
  handle, cfg = clusterer._handle(), clusterer.build_config()
  batch = [u for u in UTTERANCES if u.shape[0] >= 20]
  arrays, count = describe(batch), len(batch)
  a, b = Outputs(batch), Outputs(batch)
  stage = stage_of(clusterer, max_spectral_size=0, spectral_min_embeddings=1)
  handle.check(handle.lib.sc_predict_batch_multi_stage(
      handle.raw, arrays, count, cfg, ctypes.byref(stage), a.lp, a.diags, 16, a.kinds, a.single))
  a.report(handle)
  if condition != "FallbackClusterer":
    check = clusterer._single_check_struct()
    handle.check(handle.lib.sc_predict_batch_single(
        handle.raw, arrays, count, cfg, ctypes.byref(check), b.lp, b.diags, 16, b.single))
  elif fallback_type == "Naive":
    handle.check(handle.lib.sc_predict_batch_single_naive(
        handle.raw, arrays, count, cfg, 0.5, 0.5, b.lp, b.diags, 16, b.single))
  else:
    handle.check(handle.lib.sc_predict_batch_single_fallback(
        handle.raw, arrays, count, cfg, 0.5, b.lp, b.diags, 16, b.single))
  b.report(handle)
  a.same_as(b)
  assert set(a.kinds) == {0} and set(a.single) == {0, 1}


def test_the_library_refuses_before_its_first_launch_and_names_the_utterance():
  clusterer = make_clusterer("AffinityGmmBic", "Agglomerative", 200)
  handle, cfg = clusterer._handle(), clusterer.build_config()
  batch = [embeddings(64, "a"), embeddings(260, "c"), embeddings(1, "a"), embeddings(41, "b")]
  arrays = describe(batch)

  def refused(message, **fields):
    out = Outputs(batch)
    stage = stage_of(clusterer, **fields)
    rc = handle.lib.sc_predict_batch_multi_stage(
        handle.raw, arrays, 4, cfg, ctypes.byref(stage), out.lp, out.diags,
        fields.pop("group", 16), out.kinds, out.single)
    assert rc == _lib.SC_ERR_INVALID and message in handle.last_error(), handle.last_error()
    assert all((l == -5).all() for l in out.labels)

  refused("utterance 2: Found array with 1 sample")   # an agglomerative fallback member
  # the offset against the tested rows: the 50 centroids of utterance 0 (its 64 rows would pass),
  # the rows of utterance 3; the fallback utterance 2 is not tested
  refused("(utterance 0)", spectral_min_embeddings=2, diagonal_offset=49, max_spectral_size=50)
  # (of one row: the Naive type takes it)
  refused("(utterance 3)", spectral_min_embeddings=2, diagonal_offset=40, max_spectral_size=0,
          fallback_type=2, naive_threshold=0.5, naive_adaptation_threshold=0.5)
  # under the FallbackClusterer condition a tested utterance of one row
  refused("utterance 2: Found array with 1 sample", spectral_min_embeddings=1, single_condition=5)
  refused("relatively big number", max_spectral_size=1, spectral_min_embeddings=1)
  refused("must not be below spectral_min_embeddings", max_spectral_size=30)
  refused("adaptation_threshold cannot be smaller", fallback_type=2, naive_threshold=0.5,
          naive_adaptation_threshold=0.4)
  refused("fallback_type", fallback_type=3)
  refused("single_condition", single_condition=6)
  out = Outputs(batch)
  stage = stage_of(clusterer)
  assert handle.lib.sc_predict_batch_multi_stage(
      handle.raw, arrays, 4, cfg, ctypes.byref(stage), out.lp, out.diags, 1, out.kinds,
      out.single) == _lib.SC_ERR_INVALID
  assert "grouped form" in handle.last_error()
