"""GPU: predict_batch(batch_fallback_condition=True) of a min_clusters=1 clusterer under the
FallbackClusterer condition as ONE `sc_predict_batch_single_fallback` call -- the verdicts of the
whole batch on the device, then one grouped batch of the utterances of several clusters -- against
per-utterance predict(): verdicts, labels, routes, diags; utterances of 4096 rows and more; device
inputs; and a MultiStageStreamPool built with pool_fallback_condition=True, its main clusterer's
condition left as the constructor set it.

The batch: 70 utterances of n <= 128 and 18 of 128 < n <= 700, sizes, classes and order of
tests/test_gpu_batch_single.py (tests/_single_check_ref.py), d = 16."""

import ctypes

import numpy as np
import pytest
# (at module level on purpose: PyTorch has to be in the process before the library is loaded,
#  so that both use one HIP runtime -- INTEGRATION.md section 6)
import torch
from scipy.cluster.hierarchy import linkage
from scipy.spatial.distance import pdist

import spectral_oracle as so
import _single_check_ref as ref_lib

import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import fallback_clusterer as fb
from spectralcluster_amd import multi_stage_clusterer as ms

pytestmark = pytest.mark.gpu


def batch_cases():
  shorts = [(ref_lib.SHORT_SIZES[i % 4], ref_lib.CLASSES[(i // 4) % 3]) for i in range(70)]
  longs = [(ref_lib.CHAIN_SIZES[i % 4], ref_lib.CLASSES[(i // 4) % 3]) for i in range(18)]
  cases = shorts + longs
  order = np.random.default_rng(7).permutation(len(cases))
  return [cases[i] for i in order]


CASES = batch_cases()
UTTERANCES = [ref_lib.embeddings(n, cls) for n, cls in CASES]


def chosen_threshold():
  """The middle of the widest gap between the cases' largest merge heights (scipy, on the CPU):
  both verdicts occur, and none is near the threshold."""
  tops = sorted(linkage(pdist(ref_lib.embeddings(n, cls), "cosine"), "average")[:, 2].max()
                for n, cls in set(CASES))
  gap, at = max((b - a, i) for i, (a, b) in enumerate(zip(tops, tops[1:])))
  assert gap >= 1e-3
  return 0.5 * (tops[at] + tops[at + 1])


THRESHOLD = chosen_threshold()


def make_clusterer(threshold=THRESHOLD, **kwargs):
  options = fb.FallbackOptions(
      single_cluster_condition=fb.SingleClusterCondition.FallbackClusterer,
      fallback_clusterer_type=fb.FallbackClustererType.Agglomerative,
      agglomerative_threshold=threshold)
  refinement = sca.RefinementOptions(gaussian_blur_sigma=1, p_percentile=0.95,
                                     refinement_sequence=sca.ICASSP2018_REFINEMENT_SEQUENCE)
  return sca.SpectralClusterer(min_clusters=1, max_clusters=6, refinement_options=refinement,
                               fallback_options=options, **kwargs)


def diag_is_zeroed(diag):
  return bytes(diag) == b"\0" * ctypes.sizeof(_lib.ScDiag)


def test_batch_equals_predict():
  clusterer = make_clusterer()
  got = clusterer.predict_batch(UTTERANCES, batch_fallback_condition=True)
  assert len(got) == len(CASES) == 88
  verdicts, predicted = {}, {}
  for n, cls in set(CASES):
    u = ref_lib.embeddings(n, cls)
    verdicts[(n, cls)] = fb.check_single_cluster(clusterer.fallback_options, u, None)
    predicted[(n, cls)] = clusterer.predict(u)
  assert clusterer.last_batch_single == [verdicts[c] for c in CASES]
  assert any(clusterer.last_batch_single) and not all(clusterer.last_batch_single)
  print("threshold", THRESHOLD, "routes", clusterer.last_batch_routes)
  assert clusterer.last_batch_routes == [
      _lib.BATCH_ROUTE_FALLBACK if one else
      _lib.BATCH_ROUTE_GROUP_JACOBI if n <= 128 else _lib.BATCH_ROUTE_GROUP_LANCZOS
      for (n, _), one in zip(CASES, clusterer.last_batch_single)]
  for case, labels, one, diag in zip(CASES, got, clusterer.last_batch_single,
                                     clusterer.last_batch_diags):
    want = predicted[case]
    if one:
      assert diag_is_zeroed(diag), case
      assert np.array_equal(want, np.array([0] * case[0]))
      assert labels.dtype == want.dtype and np.array_equal(labels, want), case
    else:
      assert not diag_is_zeroed(diag), case
      assert labels.dtype == np.int64 and labels.shape == (case[0],)
      assert so.adjusted_rand_index(labels, want) == 1.0, case
  # without the flag: the loop, as before
  few = UTTERANCES[:6]
  clusterer.predict_batch(few)
  assert clusterer.last_batch_routes == [0] * 6 and clusterer.last_batch_single is None


def test_utterances_of_4096_rows_and_more_decide_inside_the_call():
  """n >= 4096: sc_ahc's own path inside the call, then route 0 for the one of several clusters."""
  clusterer = make_clusterer(threshold=0.3)
  batch = [so.blobs(4096, 16, 1, 6096, 0.02), so.blobs(4100, 16, 3, 7103, 0.2),
           ref_lib.embeddings(64, "b")]
  got = clusterer.predict_batch(batch, batch_fallback_condition=True)
  assert clusterer.last_batch_single == [True, False, True]
  assert clusterer.last_batch_routes == [3, 0, 3]
  for u, labels, one in zip(batch, got, clusterer.last_batch_single):
    want = clusterer.predict(u)
    assert labels.dtype == want.dtype and labels.shape == want.shape
    assert (np.array_equal(labels, want) if one else
            so.adjusted_rand_index(labels, want) == 1.0)


def test_device_inputs_and_rows_that_do_not_stay_resident():
  """A fp32 device tensor batch against its widened float64 NumPy twin (ingest is exact: the same
  labels and verdicts), and the same batch again under a wave budget of 256 KB: the 300-row
  utterances (0.7 MB of distances each) alone exceed it, decide on sc_ahc's own path and leave
  no rows behind, so the grouped batch ingests those tensors a second time; the others share
  small waves."""
  cases = [(n, cls) for n in (3, 64, 129, 300) for cls in ref_lib.CLASSES]
  tensors = [torch.tensor(ref_lib.embeddings(n, cls), dtype=torch.float32, device="cuda")
             for n, cls in cases]
  twins = [t.cpu().numpy().astype(np.float64) for t in tensors]
  clusterer = make_clusterer()
  want = clusterer.predict_batch(twins, batch_fallback_condition=True)
  want_single, want_routes = clusterer.last_batch_single, clusterer.last_batch_routes
  assert any(want_single) and not all(want_single)
  handle = clusterer._handle()
  for budget in (0, 256 << 10):
    handle.check(handle.lib.sc_set_reduce_wave_bytes(handle.raw, budget))
    try:
      got = clusterer.predict_batch(tensors, batch_fallback_condition=True)
    finally:
      handle.check(handle.lib.sc_set_reduce_wave_bytes(handle.raw, 0))
    assert clusterer.last_batch_single == want_single
    assert clusterer.last_batch_routes == want_routes
    for a, b in zip(got, want):
      assert a.dtype == b.dtype and np.array_equal(a, b)


def conversation(seed, count, d=16, speakers=4, noise=0.02, run=5):
  rng = np.random.default_rng(seed)
  centres = np.linalg.qr(rng.standard_normal((d, speakers)))[0].T
  who = np.repeat(rng.integers(0, speakers, (count + run - 1) // run), run)[:count]
  return centres[who] + noise * rng.standard_normal((count, d))


L, U1, U2, STEPS = 8, 24, 40, 60
ROWS = [conversation(70 + k, STEPS, run=12) for k in range(4)]


def make_main():
  options = sca.RefinementOptions(gaussian_blur_sigma=0, p_percentile=0.2,
                                  refinement_sequence=sca.ICASSP2018_REFINEMENT_SEQUENCE)
  return sca.SpectralClusterer(min_clusters=1, refinement_options=options, stop_eigenvalue=0.01)


@pytest.fixture(scope="module")
def stream_reference():
  """What four MultiStageClusterers return at every step (computed once, left unchanged)."""
  main = make_main()
  refs = [ms.MultiStageClusterer(main, L=L, U1=U1, U2=U2) for _ in range(4)]
  outs = [[refs[k].streaming_predict(ROWS[k][t]) for k in range(4)] for t in range(STEPS)]
  for step in outs:
    for labels in step:
      labels.setflags(write=False)
  return outs


@pytest.mark.parametrize("early", [False, True])
def test_stream_pool_with_the_constructors_condition_is_pooled(stream_reference, early):
  pool = ms.MultiStageStreamPool(make_main(), L=L, U1=U1, U2=U2, capacity=4,
                                 pool_early_stage=early, pool_fallback_condition=True)
  # the condition is the constructor's own
  assert (pool.main.fallback_options.single_cluster_condition ==
          fb.SingleClusterCondition.FallbackClusterer)
  assert pool._main_is_batchable()
  ids = [pool.open() for _ in range(4)]
  singles = 0
  for t in range(STEPS):
    outs = pool.streaming_predict(ids, np.stack([ROWS[k][t] for k in range(4)]))
    for k, got in enumerate(outs):
      want = stream_reference[t][k]
      assert got.dtype == want.dtype and np.array_equal(got, want), (k, t, got, want)
      singles += int(t + 1 >= L and len(np.unique(got)) == 1)
    rows = t + 1
    if rows > U1:
      expect = ms.ROUTE_POOLED_GROUPED
    elif not early or rows == 1:
      expect = ms.ROUTE_MAIN_ONLY
    else:
      expect = ms.ROUTE_EARLY_FALLBACK if rows < L else ms.ROUTE_EARLY_MAIN
    assert pool.last_routes == [expect] * 4, (t, pool.last_routes)
  assert singles > 0   # (the streams open with one speaker: some steps did say "single")
  assert len(np.unique(outs[-1])) > 1
  # the same pool without the new flag is not batchable, as before
  plain = ms.MultiStageStreamPool(make_main(), L=L, U1=U1, U2=U2, capacity=4,
                                  pool_early_stage=early)
  assert not plain._main_is_batchable()
