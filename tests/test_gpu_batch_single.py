"""GPU: predict_batch of a min_clusters=1 clusterer as ONE `sc_predict_batch_single` call -- the
single-cluster test of every utterance as group-wide device work inside the grouped batch --
against per-utterance predict(): verdicts, labels, routes; what keeps the per-utterance loop; and
a MultiStageStreamPool whose main clusterer has min_clusters=1.

The batch: 70 utterances of n <= 128 and 18 of 128 < n <= 700 (more than one wave of 64, more than
one group of 16), sizes and classes of tests/_single_check_ref.py, d = 16."""

import numpy as np
import pytest
# (at module level on purpose: PyTorch has to be in the process before the library is loaded,
#  so that both use one HIP runtime -- INTEGRATION.md section 6)
import torch  # noqa: F401

import spectral_oracle as so
import _single_check_ref as ref_lib

import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import fallback_clusterer as fb
from spectralcluster_amd import multi_stage_clusterer as ms

pytestmark = pytest.mark.gpu

CONDITIONS = {
    "AffinityGmmBic": 0.75,     # (the threshold is not read)
    "AllAffinity": 0.75,
    "NeighborAffinity": 0.75,
    "AffinityStd": 0.1,
}


def icassp_options(sigma=0, p=0.95):
  return sca.RefinementOptions(gaussian_blur_sigma=sigma, p_percentile=p,
                               refinement_sequence=sca.ICASSP2018_REFINEMENT_SEQUENCE)


def make_clusterer(condition="AffinityGmmBic", offset=1, **kwargs):
  options = fb.FallbackOptions(
      single_cluster_condition=getattr(fb.SingleClusterCondition, condition),
      single_cluster_affinity_threshold=CONDITIONS.get(condition, 0.75),
      single_cluster_affinity_diagonal_offset=offset)
  return sca.SpectralClusterer(min_clusters=1, max_clusters=6,
                               refinement_options=icassp_options(sigma=1),
                               fallback_options=options, **kwargs)


def batch_cases():
  shorts = [(ref_lib.SHORT_SIZES[i % 4], ref_lib.CLASSES[(i // 4) % 3]) for i in range(70)]
  longs = [(ref_lib.CHAIN_SIZES[i % 4], ref_lib.CLASSES[(i // 4) % 3]) for i in range(18)]
  cases = shorts + longs
  order = np.random.default_rng(7).permutation(len(cases))
  return [cases[i] for i in order]


CASES = batch_cases()
UTTERANCES = [ref_lib.embeddings(n, cls) for n, cls in CASES]
_PREDICTED = {}   # (n, class) -> predict()'s labels of an utterance of several clusters


def predicted(clusterer, n, cls):
  """predict(u) of a case the single-cluster test lets through: the spectral path does not
  depend on the condition, so it is computed once per case and shared."""
  if (n, cls) not in _PREDICTED:
    labels = clusterer.predict(ref_lib.embeddings(n, cls))
    labels.setflags(write=False)
    _PREDICTED[(n, cls)] = labels
  return _PREDICTED[(n, cls)]


@pytest.mark.parametrize("condition", list(CONDITIONS))
def test_batch_equals_predict(condition):
  clusterer = make_clusterer(condition)
  got = clusterer.predict_batch(UTTERANCES)
  assert len(got) == len(CASES) == 88
  verdicts = {}
  for n, cls in set(CASES):
    verdicts[(n, cls)] = fb.check_single_cluster(clusterer.fallback_options, None,
                                                 np.array(ref_lib.case_affinity(n, cls)))
  assert clusterer.last_batch_single == [verdicts[c] for c in CASES]
  assert any(clusterer.last_batch_single) and not all(clusterer.last_batch_single)
  print(condition, "routes", clusterer.last_batch_routes)
  assert clusterer.last_batch_routes == [
      _lib.BATCH_ROUTE_GROUP_JACOBI if n <= 128 else _lib.BATCH_ROUTE_GROUP_LANCZOS
      for n, _ in CASES]
  for (n, cls), labels, one in zip(CASES, got, clusterer.last_batch_single):
    if one:
      want = np.array([0] * n)
      assert labels.dtype == want.dtype and np.array_equal(labels, want)
    else:
      assert labels.dtype == np.int64 and labels.shape == (n,)
      assert so.adjusted_rand_index(labels, predicted(clusterer, n, cls)) == 1.0, (n, cls)


def test_offset_beyond_an_utterance_raises_before_launch():
  clusterer = make_clusterer(offset=2)
  batch = [ref_lib.embeddings(64, "a"), ref_lib.embeddings(3, "b"), ref_lib.embeddings(129, "c")]
  with pytest.raises(ValueError, match=ref_lib.OFFSET_MESSAGE) as err:
    clusterer.predict_batch(batch)
  assert "(utterance 1)" in str(err.value)
  # ... and from the library itself, which checks before its first launch
  import ctypes
  handle = clusterer._handle()
  arrays = (_lib.ScArray * 3)(*[_lib.ScArray(u.ctypes.data, _lib.SC_DTYPE_F64, _lib.SC_MEM_HOST,
                                             u.shape[0], 16, 16, 1) for u in batch])
  labels = [np.full(u.shape[0], -5, dtype=np.int64) for u in batch]
  lp = (ctypes.POINTER(ctypes.c_int64) * 3)(*[_lib.as_int64_p(l) for l in labels])
  check = _lib.ScSingleCheck(_lib.SC_SINGLE_GMM_BIC, 2, 0.0)
  rc = handle.lib.sc_predict_batch_single(handle.raw, arrays, 3, clusterer.build_config(),
                                          ctypes.byref(check), lp, None, 16, None)
  assert rc == _lib.SC_ERR_INVALID and "(utterance 1)" in handle.last_error()
  assert all((l == -5).all() for l in labels)


def test_fallback_condition_and_constraints_keep_the_loop():
  """The FallbackClusterer condition (it clusters the embeddings) and a constrained batch run
  predict() per utterance, routes all 0, as before."""
  clusterer = make_clusterer("FallbackClusterer")
  got = clusterer.predict_batch(UTTERANCES)
  assert clusterer.last_batch_routes == [0] * len(CASES) and clusterer.last_batch_single is None
  for u, labels in zip(UTTERANCES, got):
    want = clusterer.predict(u)
    assert labels.dtype == want.dtype and np.array_equal(labels, want)
  clusterer = make_clusterer(constraint_options=sca.ConstraintOptions(
      constraint_name=sca.ConstraintName.AffinityIntegration, apply_before_refinement=False,
      integration_type=sca.IntegrationType.Max))
  constraints = [sca.ConstraintMatrix([0.0] * u.shape[0], 1) for u in UTTERANCES]
  got = clusterer.predict_batch(UTTERANCES, constraint_matrices=constraints)
  assert clusterer.last_batch_routes == [0] * len(CASES) and clusterer.last_batch_single is None
  for u, c, labels in zip(UTTERANCES, constraints, got):
    want = clusterer.predict(u, c)
    assert labels.dtype == want.dtype and np.array_equal(labels, want)


def test_utterances_of_4096_rows_and_more_decide_inside_the_call():
  """n >= 4096 takes route 0 inside the call: the single call's decision on the caller's handle,
  then predict()'s eigensolver and k-means for an utterance of several clusters."""
  clusterer = make_clusterer()
  batch = [so.blobs(4096, 16, 1, 6096, 0.02), so.blobs(4100, 16, 3, 7103, 0.2),
           ref_lib.embeddings(64, "b")]
  got = clusterer.predict_batch(batch)
  assert clusterer.last_batch_single == [True, False, True]
  assert clusterer.last_batch_routes == [0, 0, 2]
  for u, labels, one in zip(batch, got, clusterer.last_batch_single):
    want = clusterer.predict(u)
    assert labels.dtype == want.dtype and labels.shape == want.shape
    assert (np.array_equal(labels, want) if one else
            so.adjusted_rand_index(labels, want) == 1.0)


def test_min_clusters_2_batch_does_not_take_the_path():
  clusterer = sca.SpectralClusterer(min_clusters=2, max_clusters=6,
                                    refinement_options=icassp_options(sigma=1))
  batch = [ref_lib.embeddings(n, "c") for n in (64, 129, 300)]
  got = clusterer.predict_batch(batch)
  assert clusterer.last_batch_single is None and clusterer.last_batch_routes == [2, 1, 1]
  for u, labels in zip(batch, got):
    assert so.adjusted_rand_index(labels, clusterer.predict(u)) == 1.0


def conversation(seed, count, d=16, speakers=4, noise=0.02, run=5):
  rng = np.random.default_rng(seed)
  centres = np.linalg.qr(rng.standard_normal((d, speakers)))[0].T
  who = np.repeat(rng.integers(0, speakers, (count + run - 1) // run), run)[:count]
  return centres[who] + noise * rng.standard_normal((count, d))


def test_stream_pool_with_min_clusters_1_main_stays_pooled():
  """Four sessions stepped past U1 (and through a compression at U2): labels are those of each
  session's own MultiStageClusterer at every step, and beyond U1 rows the sessions take the
  pooled route with the grouped main call (1), not a main.predict of their own (2).

  The multi-stage constructors set the main clusterer's condition to FallbackClusterer, as the
  reference's does; that condition clusters the embeddings and keeps main.predict per session.
  A pool is covered once the application has put one of the affinity conditions back on the
  main clusterer, which is what this test does -- on the pool's and on the sessions' alike."""
  L, U1, U2, steps = 8, 24, 40, 60

  def make_main():
    options = sca.RefinementOptions(gaussian_blur_sigma=0, p_percentile=0.2,
                                    refinement_sequence=sca.ICASSP2018_REFINEMENT_SEQUENCE)
    return sca.SpectralClusterer(min_clusters=1, refinement_options=options,
                                 stop_eigenvalue=0.01)

  rows = [conversation(70 + k, steps, run=12) for k in range(4)]
  pool = ms.MultiStageStreamPool(make_main(), L=L, U1=U1, U2=U2, capacity=4)
  ref_main = make_main()
  refs = [ms.MultiStageClusterer(ref_main, L=L, U1=U1, U2=U2) for _ in range(4)]
  ids = [pool.open() for _ in range(4)]
  assert not pool._main_is_batchable()   # (the constructors' FallbackClusterer condition)
  for main in (pool.main, ref_main):
    main.fallback_options.single_cluster_condition = fb.SingleClusterCondition.AffinityGmmBic
  assert pool._main_is_batchable()
  singles = 0
  for t in range(steps):
    outs = pool.streaming_predict(ids, np.stack([rows[k][t] for k in range(4)]))
    for k, got in enumerate(outs):
      want = refs[k].streaming_predict(rows[k][t])
      assert got.dtype == want.dtype and np.array_equal(got, want), (k, t, got, want)
      singles += int(t + 1 >= L and len(np.unique(got)) == 1)
    expect = ms.ROUTE_POOLED_GROUPED if t + 1 > U1 else 0
    assert pool.last_routes == [expect] * 4, (t, pool.last_routes)
  assert singles > 0   # (the streams open with one speaker: the test did say "single")
  assert len(np.unique(outs[-1])) > 1
