"""GPU: the verdict forms of the two linkage kernels (ahc.hip: k_batch_linkage_lds_verdict,
k_ahc_nn_chain_verdict), driven through `sc_batch_fallback_check`: "does average-linkage cosine
AHC, cut at the threshold, leave one cluster?" against scipy, bit for bit against the batched
clustering on the knife edge, and independent of what shares the call.

Sizes: 2, 3, 63, 64, 65 (the lane pair i0 / i1 of the LDS body), 127, 128 (its last sizes), 129
(the first chain member), 257, and 1025 (one more row than the chain kernel has threads).  d = 16,
dtypes mixed.  Per size one tight cluster and two far clusters."""

import ctypes

import numpy as np
import pytest
# (at module level on purpose: PyTorch has to be in the process before the library is loaded,
#  so that both use one HIP runtime -- INTEGRATION.md section 6)
import torch
from scipy.cluster.hierarchy import linkage
from scipy.spatial.distance import pdist

from spectralcluster_amd import _dlpack
from spectralcluster_amd import _lib
from spectralcluster_amd import utils

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 63, 64, 65, 127, 128, 129, 257, 1025)
THRESHOLD = 0.5
# 1e-11 absolute: a d = 16 dot product of unit rows errs below 16 * 2^-53, each of at most about
# 1025 Lance-Williams updates adds a few 2^-53 relative -- about 1e-13, two decimal orders of margin
TOL = 1e-11
DTYPES = (np.float64, np.float32, np.float16, "bfloat16")


def make_rows(n, clusters, seed, dtype):
  rng = np.random.default_rng(seed)
  centres = np.linalg.qr(rng.standard_normal((16, 4)))[0].T[:clusters]
  x = centres[np.arange(n) % clusters] + 0.02 * rng.standard_normal((n, 16))
  if dtype == "bfloat16":
    return torch.from_numpy(x).to(torch.bfloat16)
  return np.ascontiguousarray(x.astype(dtype))


def widened(x):
  if isinstance(x, torch.Tensor):
    return x.to(torch.float64).numpy()
  return x.astype(np.float64)


def build_members():
  members = []
  for i, n in enumerate(SIZES):
    for clusters in (1, 2):
      members.append(make_rows(n, clusters, 100 * n + clusters, DTYPES[(2 * i + clusters) % 4]))
  order = np.random.default_rng(3).permutation(len(members))
  return [members[i] for i in order]


MEMBERS = build_members()
# the reference, once: the largest merge height of every member's tree
REF_MAX = np.array([linkage(pdist(widened(x), "cosine"), "average")[:, 2].max() for x in MEMBERS])
REF_SINGLE = ~(REF_MAX >= THRESHOLD)


def raw_check(members, threshold, heights, single):
  """sc_batch_fallback_check into the caller's (pre-filled) outputs; returns (rc, message)."""
  handle = _lib.default_handle()
  sources = [_dlpack.describe(x, lambda: handle) for x in members]
  try:
    count = len(sources)
    rc = handle.lib.sc_batch_fallback_check(
        handle.raw, (_lib.ScArray * count)(*[s.array for s in sources]), count, float(threshold),
        _lib.as_double_p(heights), single.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
  finally:
    for s in sources:
      s.release()
  return rc, handle.last_error()


@pytest.fixture(scope="module")
def mixed():
  """The mixed batch's records (single, heights), computed once."""
  # both verdicts occur, and no reference maximum is near the threshold (asserted on the CPU,
  # before the GPU is touched)
  assert REF_SINGLE.any() and not REF_SINGLE.all()
  assert np.abs(REF_MAX - THRESHOLD).min() >= 1e-6
  heights = np.full(len(MEMBERS), np.nan)
  single = np.full(len(MEMBERS), -5, dtype=np.int32)
  rc, message = raw_check(MEMBERS, THRESHOLD, heights, single)
  assert rc == _lib.SC_OK, message
  assert set(single.tolist()) <= {0, 1} and np.isfinite(heights).all()
  return single.astype(bool), heights


def test_verdicts_and_heights_against_scipy(mixed):
  single, heights = mixed
  for x, one, h, ref in zip(MEMBERS, single, heights, REF_MAX):
    print("n=%d dtype=%s single=%s height=%.17g scipy max=%.17g diff=%.3g" % (
        x.shape[0], x.dtype, one, h, ref, h - ref))
  assert np.array_equal(single, REF_SINGLE)
  # one cluster: the largest merge height; several: the height that settled it
  assert np.abs(heights[single] - REF_MAX[single]).max() <= TOL
  assert (heights[~single] >= THRESHOLD).all()
  assert (heights[~single] <= REF_MAX[~single] + TOL).all()


def test_knife_edge_is_the_batched_clusterings(mixed):
  """threshold = h: `>=` says several; the next double above h: one -- both times what
  sc_batch_ahc's labels say for the same array."""
  single, heights = mixed
  for x, one, h in zip(MEMBERS, single, heights):
    if not one:
      continue
    for threshold, want in ((h, False), (np.nextafter(h, 2.0), True)):
      got, _ = utils.cosine_single_cluster_check_batch([x], threshold)
      labels = utils.cosine_agglomerative_clustering_batch(
          [x], linkage="average", distance_threshold=threshold)[0]
      assert bool(got[0]) == want, (x.shape[0], threshold)
      assert bool(got[0]) == (len(np.unique(labels)) == 1), (x.shape[0], threshold)


def test_a_record_does_not_depend_on_what_shares_the_call(mixed):
  single, heights = mixed
  for x, one, h in zip(MEMBERS, single, heights):
    alone, alone_h = utils.cosine_single_cluster_check_batch([x], THRESHOLD)
    assert bool(alone[0]) == bool(one) and alone_h[0] == h, (x.shape[0], alone_h[0], h)


def test_waves_of_a_small_budget_give_the_same_records(mixed):
  """12 MB a wave: the 1025-row member (8.4 MB of distances) fills one, the rest follow."""
  single, heights = mixed
  handle = _lib.default_handle()
  handle.check(handle.lib.sc_set_reduce_wave_bytes(handle.raw, 12 << 20))
  try:
    got, got_h = utils.cosine_single_cluster_check_batch(MEMBERS, THRESHOLD)
  finally:
    handle.check(handle.lib.sc_set_reduce_wave_bytes(handle.raw, 0))
  assert np.array_equal(got, single) and np.array_equal(got_h, heights)


def test_a_zero_row_names_the_utterance_and_leaves_the_outputs():
  bad = make_rows(65, 2, 5, np.float32)
  bad[17] = 0.0
  batch = [make_rows(129, 1, 6, np.float64), bad, make_rows(3, 1, 7, np.float64)]
  heights = np.full(3, np.nan)
  single = np.full(3, -5, dtype=np.int32)
  rc, message = raw_check(batch, THRESHOLD, heights, single)
  assert rc == _lib.SC_ERR_INVALID and "utterance 1" in message, message
  assert np.isnan(heights).all() and (single == -5).all()
  with pytest.raises(ValueError, match="utterance 1"):
    utils.cosine_single_cluster_check_batch(batch, THRESHOLD)
  # a member of one row: refused before anything is launched
  rc, message = raw_check([batch[0], np.ones((1, 16))], THRESHOLD, heights[:2], single[:2])
  assert rc == _lib.SC_ERR_INVALID and "utterance 1" in message and "1 sample" in message
  assert np.isnan(heights).all() and (single == -5).all()
  # NULL outputs: an error code, no crash
  handle = _lib.default_handle()
  src = _dlpack.describe(batch[0], lambda: handle)
  assert handle.lib.sc_batch_fallback_check(handle.raw, (_lib.ScArray * 1)(src.array), 1,
                                            THRESHOLD, None, None) == _lib.SC_ERR_INVALID
  src.release()
