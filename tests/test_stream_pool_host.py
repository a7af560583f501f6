"""Host side of the stream pool (no GPU): the label bookkeeping MultiStageClusterer and
MultiStageStreamPool share, the ABI version the additive sc_pool_* exports must not move, and
the tree cut of the agglomerative clustering on several threads under the host sanitizers."""

import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from spectralcluster_amd import _lib
from spectralcluster_amd import multi_stage_clusterer as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spectralcluster_amd", "csrc")

# A stream with U1 = 2, U2 = 4, worked by hand.  Per step: the pre-cluster labels of the cache
# rows, the main labels of the two centroids, whether the cache is compressed after the step,
# and what the stream returns under each de-flicker mode.
#   step 3  cache = rows 0 1 2; pre [0 1 0], main [1 0] -> rows [1 0 1]
#   step 4  cache = rows 0..3 = U2; pre [1 0 0 1], main [0 1] -> rows [1 0 0 1]; the cache becomes
#           the centroids, compression_labels = [1 0 0 1] (row -> centroid)
#   step 5  cache = centroid 0, centroid 1, row 4; compression_labels = [1 0 0 1 2];
#           pre [0 1 1], main [0 1] -> cache rows [0 1 1] -> rows [1 0 0 1 1]
# OrderBased renumbers by first occurrence.  Hungarian renames the ordered labels to overlap
# most with the previous output: at every step the overlap matrix has one best assignment
# (0 -> 1, 1 -> 0), so the result is the NoDeflicker labels as int32.
STEPS = [
    ([0, 1, 0], [1, 0], False, [1, 0, 1], [0, 1, 0]),
    ([1, 0, 0, 1], [0, 1], True, [1, 0, 0, 1], [0, 1, 1, 0]),
    ([0, 1, 1], [0, 1], False, [1, 0, 0, 1, 1], [0, 1, 1, 0, 0]),
]
COMPRESSION_AFTER = [None, [1, 0, 0, 1], [1, 0, 0, 1, 2]]


@pytest.mark.parametrize("deflicker", list(ms.Deflicker))
def test_bookkeeping_helper_hand_worked_chain(deflicker):
  state = types.SimpleNamespace(compression_labels=None,
                                previous_output=np.array([1, 0], dtype=np.int64))
  for (pre, main, compress, plain, ordered), comp in zip(STEPS, COMPRESSION_AFTER):
    got = ms.finish_stream_step(state, deflicker, np.array(pre, dtype=np.int64),
                                np.array(main, dtype=np.int64), compress)
    if deflicker == ms.Deflicker.OrderBased:
      want, dtype = ordered, np.float64
    elif deflicker == ms.Deflicker.Hungarian:
      want, dtype = plain, np.int32
    else:
      want, dtype = plain, np.float64      # chain_labels fills a float array, as the reference
    np.testing.assert_array_equal(got, want)
    assert got.dtype == dtype
    assert state.previous_output is got
    if comp is None:
      assert state.compression_labels is None
    else:
      np.testing.assert_array_equal(state.compression_labels, comp)


def test_multi_stage_clusterer_goes_through_the_helper(monkeypatch):
  """The per-stream class calls the shared helper (so the pool and it cannot drift): with the
  two clustering calls replaced by canned labels it returns the same hand-worked chain."""
  main = types.SimpleNamespace(max_spectral_size=None, fallback_options=types.SimpleNamespace())
  canned = iter(STEPS)
  current = {}

  def pre_cluster(self, rows):
    current["step"] = next(canned)
    assert rows.shape[0] == len(current["step"][0])
    return np.array(current["step"][0], dtype=np.int64)

  main.predict = lambda rows: (np.array(current["step"][1], dtype=np.int64)
                               if rows.shape[0] == 2 and "step" in current
                               else np.array([1, 0], dtype=np.int64)[:rows.shape[0]])
  monkeypatch.setattr(ms.MultiStageClusterer, "_pre_cluster", pre_cluster)
  monkeypatch.setattr(ms.utils, "get_cluster_centroids",
                      lambda rows, labels: np.stack([rows[np.asarray(labels) == c].mean(axis=0)
                                                     for c in range(int(max(labels)) + 1)]))
  calls = []
  real = ms.finish_stream_step
  monkeypatch.setattr(ms, "finish_stream_step",
                      lambda *a: calls.append(a[4]) or real(*a))
  clusterer = ms.MultiStageClusterer(main, L=1, U1=2, U2=4, deflicker=ms.Deflicker.Hungarian)
  outs = [clusterer.streaming_predict(np.array([float(i), 1.0])) for i in range(5)]
  assert calls == [False, True, False]
  for got, (_, _, _, plain, _) in zip(outs[2:], STEPS):
    np.testing.assert_array_equal(got, plain)
    assert got.dtype == np.int32
  assert clusterer.cache.shape == (3, 2)            # two centroids + the fifth row


def test_abi_version_is_still_9():
  header = open(os.path.join(ROOT, "include", "spectralcluster_amd.h")).read()
  assert re.search(r"^#define SC_ABI_VERSION (\d+)$", header, flags=re.M).group(1) == "11"
  assert _lib.SC_ABI_VERSION == 11
  assert _lib.load().sc_abi_version() == 11
  for name in ("sc_pool_create", "sc_pool_destroy", "sc_pool_reset", "sc_pool_rows",
               "sc_pool_append", "sc_pool_precluster", "sc_pool_centroids", "sc_pool_get",
               "sc_pool_compress"):
    assert name in _lib.PROTOTYPES and hasattr(_lib.load(), name), name


def test_tree_cut_on_threads_under_sanitizers(tmp_path):
  """tests/probes/ahc_tree_threads.cpp + ahc_tree.cpp as one host program with ASan + UBSan
  (without them where their runtime is not installed): concurrent cuts equal the
  single-threaded ones and nothing is reported."""
  cxx = shutil.which("g++")
  if cxx is None:
    pytest.fail("g++ is needed to build the host library and this program")
  base = [cxx, "-std=c++17", "-O1", "-g", "-pthread", "-I", CSRC,
          os.path.join(ROOT, "tests", "probes", "ahc_tree_threads.cpp"),
          os.path.join(CSRC, "ahc_tree.cpp")]
  exe = str(tmp_path / "ahc_tree_threads")
  sanitized = subprocess.run(
      base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe],
      capture_output=True, text=True)
  if sanitized.returncode != 0:
    assert "san" in sanitized.stderr, sanitized.stderr   # only a missing runtime is excused
    subprocess.run(base + ["-o", exe], check=True, capture_output=True, text=True)
  run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
  assert run.returncode == 0, run.stdout + run.stderr
  assert run.stdout.startswith("ok:"), run.stdout
  assert run.stderr == ""
