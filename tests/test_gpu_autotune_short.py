"""GPU: one AutoTune level of a short utterance (n <= 128) as (matrix, p) pairs --
`sc_eig_ncluster_sweep` runs ONE front launch (k_short_sweep_front) and ONE Jacobi launch for the
level instead of a whole single call per value.

  * per value the sweep reports what `_eig_resident(p)` reports: the same number of clusters, the
    eigenvalues and the largest eigengap within 1e-10 relative, the dense Jacobi path;
  * the front staged for every pair (`sc_stage_front`, route SHORT_SWEEP) is the oracle's chain
    on the device's own affinity: cut vector and refined matrix bit for bit (tests/_front_ref.py,
    through the checks of tests/test_gpu_front.py);
  * `sc_sweep_adopt` returns the winner's eigenvectors at these sizes, and the labels they give
    are those of a fresh evaluation of the winner.

Inputs: so.blobs(n, 32, 3, seed=1000 + n).  The two searches: Turn-to-Diarize (the preset, values
in 0.40 .. 0.95) and ICASSP2018 + GraphCut (max_clusters=8, values in 0.55 .. 0.95).
"""

import copy
import ctypes
import dataclasses

import numpy as np
import pytest

import spectral_oracle as so
import spectralcluster_amd as sca
from spectralcluster_amd import _lib
import test_gpu_front as tgf

pytestmark = pytest.mark.gpu

SIZES = (3, 17, 64, 96, 97, 128)
SEARCHES = ("ttd", "icassp")
RANGE = {"ttd": (0.40, 0.95), "icassp": (0.55, 0.95)}
SC_EIG_PATH_DENSE_JACOBI = 1
CUT_SHORT_FRONT = 4  # SC_FRONT_INFO_CUT_KERNEL: k_short_sweep_front


def embeddings(n):
  return so.blobs(n, 32, 3, seed=1000 + n)


def clusterer_for(search):
  if search == "ttd":
    return copy.deepcopy(sca.configs.turntodiarize_clusterer)
  return sca.SpectralClusterer(
      min_clusters=2, max_clusters=8,
      refinement_options=copy.deepcopy(sca.configs.icassp2018_refinement_options),
      laplacian_type=sca.LaplacianType.GraphCut,
      autotune=sca.AutoTune(0.55, 0.95, 0.05, 2))


def oracle_config(search):
  if search == "ttd":
    return so.turntodiarize_config(constraint_name=so.CONSTRAINT_NONE)
  return so.icassp2018_config(max_clusters=8, laplacian_type=so.LAPLACIAN_GRAPH_CUT)


def values(search, count):
  lo, hi = RANGE[search]
  return [float(p) for p in np.linspace(lo, hi, count)]


def resident(clusterer, n):
  """The utterance's affinity resident in the clusterer's handle, no constraint."""
  handle = clusterer._handle()
  clusterer._set_constraint(handle, n, None)
  clusterer._upload(handle, embeddings(n))
  return handle


def run_short_front(ocfg, x, ps):
  """tgf.run_front for route SHORT_SWEEP (that helper sizes its outputs by `ps` on route SWEEP
  only): one dict per value with the arrays sc_stage_front wrote + "info"."""
  h = _lib.default_handle()
  cfg = tgf.sc_config(ocfg)
  x = np.ascontiguousarray(x, dtype=np.float64)
  n, d = x.shape
  count = len(ps)
  xs_p = (_lib._c_double_p * 1)(_lib.as_double_p(x))
  ns = (ctypes.c_int32 * 1)(n)
  ps_arr = np.ascontiguousarray(ps, dtype=np.float64)
  outs = (_lib.ScFrontOut * count)()
  arrays = []
  for z in range(count):
    member = {name: np.full((n, n) if name in tgf.MATRICES else (n,), np.nan)
              for name in _lib.FRONT_OUTPUTS}
    for name, arr in member.items():
      setattr(outs[z], name, _lib.as_double_p(arr))
    arrays.append(member)
  h.check(h.lib.sc_stage_front(h.raw, _lib.SC_FRONT_ROUTE_SHORT_SWEEP, ctypes.byref(cfg), count,
                               ns, d, xs_p, None, _lib.as_double_p(ps_arr), outs))
  members = []
  for z in range(count):
    info = dict(zip(_lib.FRONT_INFO_NAMES, outs[z].info))
    got = {name: arr for i, (name, arr) in enumerate(arrays[z].items())
           if info["written"] >> i & 1}
    got["info"] = info
    members.append(got)
  return members


def rel(got, want):
  want = np.asarray(want, dtype=np.float64)
  return np.max(np.abs(np.asarray(got) - want) / np.maximum(np.abs(want), 1e-300), initial=0.0)


@pytest.mark.parametrize("count", (5, 20))
@pytest.mark.parametrize("search", SEARCHES)
@pytest.mark.parametrize("n", SIZES)
def test_sweep_reports_what_single_evaluations_report(n, search, count):
  clusterer = clusterer_for(search)
  handle = resident(clusterer, n)
  ps = values(search, count)
  swept = clusterer._eig_sweep(handle, ps)
  assert len(swept) == count
  for p, got in zip(ps, swept):
    want = clusterer._eig_resident(handle, p)
    print("n=%d %s p=%.4f: clusters %d/%d, max_delta %r/%r, eigenvalue rel %.3g" % (
        n, search, p, got.n_clusters_raw, want.n_clusters_raw, got.max_delta, want.max_delta,
        rel(got.eigenvalue_array(), want.eigenvalue_array())))
    assert got.n == want.n == n
    assert got.eig_path == want.eig_path == SC_EIG_PATH_DENSE_JACOBI
    assert got.n_clusters_raw == want.n_clusters_raw
    assert got.n_eigenvalues == want.n_eigenvalues
    assert rel(got.eigenvalue_array(), want.eigenvalue_array()) <= 1e-10
    assert rel([got.max_delta], [want.max_delta]) <= 1e-10
    assert got.eig_descending == want.eig_descending
    assert got.symmetry_state == want.symmetry_state
    assert got.diffuse_path == want.diffuse_path


@pytest.mark.parametrize("count", (5, 20))
@pytest.mark.parametrize("search", SEARCHES)
@pytest.mark.parametrize("n", SIZES)
def test_staged_front_of_every_pair_is_the_oracle_chain(n, search, count):
  ocfg = oracle_config(search)
  ps = values(search, count)
  members = run_short_front(ocfg, embeddings(n), ps)
  assert len(members) == count
  if search == "ttd":
    expect = {"blur_kernel": tgf.NO_BLUR, "crop_source": tgf.CROP_NONE,
              "cut_kernel": CUT_SHORT_FRONT, "diffuse_path": tgf.NONE, "free_op": 0,
              "digits_fused": 0, "folded_rownorm": 0}
  else:  # below 128 rows the single call crops and blurs with its unfused kernels
    expect = {"blur_kernel": tgf.TILE if n >= 128 else tgf.GENERIC,
              "crop_source": tgf.CROP_EPILOGUE if n >= 128 else tgf.CROP_NONE,
              "cut_kernel": CUT_SHORT_FRONT, "diffuse_path": tgf.EXPLICIT, "free_op": 0,
              "digits_fused": 0, "folded_rownorm": 1}
  for p, got in zip(ps, members):
    tgf.check_member(got, dataclasses.replace(ocfg, p_percentile=p), expect,
                     "short sweep %s n=%d p=%g" % (search, n, p))
    assert np.array_equal(got["a0"], members[0]["a0"])


def test_more_values_than_the_entry_stages_are_refused():
  with pytest.raises(_lib.UnsupportedOnDeviceError):   # one launch holds 64 pairs
    run_short_front(oracle_config("ttd"), embeddings(17), values("ttd", 65))
  with pytest.raises(_lib.UnsupportedOnDeviceError):   # not a short level
    run_short_front(oracle_config("ttd"), embeddings(200), values("ttd", 5))


@pytest.mark.parametrize("search", SEARCHES)
@pytest.mark.parametrize("n", SIZES)
def test_adopted_winner_gives_the_labels_of_a_fresh_evaluation(n, search):
  """On a tree that evaluates a short level one value at a time nothing is adoptable:
  sc_sweep_adopt returns SC_ERR_UNSUPPORTED there."""
  clusterer = clusterer_for(search)
  handle = resident(clusterer, n)
  ps = [float(p) for p in clusterer.autotune.get_percentile_range()]
  swept = clusterer._eig_sweep(handle, ps)
  ratios = [float(clusterer.autotune.ratio(p, d.max_delta)) for p, d in zip(ps, swept)]
  index = int(np.argmin(ratios))
  p = ps[index]
  diag = _lib.ScDiag()
  rc = handle.lib.sc_sweep_adopt(handle.raw, clusterer.build_config(p), index, diag)
  assert rc == _lib.SC_OK, handle.last_error()
  assert diag.n_clusters_raw == swept[index].n_clusters_raw
  assert handle.lib.sc_num_eigenvectors(handle.raw) == n  # every eigenvector, like a single call
  k = max(int(diag.n_clusters_raw), clusterer.min_clusters)
  adopted = np.empty(n, dtype=np.int64)
  handle.check(handle.lib.sc_cluster(handle.raw, clusterer.build_config(p), k,
                                     _lib.as_int64_p(adopted), diag))
  fresh_diag = clusterer._eig_resident(handle, p)
  assert int(fresh_diag.n_clusters_raw) == int(swept[index].n_clusters_raw)
  fresh = np.empty(n, dtype=np.int64)
  handle.check(handle.lib.sc_cluster(handle.raw, clusterer.build_config(p), k,
                                     _lib.as_int64_p(fresh), fresh_diag))
  assert np.array_equal(adopted, fresh), (n, search, p, adopted, fresh)
  # ... and predict() itself, which searches, adopts and clusters
  labels = clusterer_for(search).predict(embeddings(n))
  if clusterer.autotune.search_level == 1:
    assert np.array_equal(labels, fresh)
  else:
    assert labels.shape == (n,)


def test_a_level_wider_than_one_launch():
  """70 values: a launch of 64 pairs, then one of 6 in the arenas of the first -- whose values are
  no longer adoptable; the last six are."""
  n, search = 33, "ttd"
  clusterer = clusterer_for(search)
  handle = resident(clusterer, n)
  ps = values(search, 70)
  swept = clusterer._eig_sweep(handle, ps)
  for index in (0, 5, 63, 64, 69):
    want = clusterer._eig_resident(handle, ps[index])
    assert swept[index].n_clusters_raw == want.n_clusters_raw
    assert rel(swept[index].eigenvalue_array(), want.eigenvalue_array()) <= 1e-10
  # (the single evaluations above replaced nothing in the member arenas)
  diag = _lib.ScDiag()
  adopt = lambda i: handle.lib.sc_sweep_adopt(handle.raw, clusterer.build_config(ps[i]), i, diag)
  assert adopt(3) == _lib.SC_ERR_UNSUPPORTED
  assert adopt(30) == _lib.SC_OK and adopt(66) == _lib.SC_OK
