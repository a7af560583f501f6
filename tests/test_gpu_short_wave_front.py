"""GPU: the front of one wave of the short route of `predict_batch` (utterances of n <= 128) as ONE
chain of launches for up to 64 members -- `k_short_wave_front`, a workgroup per member, between
the grouped GEMMs -- instead of 6 to 9 launches per member.

  * every array `sc_stage_front(SHORT_WAVE)` writes for a member is bit for bit what
    `sc_stage_front(SINGLE)` writes for that member alone, and the same outputs are written;
  * the same members against the oracle's chain on the device's own affinity (the checks of
    tests/test_gpu_front.py): cut vector and refined matrix bit for bit;
  * a member's outputs do not depend on its position in the wave or on its companions, and a wave
    is at most 3 ceil(count / 16) + 3 kernel launches;
  * what the route does not cover is refused, never run another way;
  * `predict_batch` on top of it returns each member's own `predict()` -- labels and eigenvalues
    equal --, the same as with SC_SHORT_FRONT_MEMBERWISE=1 in a fresh process; d > 512 falls back;
  * a pooled streaming run (`MultiStageStreamPool`) on top of it equals the per-session class.

Sizes: reflect with n <= radius at both radii (2 .. 9), the 64-row block boundary of the
symmetrise argument order (63 .. 65, 96, 97), odd and even LDS pitch, the full matrix (127, 128).
Widths: `ldx` padding (7), no padding (16, 256), the last width of the envelope (512).
"""

import copy
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
# (PyTorch in the process before the library is loaded: one HIP runtime)
import torch  # noqa: F401

import spectral_oracle as so
import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import multi_stage_clusterer as ms
import test_gpu_front as tgf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHORT_WAVE = _lib.SC_FRONT_ROUTE_SHORT_WAVE
CUT_WAVE_FRONT = 5  # SC_FRONT_INFO_CUT_KERNEL: k_short_wave_front
SIZES = (2, 3, 5, 9, 17, 63, 64, 65, 96, 97, 127, 128)
WIDTHS = (7, 16, 256, 512)

ICASSP, TTD = tgf.ICASSP, tgf.TTD
PERCENTILE_DIFFUSE = dataclasses.replace(  # the sequence of tests/test_gpu_batch_short.py
    ICASSP, sequence=(so.OP_ROW_WISE_THRESHOLD, so.OP_SYMMETRIZE, so.OP_DIFFUSE,
                      so.OP_ROW_WISE_NORMALIZE),
    threshold_type=so.THRESHOLD_PERCENTILE, p_percentile=0.9)
CONFIGS = {
    "icassp_sigma1": ICASSP,
    "icassp_sigma2": dataclasses.replace(ICASSP, gaussian_blur_sigma=2),
    "ttd_p40": dataclasses.replace(TTD, p_percentile=0.4),
    "ttd_p95": dataclasses.replace(TTD, p_percentile=0.95),
    "percentile_diffuse": PERCENTILE_DIFFUSE,
}
for _lap in (so.LAPLACIAN_NONE, so.LAPLACIAN_AFFINITY, so.LAPLACIAN_UNNORMALIZED,
             so.LAPLACIAN_RANDOM_WALK, so.LAPLACIAN_GRAPH_CUT):
  CONFIGS["icassp_lap%d" % _lap] = dataclasses.replace(ICASSP, laplacian_type=_lap)
  # (the same five on the sequence that ends without Diffuse: the front kernel's own statistics)
  CONFIGS["ttd_lap%d" % _lap] = dataclasses.replace(TTD, p_percentile=0.7, laplacian_type=_lap)
for _name, _kw in tgf.OPTIONS.items():
  CONFIGS["option_" + _name] = dataclasses.replace(ICASSP, **_kw)


def embeddings(n, d):
  return so.blobs(n, d, 2 + n % 3, seed=100 * n + d)


def single(ocfg, x):
  return tgf.run_front(tgf.SINGLE, ocfg, xs=[x])[0]


def assert_same_front(got, want, name):
  """Every array the single call wrote, bit for bit, and nothing else written."""
  assert got["info"]["written"] == want["info"]["written"], (name, got["info"], want["info"])
  for key, arr in want.items():
    if key == "info":
      continue
    assert key in got, (name, key)
    assert np.array_equal(got[key], arr), (name, key, float(np.nanmax(np.abs(got[key] - arr))))


def expected_info(ocfg):
  diffuse = so.OP_DIFFUSE in ocfg.sequence
  return {"cut_kernel": CUT_WAVE_FRONT, "diffuse_path": tgf.EXPLICIT if diffuse else tgf.NONE,
          "free_op": 0, "digits_fused": 0,
          "folded_rownorm": int(ocfg.sequence[-1] == so.OP_ROW_WISE_NORMALIZE)}


# ------------------------------------------------- 1 + 2. the single call's bits, and the oracle
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_wave_front_is_the_single_front(config, d):
  ocfg = CONFIGS[config]
  xs = [embeddings(n, d) for n in SIZES]
  wave = tgf.run_front(SHORT_WAVE, ocfg, xs=xs)
  bound = 3 * -(-len(xs) // 16) + 3
  for n, x, got in zip(SIZES, xs, wave):
    name = "%s d=%d n=%d" % (config, d, n)
    assert_same_front(got, single(ocfg, x), name)
    assert 0 < got["info"]["launches"] <= bound, (name, got["info"])
    tgf.check_member(got, ocfg, expected_info(ocfg), name)


# ------------------------------------------------------------------------- 3. wave mechanics
MECH_SIZES = (128, 127, 97, 96, 65, 64, 63, 40, 17, 9, 5, 3, 2)
MECH_D = 24


@pytest.fixture(scope="module")
def single_fronts():
  """The single call's front of every member the mechanics cases use, computed once."""
  return {(tag, n): single(ocfg, embeddings(n, MECH_D))
          for tag, ocfg in (("icassp", ICASSP), ("ttd", CONFIGS["ttd_p95"])) for n in MECH_SIZES}


@pytest.mark.parametrize("tag", ["icassp", "ttd"])
@pytest.mark.parametrize("count", [1, 16, 17, 64])
def test_wave_mechanics(single_fronts, count, tag):
  ocfg = ICASSP if tag == "icassp" else CONFIGS["ttd_p95"]
  # mixed sizes in descending order (members repeat: the same member at several positions) ...
  descending = sorted((MECH_SIZES[i % len(MECH_SIZES)] for i in range(count)), reverse=True)
  # ... and shuffled, the first member once more at the end
  shuffled = list(np.random.default_rng(count).permutation(descending))
  shuffled[-1] = shuffled[0]
  bound = 3 * -(-count // 16) + 3
  for order in (descending, shuffled):
    wave = tgf.run_front(SHORT_WAVE, ocfg, xs=[embeddings(int(n), MECH_D) for n in order])
    assert len(wave) == count
    for z, (n, got) in enumerate(zip(order, wave)):
      name = "%s count=%d position=%d n=%d" % (tag, count, z, n)
      assert_same_front(got, single_fronts[tag, int(n)], name)
      assert got["info"]["cut_kernel"] == CUT_WAVE_FRONT, (name, got["info"])
      assert 0 < got["info"]["launches"] <= bound, (name, got["info"], bound)


# -------------------------------------------------------------------------------- 4. refusals
def test_refusals():
  ok = embeddings(40, 16)
  with pytest.raises(_lib.UnsupportedOnDeviceError):
    tgf.run_front(SHORT_WAVE, ICASSP, xs=[ok, embeddings(129, 16)])
  with pytest.raises(_lib.UnsupportedOnDeviceError):
    tgf.run_front(SHORT_WAVE, ICASSP, xs=[embeddings(40, 513)])
  outside = dataclasses.replace(ICASSP, sequence=(so.OP_ROW_WISE_THRESHOLD,
                                                  so.OP_ROW_WISE_NORMALIZE))
  with pytest.raises(_lib.UnsupportedOnDeviceError):
    tgf.run_front(SHORT_WAVE, outside, xs=[ok])
  with pytest.raises(_lib.UnsupportedOnDeviceError):
    tgf.run_front(SHORT_WAVE, ICASSP, xs=[ok] * 65)
  # ... and the handle runs the route afterwards
  got, = tgf.run_front(SHORT_WAVE, ICASSP, xs=[ok])
  assert_same_front(got, single(ICASSP, ok), "after the refusals")


# ------------------------------------------------------------------------------ 5. end to end
def clusterer(preset):
  if preset == "icassp":
    return sca.SpectralClusterer(
        min_clusters=2, max_clusters=7,
        refinement_options=copy.deepcopy(sca.configs.icassp2018_refinement_options))
  # the Turn-to-Diarize sequence and clusterer settings at one p (no search, no constraint)
  options = copy.deepcopy(sca.configs.turntodiarize_refinement_options)
  options.p_percentile = 0.9
  return sca.SpectralClusterer(min_clusters=2, max_clusters=7, refinement_options=options,
                               laplacian_type=sca.LaplacianType.GraphCut, row_wise_renorm=True)


def batch_utterances(count=2 * 64 + 5, d=16, seed=17):
  rng = np.random.default_rng(seed)
  ns = [int(n) for n in rng.integers(12, 129, count - 2)] + [128, 12]
  return [so.blobs(n, d, 2 + i % 3, seed=4000 + i) for i, n in enumerate(ns)]


_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
sys.path.insert(0, sys.argv[1] + "/oracle")
import numpy as np
import torch
import test_gpu_short_wave_front as t
c = t.clusterer(sys.argv[2])
labels = c.predict_batch(t.batch_utterances(), group=16)
out = {"routes": np.asarray(c.last_batch_routes)}
for i, lab in enumerate(labels):
  out["labels_%d" % i] = lab
  out["w_%d" % i] = c.last_batch_diags[i].eigenvalue_array()
np.savez(sys.argv[3], **out)
print("CHILD_OK")
"""


@pytest.mark.parametrize("preset", ["icassp", "ttd"])
def test_predict_batch_on_the_wave_front(tmp_path, preset):
  utts = batch_utterances()
  c = clusterer(preset)
  got = c.predict_batch(utts, group=16)
  assert c.last_batch_routes == [_lib.BATCH_ROUTE_GROUP_JACOBI] * len(utts)
  w = [d.eigenvalue_array().copy() for d in c.last_batch_diags]
  for i, u in enumerate(utts):
    want = c.predict(u)
    assert np.array_equal(got[i], want), (i, u.shape)
    assert np.array_equal(w[i], c.last_diag.eigenvalue_array()), (i, u.shape)
  again = c.predict_batch(utts, group=16)
  for i in range(len(utts)):
    assert np.array_equal(again[i], got[i]), i
    assert np.array_equal(c.last_batch_diags[i].eigenvalue_array(), w[i]), i
  # the member-by-member front, in a process of its own (the switch is read once per process)
  script, out = tmp_path / "child.py", tmp_path / "memberwise.npz"
  script.write_text(_CHILD)
  env = dict(os.environ, SC_SHORT_FRONT_MEMBERWISE="1")
  r = subprocess.run([sys.executable, str(script), ROOT, preset, str(out)], capture_output=True,
                     text=True, timeout=300, env=env)
  assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
  other = np.load(out)
  assert list(other["routes"]) == c.last_batch_routes
  for i in range(len(utts)):
    assert np.array_equal(other["labels_%d" % i], got[i]), i
    assert np.array_equal(other["w_%d" % i], w[i]), i


def test_wider_embeddings_fall_back():
  """d = 600: outside the envelope, the short route keeps its member-by-member front."""
  utts = batch_utterances(count=9, d=600, seed=23)
  c = clusterer("icassp")
  got = c.predict_batch(utts, group=16)
  assert c.last_batch_routes == [_lib.BATCH_ROUTE_GROUP_JACOBI] * len(utts)
  for i, u in enumerate(utts):
    assert np.array_equal(got[i], c.predict(u)), i
    w, w1 = c.last_batch_diags[i].eigenvalue_array(), c.last_diag.eigenvalue_array()
    assert w.shape == w1.shape and np.max(np.abs(w - w1)) <= 1e-10 * np.max(np.abs(w1)), i


def test_zero_row_raises_like_predict():
  utts = batch_utterances(count=64 + 5, seed=29)
  bad = utts[2].copy()
  bad[7] = 0.0
  c = clusterer("icassp")
  with pytest.raises(Exception) as one:
    c.predict(bad)
  with pytest.raises(type(one.value)):
    c.predict_batch(utts[:2] + [bad] + utts[3:], group=16)
  ok = c.predict_batch(utts, group=16)  # the handle and its member arenas stay usable
  assert c.last_batch_routes == [_lib.BATCH_ROUTE_GROUP_JACOBI] * len(utts)
  for i in (0, 2, 5, 68):
    assert np.array_equal(ok[i], c.predict(utts[i])), i


# ------------------------------------------------------------------------------------ 6. pool
def conversation(seed, count, d=16, speakers=4, noise=0.02, run=5):
  """The generator of tests/test_gpu_stream_pool.py."""
  rng = np.random.default_rng(seed)
  centres = np.linalg.qr(rng.standard_normal((d, speakers)))[0].T
  who = np.repeat(rng.integers(0, speakers, (count + run - 1) // run), run)[:count]
  return centres[who] + noise * rng.standard_normal((count, d))


def pool_main():
  options = sca.RefinementOptions(gaussian_blur_sigma=0, p_percentile=0.2,
                                  refinement_sequence=sca.ICASSP2018_REFINEMENT_SEQUENCE)
  return sca.SpectralClusterer(refinement_options=options, stop_eigenvalue=0.01)


def test_stream_pool_on_the_wave_front():
  L, U1, U2, sessions, steps = 10, 20, 40, 8, 110
  rows = [conversation(300 + k, steps) for k in range(sessions)]
  pool = ms.MultiStageStreamPool(pool_main(), L=L, U1=U1, U2=U2, capacity=sessions,
                                 pool_early_stage=True)
  ref_main = pool_main()
  refs = [ms.MultiStageClusterer(ref_main, L=L, U1=U1, U2=U2) for _ in range(sessions)]
  ids = [pool.open() for _ in range(sessions)]
  for t in range(steps):
    outs = pool.streaming_predict(ids, np.stack([rows[k][t] for k in range(sessions)]))
    for k, got in enumerate(outs):
      want = refs[k].streaming_predict(rows[k][t])
      assert got.dtype == want.dtype and np.array_equal(got, want), (k, t)
