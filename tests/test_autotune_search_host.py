"""CPU: `sc_host_autotune_search` (csrc/autotune_search.cpp) against `AutoTune.tune` on seeded
random tables: the values evaluated, in order, the winner, its index and the narrowed state left
behind -- all as exact doubles.  No GPU."""

import copy
import ctypes

import numpy as np
import pytest

import spectralcluster_amd as sca
from spectralcluster_amd import _lib

PROXIES = (sca.AutoTuneProxy.PercentileOverNME, sca.AutoTuneProxy.PercentileSqrtOverNME)
PRESET = (0.40, 0.95, 0.05)   # configs.turntodiarize_clusterer's search
DEFAULTS = (0.60, 0.95, 0.01)  # AutoTune()'s


class Table:
  """max_delta_norm per p_percentile, drawn on first request and then fixed: the Python search
  fills it, the library's search must ask for the same keys."""

  def __init__(self, seed, quantum=None):
    self.rng = np.random.default_rng(seed)
    self.quantum = quantum
    self.values = {}

  def gap(self, p, may_draw):
    if p not in self.values:
      assert may_draw, "the library evaluated %r, AutoTune.tune did not" % p
      g = float(self.rng.uniform(0.05, 1.0))
      if self.quantum:  # few distinct values: exact ties
        g = max(self.quantum, round(g / self.quantum) * self.quantum)
      self.values[p] = g
    return self.values[p]


def python_search(at, table, fixed_ratio=None):
  """AutoTune.tune on a copy: (evaluated ps per level, best_p, best_index, last_p, state)."""
  at = copy.deepcopy(at)
  levels = []

  def evaluate_many(ps):
    levels.append([float(p) for p in ps])
    out = []
    for p in ps:
      r = fixed_ratio if fixed_ratio is not None else at.ratio(p, table.gap(float(p), True))
      out.append((r, len(out), p))  # "vectors" slot carries nothing the search reads
    return out

  grids = []
  real_range = at.get_percentile_range

  def spying_range():
    grids.append([float(p) for p in real_range()])
    return grids[-1]

  at.get_percentile_range = spying_range
  _, _, best_p = at.tune(None, evaluate_many=evaluate_many)
  # the winner's index in its level's grid: tune() keeps it to itself; recover it from the level
  # that evaluated best_p (a value is evaluated in one level only)
  best_index = None
  for grid, ps in zip(grids, levels):
    if float(best_p) in ps:
      best_index = grid.index(float(best_p))
  flat = [p for ps in levels for p in ps]
  return levels, float(best_p), best_index, flat[-1], (
      float(at.p_percentile_min), float(at.p_percentile_max), float(at.search_step))


def library_search(at, table, fixed_ratio=None, fail_at=None, may_draw=False):
  lib = _lib.load()
  state = at.to_struct()
  levels = []
  raised = []

  def evaluate(ps, count, ratios_out, user):
    del user
    vals = [float(ps[i]) for i in range(count)]
    levels.append(vals)
    if fail_at is not None and len(levels) == fail_at:
      return _lib.SC_ERR_HIP
    try:
      for i, p in enumerate(vals):
        if fixed_ratio is not None:
          ratios_out[i] = fixed_ratio
          continue
        r = ctypes.c_double(0.0)
        assert lib.sc_host_autotune_ratio(ctypes.byref(state), p, table.gap(p, may_draw),
                                          ctypes.byref(r)) == _lib.SC_OK
        ratios_out[i] = r.value
    except BaseException as exc:  # pylint: disable=broad-except
      raised.append(exc)  # (an exception cannot cross the C frames: raised again below)
      return _lib.SC_ERR_UNSUPPORTED
    return _lib.SC_OK

  best_p, last_p = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
  best_index = ctypes.c_int(-1)
  narrowed = _lib.ScAutoTune()
  before = bytes(state)
  rc = lib.sc_host_autotune_search(ctypes.byref(state), _lib.AUTOTUNE_EVALUATE(evaluate), None,
                                   ctypes.byref(best_p), ctypes.byref(best_index),
                                   ctypes.byref(last_p), ctypes.byref(narrowed))
  if raised:
    raise raised[0]
  assert bytes(state) == before  # the entry state is read only
  return rc, levels, best_p.value, best_index.value, last_p.value, narrowed


def check_same(at, seed, quantum=None, fixed_ratio=None):
  table = Table(seed, quantum)
  want_levels, want_p, want_index, want_last, want_state = python_search(at, table, fixed_ratio)
  rc, levels, best_p, best_index, last_p, narrowed = library_search(at, table, fixed_ratio)
  assert rc == _lib.SC_OK
  assert levels == want_levels  # the same doubles, in the same order, level by level
  assert best_p == want_p and best_index == want_index and last_p == want_last
  assert (narrowed.p_min, narrowed.p_max, narrowed.step) == want_state
  assert narrowed.levels == at.search_level and narrowed.proxy == at.proxy.value
  return want_levels, narrowed


def test_batch_entry_is_declared_and_refuses_null_arguments():
  lib = _lib.load()
  assert "sc_predict_batch_autotune" in _lib.PROTOTYPES
  assert lib.sc_predict_batch_autotune(None, None, None, 0, None, None, None, None, None, 16,
                                       None) == _lib.SC_ERR_INVALID


def test_struct_mirror_matches_the_header():
  assert ctypes.sizeof(_lib.ScAutoTune) == 32
  assert [f for f, _ in _lib.ScAutoTune._fields_] == ["p_min", "p_max", "step", "levels", "proxy"]
  assert _lib.ScAutoTune.levels.offset == 24 and _lib.ScAutoTune.proxy.offset == 28
  at = sca.AutoTune(0.4, 0.95, 0.05, 2, sca.AutoTuneProxy.PercentileOverNME).to_struct()
  assert (at.p_min, at.p_max, at.step, at.levels, at.proxy) == (0.4, 0.95, 0.05, 2, 1)
  assert (_lib.SC_AUTOTUNE_PERCENTILE_OVER_NME, _lib.SC_AUTOTUNE_PERCENTILE_SQRT_OVER_NME) == (
      sca.AutoTuneProxy.PercentileOverNME.value, sca.AutoTuneProxy.PercentileSqrtOverNME.value)


@pytest.mark.parametrize("proxy", PROXIES)
def test_ratio_is_autotune_ratio(proxy):
  lib = _lib.load()
  at = sca.AutoTune(proxy=proxy)
  state = at.to_struct()
  rng = np.random.default_rng(7)
  for p, g in zip(rng.uniform(0.0, 1.0, 200), rng.uniform(1e-3, 5.0, 200)):
    r = ctypes.c_double(0.0)
    assert lib.sc_host_autotune_ratio(ctypes.byref(state), p, g, ctypes.byref(r)) == _lib.SC_OK
    assert r.value == float(at.ratio(p, g))
  state.proxy = 3
  assert lib.sc_host_autotune_ratio(ctypes.byref(state), 0.5, 1.0,
                                    ctypes.byref(ctypes.c_double())) == _lib.SC_ERR_INVALID


@pytest.mark.parametrize("grid", (PRESET, DEFAULTS), ids=("preset", "defaults"))
@pytest.mark.parametrize("levels", (1, 2, 3))
@pytest.mark.parametrize("proxy", PROXIES)
def test_search_matches_tune(grid, levels, proxy):
  for seed in range(8):
    at = sca.AutoTune(grid[0], grid[1], grid[2], levels, proxy)
    evaluated, _ = check_same(at, 100 * levels + seed)
    assert len(evaluated) == levels
    assert len(evaluated[0]) == (11 if grid is PRESET else 35)


@pytest.mark.parametrize("levels", (1, 2, 3))
def test_exact_ties_first_one_wins(levels):
  for seed in range(8):  # three or four distinct gaps over a level: ties at every minimum
    check_same(sca.AutoTune(0.40, 0.95, 0.05, levels, sca.AutoTuneProxy.PercentileOverNME),
               seed, quantum=0.3)
  # every ratio equal: a level's minimum starts from infinity again, so the first value the
  # LAST level evaluates is the winner (index 0 only in the first level: a narrowed grid begins
  # with a value that has been searched)
  at = sca.AutoTune(0.60, 0.95, 0.01, levels)
  check_same(at, 0, fixed_ratio=1.0)
  rc, evaluated, best_p, best_index, _, _ = library_search(at, Table(0), fixed_ratio=1.0)
  assert rc == _lib.SC_OK and best_p == evaluated[-1][0]
  assert best_index == (0 if levels == 1 else 1)


@pytest.mark.parametrize("levels", (1, 3))
def test_one_value_grid(levels):
  # ceil(0.04 / 0.05) = 1: linspace gives [min]; the search stops after it
  at = sca.AutoTune(0.90, 0.94, 0.05, levels)
  evaluated, narrowed = check_same(at, 3)
  assert evaluated == [[0.90]]
  assert (narrowed.p_min, narrowed.p_max, narrowed.step) == (0.90, 0.94, 0.05)  # not narrowed


def test_step_below_the_minimum_stops_after_one_level():
  at = sca.AutoTune(0.90, 0.9004, 5e-5, 3)
  evaluated, _ = check_same(at, 4)
  assert len(evaluated) == 1 and len(evaluated[0]) >= 8
  # ... and a search whose halved step falls below it in the second level stops there
  at = sca.AutoTune(0.90, 0.902, 1.5e-4, 3)
  assert len(check_same(at, 5)[0]) == 2


@pytest.mark.parametrize("proxy", PROXIES)
def test_entry_state_narrowed_by_an_earlier_search(proxy):
  at = sca.AutoTune(0.40, 0.95, 0.05, 2, proxy)
  for visit in range(3):  # each search starts where the previous one left the object
    table = Table(40 + visit)
    want = python_search(at, table)
    rc, levels, best_p, best_index, last_p, narrowed = library_search(at, table)
    assert rc == _lib.SC_OK and levels == want[0]
    assert (best_p, best_index, last_p) == want[1:4]
    assert (narrowed.p_min, narrowed.p_max, narrowed.step) == want[4]
    at.p_percentile_min, at.p_percentile_max, at.search_step = want[4]
  assert at.search_step == 0.05 / 64


def test_errors_where_tune_raises():
  lib = _lib.load()
  cb = _lib.AUTOTUNE_EVALUATE(lambda ps, count, out, user: _lib.SC_OK)
  assert lib.sc_host_autotune_search(None, cb, None, None, None, None, None) == _lib.SC_ERR_INVALID
  for at in (sca.AutoTune(0.4, 0.95, 0.05, 0),     # no level: tune() has no winner to return
             sca.AutoTune(0.4, 0.95, 0.0, 1),      # ceil(inf)
             sca.AutoTune(0.95, 0.40, 0.05, 1),    # linspace of a negative count
             sca.AutoTune(0.95, 0.95, 0.05, 1)):   # an empty grid
    rc, _, _, _, _, _ = library_search(at, Table(0))
    assert rc == _lib.SC_ERR_INVALID
    with pytest.raises(Exception):
      python_search(at, Table(0))
  # every ratio NaN: no strict minimum
  rc, _, _, _, _, _ = library_search(sca.AutoTune(0.4, 0.95, 0.05, 1), Table(0),
                                     fixed_ratio=float("nan"))
  assert rc == _lib.SC_ERR_INVALID
  # the evaluator's status ends the search and is returned
  rc, levels, _, _, _, _ = library_search(sca.AutoTune(0.4, 0.95, 0.05, 3), Table(0), fail_at=2,
                                          may_draw=True)
  assert rc == _lib.SC_ERR_HIP and len(levels) == 2
