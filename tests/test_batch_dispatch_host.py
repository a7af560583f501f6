"""CPU: the dispatch of predict_batch, predict_affinity_batch and predict_device_batch as a
whole.  Every case of the grid in `_batch_grid.py` is replayed on a fresh clusterer wired to the
stand-in library of `_batch_fake.py` and its outcome -- the library calls with their arguments,
the looped utterances, the exception or the results and `last_batch_*` -- is compared, as a
string, with the line `tests/golden/batch_dispatch.json` holds for it.  The table was recorded
before `spectral_clusterer.py` was split into a plan and its executors
(`python tests/_batch_grid.py --write`); a change of dispatch shows up as a diff of it.  No
device and no built library are needed."""

import json
import re

import pytest

import _batch_fake
import _batch_grid

CASES = _batch_grid.cases()
TABLE = _batch_grid.load_table()
OUTCOMES = {cid: json.loads(line) for cid, line in TABLE.items()}

FEW = ("ValueError: Found array with 1 sample(s) while a minimum of 2 is required by "
       "AgglomerativeClustering.")
BIG = "ValueError: max_spectral_size should be a relatively big number"
OFFSET = ("ValueError: single_cluster_affinity_diagonal_offset must be significantly smaller than "
          "affinity matrix dimension")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_case_does_what_the_table_says(case):
  assert _batch_grid.run(case) == TABLE[case[0]]


def test_the_table_holds_the_grid_and_nothing_else():
  ids = [c[0] for c in CASES]
  assert len(set(ids)) == len(ids) <= 2000
  assert sorted(TABLE) == sorted(ids)
  with open(_batch_grid.TABLE, "rb") as f:
    raw = f.read()
  assert len(raw) < 256 * 1024
  assert raw.count(b"\n") == len(ids) + 2  # one case per line between the braces


def _symbols(outcome):
  return [_batch_fake.PREFIX + e.split()[0] for e in outcome["ev"] if " rows=" in e]


def _looped(outcome):
  return [e for e in outcome["ev"] if re.fullmatch(r"p\d+(\+c)?", e)]


def test_every_batch_symbol_is_the_outcome_of_a_case():
  assert len(_batch_fake.BATCH_SYMBOLS) == 14
  called = {s for outcome in OUTCOMES.values() for s in _symbols(outcome)}
  assert called == set(_batch_fake.BATCH_SYMBOLS)
  # ... and a case that makes a library batch call loops nothing, and the other way round
  for cid, outcome in OUTCOMES.items():
    assert not (_symbols(outcome) and _looped(outcome)), cid


# what keeps the per-utterance loop -> (the case that loops, the neighbour that is one call, its
# symbol)
LOOPS = {
    "AutoTune without the flag": ("batch/at/g-s-/none/none/f64", "batch/at/g-s-/ate/none/f64",
                                  "autotune"),
    "a raw ndarray constraint": ("batch/c_plain/g-s-/none/raw/f64",
                                 "batch/c_plain/g-s-/none/cm/f64", "constrained"),
    "group=1": ("batch/c_plain/g1s-/none/cm/f64", "batch/c_plain/g-s-/none/cm/f64",
                "constrained"),
    "streams": ("batch/c_plain/g-s2/none/cm/f64", "batch/c_plain/g-s-/none/cm/f64",
                "constrained"),
    "group=1, min_clusters=1": ("batch/s_AllAffinity_Agglomerative/g1s-/none/none/f64",
                                "batch/s_AllAffinity_Agglomerative/g-s-/none/none/f64", "single"),
    "streams, reduced": ("batch/both/g-s2/none/none/f64", "batch/both/g-s-/none/none/f64",
                         "reduced"),
    "no batch_fallback_condition": (
        "batch/s_FallbackClusterer_Agglomerative/g-s-/none/none/f64",
        "batch/s_FallbackClusterer_Agglomerative/g-s-/bfc/none/f64", "single_fallback"),
    "no batch_naive_fallback, fallback condition": (
        "batch/s_FallbackClusterer_Naive/g-s-/bfc/none/f64",
        "batch/s_FallbackClusterer_Naive/g-s-/bfc+bnf/none/f64", "single_naive"),
    "no batch_naive_fallback, reduced": ("batch/both_naive/g-s-/none/none/f64",
                                         "batch/both_naive/g-s-/bnf/none/f64", "reduced_naive"),
    "no batch_multi_stage": ("batch/m1_both/g-s-/none/none/f64", "batch/m1_both/g-s-/bms/none/f64",
                             "multi_stage"),
    "a user affinity function": ("batch/aff_fn/g-s-/all/none/f64", "batch/plain/g-s-/all/none/f64",
                                 "grouped"),
    "a user k-means function": ("batch/km_fn/g-s-/all/none/f64", "batch/plain/g-s-/all/none/f64",
                                "grouped"),
    "euclidean without batch_any_metric, single": ("batch/s_euclid/g-s-/none/none/f64",
                                                   "batch/s_euclid/g-s-/bam/none/f64", "single"),
    "euclidean without batch_any_metric, reduced": (
        "batch/both_euclid/g-s-/none/none/f64", "batch/both_euclid/g-s-/bam/none/f64", "reduced"),
    "euclidean without batch_any_metric, constrained": (
        "batch/c_euclid/g-s-/none/cm/f64", "batch/c_euclid/g-s-/all/cm/f64", "constrained"),
    "affinities: a raw ndarray constraint": (
        "affinity/c_plain/g-s-/none/raw/f64", "affinity/c_plain/g-s-/none/cm/f64", "affinities"),
    "affinities: group=1": ("affinity/plain/g1s-/none/none/f64",
                            "affinity/plain/g-s-/none/none/f64", "affinities"),
    "affinities: AutoTune": ("affinity/at/g-s-/none/none/f64", "affinity/plain/g8s-/none/none/f64",
                             "affinities"),
}


@pytest.mark.parametrize("reason", sorted(LOOPS))
def test_the_loop_is_the_outcome_for_every_reason_the_docstring_gives(reason):
  loops, calls, symbol = LOOPS[reason]
  outcome = OUTCOMES[loops]
  assert "exc" not in outcome and _symbols(outcome) == []
  assert [e.rstrip("+c") for e in _looped(outcome)] == ["p4", "p9", "p13"]
  assert outcome["routes"] == [0, 0, 0]
  assert all(re.fullmatch(r"<i8:7\*\d+", r) for r in outcome["res"])
  assert _symbols(OUTCOMES[calls]) == [_batch_fake.PREFIX + symbol]
  assert _looped(OUTCOMES[calls]) == []


def test_every_per_utterance_error_is_the_outcome_of_a_case():
  raised = {outcome["exc"] for outcome in OUTCOMES.values() if "exc" in outcome}
  for text in (FEW, FEW + " (utterance 0)", BIG, BIG + " (utterance 1)",
               OFFSET + " (utterance 0)",
               "ValueError: constraint_matrices must be as long as the batch",
               "ValueError: adaptation_threshold cannot be smaller than threshold"):
    assert text in raised, text
  # a case that raises before the call made no batch call
  for cid, outcome in OUTCOMES.items():
    if outcome.get("exc", "").startswith("ValueError"):
      assert _symbols(outcome) == [], cid
