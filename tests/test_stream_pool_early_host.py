"""CPU: the two stream-pool entries of the early stage (sc_pool_fallback, sc_pool_cache) are
exported by the library, declared in the header and in the ctypes mirror, and reject a NULL pool;
the pool class carries the opt-in flag and the two route codes.  No compute call is made (there
is no GPU here)."""

import ctypes
import inspect
import os
import re

from spectralcluster_amd import _lib
from spectralcluster_amd import multi_stage_clusterer as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sc_pool_fallback", "sc_pool_cache")


def test_library_exports_the_early_stage_entries():
  header = open(os.path.join(ROOT, "include", "spectralcluster_amd.h")).read()
  declared = set(re.findall(r"^(?:int|const char\*)\s+(sc_[a-z0-9_]+)\s*\(", header, flags=re.M))
  lib = _lib.load()
  for name in ENTRIES:
    assert name in declared, name
    assert name in _lib.PROTOTYPES, name
    assert hasattr(lib, name), name
  assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)
  # additions only: no struct changed
  assert lib.sc_abi_version() == _lib.SC_ABI_VERSION == 11


def test_null_pool_is_invalid():
  lib = _lib.load()
  slots = (ctypes.c_int32 * 1)(0)
  labels = (ctypes.c_int64 * 4)()
  out = (ctypes.POINTER(ctypes.c_int64) * 1)(ctypes.cast(labels, ctypes.POINTER(ctypes.c_int64)))
  assert lib.sc_pool_fallback(None, slots, 1, 0.5, out) == _lib.SC_ERR_INVALID
  assert lib.sc_pool_cache(None, 0, ctypes.byref(_lib.ScArray())) == _lib.SC_ERR_INVALID


def test_pool_class_has_the_flag_and_the_route_codes():
  assert ms.ROUTE_EARLY_FALLBACK == 3
  assert ms.ROUTE_EARLY_MAIN == 4
  # (the codes that were there keep their values)
  assert (ms.ROUTE_MAIN_ONLY, ms.ROUTE_POOLED_GROUPED, ms.ROUTE_POOLED_SINGLE) == (0, 1, 2)
  parameter = inspect.signature(ms.MultiStageStreamPool).parameters["pool_early_stage"]
  assert parameter.default is False
  assert parameter.kind is inspect.Parameter.KEYWORD_ONLY
