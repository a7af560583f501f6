"""Host side of the constrained batch: `sc_predict_batch_constrained` and its test entry
`sc_stage_constraint_band_group` were additions to ABI 8 (now 9) -- declared in the header, mirrored in
`_lib.PROTOTYPES`, exported by the library, and safe to call with a NULL handle.  No GPU."""

import ctypes
import os
import re

from spectralcluster_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spectralcluster_amd.h")
NEW_SYMBOLS = ("sc_predict_batch_constrained", "sc_stage_constraint_band_group")


def declared_functions():
  header = open(HEADER).read()
  return set(re.findall(r"^(?:int|const char\*)\s+(sc_[a-z0-9_]+)\s*\(", header, flags=re.M))


def test_new_symbols_are_declared_mirrored_and_exported():
  declared = declared_functions()
  lib = _lib.load()
  for name in NEW_SYMBOLS:
    assert name in declared
    assert name in _lib.PROTOTYPES
    assert getattr(lib, name) is not None
  assert declared == set(_lib.PROTOTYPES)


def test_abi_version_is_9():
  assert _lib.SC_ABI_VERSION == 11
  assert _lib.load().sc_abi_version() == 11
  text = open(HEADER).read()
  assert re.search(r"#define\s+SC_ABI_VERSION\s+11\b", text)


def test_null_handle_is_invalid():
  lib = _lib.load()
  cfg = _lib.ScConfig()
  lib.sc_config_default(cfg)
  assert lib.sc_predict_batch_constrained(None, None, None, 0, cfg, None, None, 16) == \
      _lib.SC_ERR_INVALID
  ns = (ctypes.c_int32 * 1)(4)
  assert lib.sc_stage_constraint_band_group(None, cfg, 1, ns, None, None, None) == \
      _lib.SC_ERR_INVALID
