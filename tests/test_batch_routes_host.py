"""CPU: the report of what ran in a batch (sc_last_batch_routes) is exported by the library,
declared in the header and in the ctypes mirror, and rejects a NULL handle.  No compute call is
made (there is no GPU here)."""

import ctypes
import os
import re

from spectralcluster_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_batch_route_report():
  header = open(os.path.join(ROOT, "include", "spectralcluster_amd.h")).read()
  declared = set(re.findall(r"^(?:int|const char\*)\s+(sc_[a-z0-9_]+)\s*\(", header, flags=re.M))
  lib = _lib.load()
  assert "sc_last_batch_routes" in declared
  assert "sc_last_batch_routes" in _lib.PROTOTYPES
  assert hasattr(lib, "sc_last_batch_routes")
  assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)
  # the route codes of the header and of the binding agree
  for name, value in (("SINGLE", 0), ("GROUP_LANCZOS", 1), ("GROUP_JACOBI", 2)):
    assert re.search(r"SC_BATCH_ROUTE_%s\s*=\s*%d\b" % (name, value), header), name
    assert getattr(_lib, "BATCH_ROUTE_" + name) == value
  # an addition only: the structs are the parent's (ABI 9: the test entry of the refinement front)
  assert lib.sc_abi_version() == _lib.SC_ABI_VERSION == 11


def test_null_handle_is_invalid():
  lib = _lib.load()
  routes = (ctypes.c_int32 * 4)()
  assert lib.sc_last_batch_routes(None, routes, 4) == _lib.SC_ERR_INVALID
