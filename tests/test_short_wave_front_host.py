"""CPU: the interface additions of the short wave front -- the new enumerators of
include/spectralcluster_amd.h against their mirrors in spectralcluster_amd/_lib.py, the ABI
version they were added under, and the route switch in csrc/switches.h."""

import os
import re

from spectralcluster_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
  with open(os.path.join(ROOT, *parts)) as f:
    return f.read()


def enumerator(header, name):
  m = re.search(r"\b%s\s*=\s*(\d+)" % name, header)
  assert m, name
  return int(m.group(1))


def test_enumerators_match_the_python_mirror():
  header = read("include", "spectralcluster_amd.h")
  assert enumerator(header, "SC_FRONT_ROUTE_SHORT_WAVE") == _lib.SC_FRONT_ROUTE_SHORT_WAVE == 4
  assert enumerator(header, "SC_FRONT_INFO_LAUNCHES") == _lib.SC_FRONT_INFO_LAUNCHES == 13
  assert enumerator(header, "SC_FRONT_INFO_CUT_KERNEL") == _lib.SC_FRONT_INFO_CUT_KERNEL == 11
  assert "5 k_short_wave_front" in header
  # every slot of info that has a name in the header has the same place in the mirror
  for slot, name in enumerate(_lib.FRONT_INFO_NAMES):
    assert enumerator(header, "SC_FRONT_INFO_" + name.upper()) == slot, name
  assert len(_lib.FRONT_INFO_NAMES) <= enumerator(header, "SC_FRONT_INFO_COUNT")
  assert enumerator(header, "SC_FRONT_INFO_COUNT") == _lib.SC_FRONT_INFO_COUNT
  # the other routes keep their numbers
  for value, name in enumerate(("SINGLE", "GROUPED", "SWEEP", "SHORT_SWEEP")):
    assert enumerator(header, "SC_FRONT_ROUTE_" + name) == value
    assert getattr(_lib, "SC_FRONT_ROUTE_" + name) == value


def test_abi_version_is_unchanged():
  header = read("include", "spectralcluster_amd.h")
  assert re.search(r"#define\s+SC_ABI_VERSION\s+11\b", header)
  assert _lib.SC_ABI_VERSION == 11


def test_switch_is_listed_with_the_other_route_switches():
  switches = read("spectralcluster_amd", "csrc", "switches.h")
  assert 'getenv("SC_SHORT_FRONT_MEMBERWISE")' in switches
  assert "short_front_memberwise()" in switches
  # ... and it is the one place the library reads it
  csrc = os.path.join(ROOT, "spectralcluster_amd", "csrc")
  for name in sorted(os.listdir(csrc)):
    if name.endswith((".hip", ".cpp", ".h")) and name != "switches.h":
      assert "SC_SHORT_FRONT_MEMBERWISE" not in read("spectralcluster_amd", "csrc", name).replace(
          "SC_SHORT_FRONT_MEMBERWISE=1", ""), name
