"""What the library answers for bad `sc_array` descriptors, entry point by entry point: the return
code and the `sc_last_error` text.  Needs the GPU (a handle), but every case fails in validation:
nothing is launched or copied.  Descriptors are 4 x 3 or 4 x 4 over one host buffer.

  python tools/make_descriptor_errors_golden.py   writes tests/golden/descriptor_errors.json

tests/test_gpu_stage_device.py replays `CASES` against that file.
"""

import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from spectralcluster_amd import _lib  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "descriptor_errors.json")
F64, F32, F16, BF16, I64, I32 = (_lib.SC_DTYPE_F64, _lib.SC_DTYPE_F32, _lib.SC_DTYPE_F16,
                                 _lib.SC_DTYPE_BF16, _lib.SC_DTYPE_I64, _lib.SC_DTYPE_I32)
HOST, DEVICE = _lib.SC_MEM_HOST, _lib.SC_MEM_DEVICE

BUF = np.zeros(64, dtype=np.float64)  # every descriptor's memory (none of it is read or written)
AT = BUF.ctypes.data
LABELS = np.zeros(8, dtype=np.int64)


def arr(rows, cols, rs=None, cs=1, dtype=F64, location=HOST, data=AT):
  return _lib.ScArray(data, dtype, location, rows, cols, cols if rs is None else rs, cs)


def matrix_faults(rows, cols):
  """(name, descriptor or None) that no entry point takes as a (rows, cols) input."""
  return [
      ("NULL descriptor", None),
      ("NULL data", arr(rows, cols, data=None)),
      ("zero rows", arr(0, cols)),
      ("zero columns", arr(rows, 0)),
      ("rows that fit no int", arr(2**31, cols)),
      ("dtype below the range", arr(rows, cols, dtype=-1)),
      ("dtype above the range", arr(rows, cols, dtype=BF16 + 1)),
      ("an integer dtype", arr(rows, cols, dtype=I64)),
      ("bad location", arr(rows, cols, location=5)),
      ("negative row stride", arr(rows, cols, rs=-cols)),
      ("negative column stride", arr(rows, cols, cs=-1)),
      ("host pointer labelled device", arr(rows, cols, location=DEVICE)),
      # two at once: which one answers
      ("NULL data and a bad dtype", arr(rows, cols, data=None, dtype=9)),
      ("bad dtype and bad location", arr(rows, cols, dtype=9, location=5)),
      ("bad location and a negative stride", arr(rows, cols, rs=-1, location=5)),
      ("negative stride and a host pointer labelled device", arr(rows, cols, cs=-1, location=DEVICE)),
  ]


def out_faults(rows, cols):
  """... as a (rows, cols) output."""
  by_rows = [  # (a dimension of one element addresses nothing: these need rows > 1)
      ("zero row stride", arr(rows, cols, rs=0)),
      ("overlapping rows", arr(rows, cols, rs=cols - 1)),
      ("both strides 1", arr(rows, cols, rs=1, cs=1)),
  ] if rows > 1 else []
  return matrix_faults(rows, cols)[:2] + by_rows + [
      ("wrong shape", arr(rows, cols + 1)),
      ("transposed shape", arr(cols + 1, rows)),
      ("dtype above the range", arr(rows, cols, dtype=BF16 + 1)),
      ("bad location", arr(rows, cols, location=5)),
      ("negative row stride", arr(rows, cols, rs=-cols)),
      ("zero column stride", arr(rows, cols, cs=0)),
      ("host pointer labelled device", arr(rows, cols, location=DEVICE)),
      ("wrong shape and not injective", arr(rows, cols + 1, cs=0)),
      ("negative stride and not injective", arr(rows, cols, rs=-1, cs=0)),
      ("not injective and a host pointer labelled device", arr(rows, cols, cs=0, location=DEVICE)),
  ]


def vec(n, stride=1, dtype=I64, location=HOST, data=AT, rows=1):
  return _lib.ScArray(data, dtype, location, rows, n, 0, stride)


def label_faults(n, output):
  faults = [
      ("NULL data", vec(n, data=None)),
      ("two rows", vec(n, rows=2)),
      ("float16", vec(n, dtype=F16)),
      ("dtype above the range", vec(n, dtype=I32 + 1)),
      ("bad location", vec(n, location=5)),
      ("negative stride", vec(n, stride=-1)),
      ("host pointer labelled device", vec(n, location=DEVICE)),
      ("float16 and bad location", vec(n, dtype=F16, location=5)),
      ("zero stride and a host pointer labelled device", vec(n, stride=0, location=DEVICE)),
  ]
  if output:  # (an input may be float64 and may repeat one entry)
    faults += [("float64", vec(n, dtype=F64)), ("zero stride", vec(n, stride=0))]
  else:
    faults.append(("wrong length", vec(n + 1)))
  return faults


def pair(first, second):
  """Two descriptors as a C array; member 1 is the one under test."""
  return (_lib.ScArray * 2)(first, second)


def _cases():
  """name -> a function of (lib, raw handle) that makes the call and returns its code."""
  cases = {}
  p = lambda a: None if a is None else ctypes.byref(a)

  def add(name, call):
    assert name not in cases, name
    cases[name] = call

  for name, a in matrix_faults(4, 3):
    add("sc_set_embeddings_array: " + name, lambda lib, h, a=a: lib.sc_set_embeddings_array(h, p(a)))
    add("sc_stage_affinity_array x: " + name,
        lambda lib, h, a=a: lib.sc_stage_affinity_array(h, p(a), p(arr(4, 4))))
    add("sc_stage_kmeans_metric_array: " + name,
        lambda lib, h, a=a: lib.sc_stage_kmeans_metric_array(h, p(a), 10, 0, None, None, None))
    add("sc_stage_kmeans_general_array: " + name,
        lambda lib, h, a=a: lib.sc_stage_kmeans_general_array(h, p(a), 2, 10, 0, 0.0, None, None,
                                                              None, None))
  big = arr(65536, 65536)
  add("sc_stage_kmeans_metric_array: 2^32 elements",
      lambda lib, h: lib.sc_stage_kmeans_metric_array(h, p(big), 10, 0, None, None, None))
  add("sc_stage_kmeans_general_array: 2^32 elements",
      lambda lib, h: lib.sc_stage_kmeans_general_array(h, p(big), 2, 10, 0, 0.0, None, None, None,
                                                       None))
  for name, a in matrix_faults(4, 4) + [("not square", arr(4, 3)),
                                        ("not square and a bad dtype", arr(4, 3, dtype=9))]:
    add("sc_set_affinity_array: " + name, lambda lib, h, a=a: lib.sc_set_affinity_array(h, p(a)))
    add("sc_set_constraint_array: " + name,
        lambda lib, h, a=a: lib.sc_set_constraint_array(h, p(a)))
    add("sc_stage_eig_array in: " + name,
        lambda lib, h, a=a: lib.sc_stage_eig_array(h, p(a), 2, 1, p(arr(1, 2)), p(arr(4, 2)),
                                                   None))
  for name, o in out_faults(4, 4):
    add("sc_stage_affinity_array out: " + name,
        lambda lib, h, o=o: lib.sc_stage_affinity_array(h, p(arr(4, 3)), p(o)))
  for name, o in out_faults(1, 2):
    add("sc_stage_eig_array values: " + name,
        lambda lib, h, o=o: lib.sc_stage_eig_array(h, p(arr(4, 4)), 2, 1, p(o), p(arr(4, 2)), None))
  for name, o in out_faults(4, 2):
    add("sc_stage_eig_array vectors: " + name,
        lambda lib, h, o=o: lib.sc_stage_eig_array(h, p(arr(4, 4)), 2, 1, p(arr(1, 2)), p(o), None))

  def labels_egress(lib, h, o):
    ptrs = (ctypes.POINTER(ctypes.c_int64) * 2)(
        LABELS.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
        LABELS.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    return lib.sc_labels_egress(h, ptrs, 2, pair(vec(6), o))
  for name, o in label_faults(6, True) + [("negative length", vec(-1))]:
    add("sc_labels_egress out 1: " + name, lambda lib, h, o=o: labels_egress(lib, h, o))

  def centroids(lib, h, x=None, lab=None, out=None):
    return lib.sc_cluster_centroids_arrays(
        h, pair(arr(4, 3), arr(4, 3) if x is None else x),
        pair(vec(4), vec(4) if lab is None else lab), 2,
        pair(arr(2, 3), arr(2, 3) if out is None else out), None)
  for name, a in matrix_faults(4, 3)[1:] + [("another d", arr(4, 4))]:
    add("sc_cluster_centroids_arrays x 1: " + name, lambda lib, h, a=a: centroids(lib, h, x=a))
  for name, l in label_faults(4, False):
    add("sc_cluster_centroids_arrays labels 1: " + name,
        lambda lib, h, l=l: centroids(lib, h, lab=l))
  for name, o in out_faults(2, 3)[1:] + [("negative rows", arr(-1, 3))]:
    add("sc_cluster_centroids_arrays out 1: " + name, lambda lib, h, o=o: centroids(lib, h, out=o))
  return cases


CASES = _cases()


def record(handle, key):
  code = CASES[key](handle.lib, handle.raw)
  return {"code": int(code), "error": handle.lib.sc_last_error(handle.raw).decode()}


def main():
  handle = _lib.default_handle()
  table = {key: record(handle, key) for key in CASES}
  os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
  out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
  with open(out, "w") as f:
    json.dump(table, f, indent=1, sort_keys=True)
    f.write("\n")
  print("%s: %d cases, %d refused" % (out, len(table), sum(v["code"] != 0 for v in table.values())))


if __name__ == "__main__":
  main()
