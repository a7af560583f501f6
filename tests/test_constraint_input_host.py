"""CPU: `DenseConstraints`, a dense constraint matrix taken where it is.  What the wrapper accepts
and rejects is decided before any device is touched; the new entry points are declared,
prototyped, exported and listed; the ABI version and the batch descriptor did not move."""

import ctypes
import os
import re

import numpy as np
import pytest

import spectralcluster_amd as sca
from spectralcluster_amd import _lib
from spectralcluster_amd import constraint as con

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sc_set_constraint_array", "sc_stage_constraint_array",
               "sc_predict_batch_constraint_arrays", "sc_stage_constraint_dense_group",
               "sc_stage_gemm_pair_group")


def test_dense_constraints_is_exported_and_stores_the_object_as_it_is():
  assert sca.DenseConstraints is con.DenseConstraints
  assert "DenseConstraints" in sca.__all__
  wide = np.zeros((6, 12), dtype=np.float32)
  for q in (np.eye(6), np.eye(6, dtype=np.float32), np.eye(6, dtype=np.float16),
            np.eye(6).T, wide[:, ::2], np.zeros((1, 1))):
    d = sca.DenseConstraints(q)
    assert d.matrix is q  # no copy, no conversion
    assert d.n == q.shape[0] and d.shape == q.shape


def test_dense_constraints_rejects_what_is_no_float_square_matrix():
  with pytest.raises(ValueError, match="constraint matrix must be a square matrix"):
    sca.DenseConstraints(np.zeros((4, 5)))
  with pytest.raises(ValueError, match="constraint matrix must be 2-dimensional"):
    sca.DenseConstraints(np.zeros(9))
  with pytest.raises(ValueError, match="constraint matrix must be 2-dimensional"):
    sca.DenseConstraints(np.zeros((3, 3, 3)))
  with pytest.raises(TypeError, match="constraint matrix must be float64"):
    sca.DenseConstraints(np.eye(4, dtype=np.int32))
  with pytest.raises(TypeError, match="constraint matrix must be float64"):
    sca.DenseConstraints(np.eye(4, dtype=bool))
  with pytest.raises(ValueError, match="negative strides"):
    sca.DenseConstraints(np.eye(4)[::-1])
  with pytest.raises(ValueError, match="negative strides"):
    sca.DenseConstraints(np.eye(4, dtype=np.float32)[:, ::-1])
  with pytest.raises(TypeError, match="numpy array or support __dlpack__"):
    sca.DenseConstraints([[1.0, 0.0], [0.0, 1.0]])


class FakeTensor:
  """What a DLPack producer shows without handing out a capsule: shape, dtype, stride()."""

  def __init__(self, shape, dtype, strides):
    self.shape, self.dtype, self._strides = shape, dtype, strides

  def stride(self):
    return self._strides

  def __dlpack__(self, stream=None):
    raise AssertionError("no capsule is asked for at construction")

  def __dlpack_device__(self):
    raise AssertionError("the device is not asked for at construction")


def test_a_dlpack_object_is_checked_at_construction_through_its_attributes():
  for dtype in ("torch.float64", "torch.float32", "torch.float16", "torch.bfloat16", "float32"):
    assert sca.DenseConstraints(FakeTensor((4, 4), dtype, (4, 1))).n == 4
  assert sca.DenseConstraints(FakeTensor((4, 4), "torch.float16", (1, 4))).n == 4  # a .T view
  for dtype in ("torch.int32", "torch.bool", "int64", "torch.complex64", "torch.float8_e4m3fn"):
    with pytest.raises(TypeError, match="constraint matrix must be float64"):
      sca.DenseConstraints(FakeTensor((4, 4), dtype, (4, 1)))
  with pytest.raises(ValueError, match="negative strides"):
    sca.DenseConstraints(FakeTensor((4, 4), "float32", (-4, 1)))
  with pytest.raises(ValueError, match="square"):
    sca.DenseConstraints(FakeTensor((4, 5), "float32", (5, 1)))
  # ... so a batch refuses it before any other source is described
  c = constrained_clusterer()
  with pytest.raises(TypeError, match="constraint matrix must be float64"):
    c.predict_batch([np.ones((4, 2))] * 2, constraint_matrices=[
        sca.DenseConstraints(np.eye(4)),
        sca.DenseConstraints(FakeTensor((4, 4), "torch.int32", (4, 1)))])


def test_the_embeddings_errors_kept_their_wording():
  from spectralcluster_amd import _dlpack
  assert _dlpack.dtype_message("embeddings", "DLPack type code 0, 32 bits, 1 lanes") == (
      "embeddings must be float64, float32, float16 or bfloat16 "
      "(DLPack type code 0, 32 bits, 1 lanes)")
  assert _dlpack.negative_strides_message("embeddings") == (
      "embeddings with negative strides are not supported")


def test_the_affinity_checks_kept_their_wording():
  c = sca.SpectralClusterer(min_clusters=2, max_clusters=5)
  with pytest.raises(ValueError, match=r"affinity must be 2-dimensional, got shape \(9,\)"):
    c.predict_affinity(np.zeros(9))
  with pytest.raises(ValueError, match=r"affinity 1 must be a square matrix, got shape \(4, 5\)"):
    c.predict_affinity_batch([np.eye(4), np.zeros((4, 5))])


@pytest.mark.parametrize("operator", [con.AffinityIntegration(con.IntegrationType.Max),
                                      con.ConstraintPropagation(0.4)])
def test_check_input_gives_the_same_shape_message(operator):
  operator.check_input(np.eye(5), sca.DenseConstraints(np.eye(5, dtype=np.float16)))
  with pytest.raises(ValueError, match="affinity and constraint matrix must have the same shape"):
    operator.check_input(np.eye(5), sca.DenseConstraints(np.eye(6)))
  with pytest.raises(ValueError, match="same shape"):  # ... from adjust_affinity, before a device
    operator.adjust_affinity(np.eye(5), sca.DenseConstraints(np.eye(6)))


def constrained_clusterer():
  return sca.SpectralClusterer(
      min_clusters=2, max_clusters=5,
      constraint_options=sca.ConstraintOptions(
          constraint_name=sca.ConstraintName.ConstraintPropagation,
          apply_before_refinement=True, constraint_propagation_alpha=0.4))


def test_a_batch_gives_the_same_shape_message_before_anything_is_launched():
  c = constrained_clusterer()
  us = [np.ones((6, 4)), np.ones((7, 4))]
  wrong = [sca.DenseConstraints(np.eye(6)), sca.DenseConstraints(np.eye(8, dtype=np.float32))]
  with pytest.raises(ValueError, match="same shape"):
    c.predict_affinity_batch([np.eye(6), np.eye(7)], wrong)
  with pytest.raises(ValueError, match="as long as the batch"):
    c.predict_batch(us, constraint_matrices=wrong[:1])
  with pytest.raises(ValueError, match="as long as the batch"):
    c.predict_affinity_batch([np.eye(6)], wrong)


def test_new_symbols_are_declared_prototyped_exported_and_listed():
  header = open(os.path.join(ROOT, "include", "spectralcluster_amd.h")).read()
  declared = set(re.findall(r"^(?:int|const char\*)\s+(sc_[a-z0-9_]+)\s*\(", header, flags=re.M))
  integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
  lib = _lib.load()
  for name in NEW_SYMBOLS:
    assert name in declared, name
    assert name in _lib.PROTOTYPES, name
    assert hasattr(lib, name), name
    assert "`%s`" % name in integration, name
  assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)


def test_abi_version_is_still_10_everywhere():
  header = open(os.path.join(ROOT, "include", "spectralcluster_amd.h")).read()
  assert re.search(r"^#define SC_ABI_VERSION 11$", header, flags=re.M)
  assert _lib.SC_ABI_VERSION == 11
  assert _lib.load().sc_abi_version() == 11  # functions were only added


def test_the_batch_descriptor_did_not_move():
  size = ctypes.c_int(0)
  offsets = (ctypes.c_int * 6)()
  assert _lib.load().sc_constraint_desc_layout(ctypes.byref(size), offsets) == _lib.SC_OK
  assert size.value == ctypes.sizeof(_lib.ScConstraintDesc) == 40
  assert list(offsets) == [0, 4, 8, 16, 24, 32]
  assert [getattr(_lib.ScConstraintDesc, f).offset for f, _ in
          _lib.ScConstraintDesc._fields_] == list(offsets)


def test_entry_points_reject_a_null_handle():
  lib = _lib.load()
  assert lib.sc_set_constraint_array(None, None) == _lib.SC_ERR_INVALID
  assert lib.sc_stage_constraint_array(None, None, None, None, 4, None) == _lib.SC_ERR_INVALID
  assert lib.sc_predict_batch_constraint_arrays(None, None, None, None, 0, None, None, None, 16,
                                                0) == _lib.SC_ERR_INVALID
  assert lib.sc_stage_constraint_dense_group(None, None, 1, None, None, None,
                                             None) == _lib.SC_ERR_INVALID
  assert lib.sc_stage_gemm_pair_group(None, 1, None, None, None, None, None, 0,
                                      0) == _lib.SC_ERR_INVALID
