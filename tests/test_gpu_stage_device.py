"""GPU: the building blocks with input and result where the caller holds them --
`utils.compute_affinity_matrix`, the six `refine`, `laplacian.compute_laplacian` and
`utils.compute_sorted_eigenvectors` on device tensors and host arrays of float64 / float32 /
float16 / bfloat16, contiguous, pitched or transposed, with `out=`.  Widening is exact and the
kernels are those of the float64 path, so every check is an equality: `f(input, out=o)` is, bit for
bit, `_narrow_ref` of `f(the widened float64 ndarray)` (a NaN by position)."""

import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
# (at module level on purpose: PyTorch has to be in the process before the library is loaded,
#  so that both use one HIP runtime -- INTEGRATION.md section 6)
import torch

import _narrow_ref as nr

import spectralcluster_amd as sca
from spectralcluster_amd import _dlpack
from spectralcluster_amd import _lib
from spectralcluster_amd import laplacian
from spectralcluster_amd import refinement
from spectralcluster_amd import utils

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FLOAT = {"float64": torch.float64, "float32": torch.float32, "float16": torch.float16,
         "bfloat16": torch.bfloat16}
INT = {"float64": torch.int64, "float32": torch.int32, "float16": torch.int16,
       "bfloat16": torch.int16}
# one element; one pair; an odd size below the tile; the tile; one past it; two tiles and one;
# more than three tiles with a ragged edge and a pitch rounded up
SIZES = [1, 2, 17, 64, 65, 129, 200]
LAYOUTS = ("contiguous", "pitched", "transposed")

OPERATORS = {
    "CropDiagonal": refinement.CropDiagonal,
    "GaussianBlur1": lambda: refinement.GaussianBlur(1),
    "GaussianBlur2": lambda: refinement.GaussianBlur(2),
    "RowWiseThreshold": refinement.RowWiseThreshold,
    "RowWiseThresholdPercentile": lambda: refinement.RowWiseThreshold(
        0.9, 0.01, refinement.ThresholdType.Percentile, True, True),
    "SymmetrizeMax": refinement.Symmetrize,
    "SymmetrizeAverage": lambda: refinement.Symmetrize(refinement.SymmetrizeType.Average),
    "Diffuse": refinement.Diffuse,
    "RowWiseNormalize": refinement.RowWiseNormalize,
}


def holder(rows, cols, dtype, layout, device):
  """An uninitialised-looking (rows, cols) view in `layout`, inside a tensor filled with 3."""
  t = FLOAT[dtype]
  if layout == "contiguous":
    return torch.full((rows, cols), 3.0, dtype=t, device=device)
  if layout == "pitched":  # begins one element into a row: a misaligned base, a pitch above cols
    return torch.full((rows + 1, cols + 7), 3.0, dtype=t, device=device)[1:, 1:1 + cols]
  return torch.full((cols, rows + 3), 3.0, dtype=t, device=device)[:, 2:2 + rows].t()


def placed(values: torch.Tensor, dtype, layout, device):
  """`values` (a CPU tensor of `dtype`) in `layout` on `device`."""
  h = holder(values.shape[0], values.shape[1], dtype, layout, device)
  h.copy_(values)
  return h


def bits_of(t) -> np.ndarray:
  if isinstance(t, np.ndarray):
    return np.ascontiguousarray(t).view(nr.BITS[str(t.dtype)])
  name = str(t.dtype).split(".")[-1]
  return t.contiguous().cpu().view(INT[name]).numpy().view(nr.BITS[name])


def matrix(n, dtype, seed):
  """A non-symmetric affinity-like (n, n) matrix, as a CPU tensor of `dtype`."""
  g = torch.Generator().manual_seed(seed)
  return (torch.rand(n, n, generator=g, dtype=torch.float64) * 0.9 + 0.05).to(FLOAT[dtype])


def check_function(f, make_input, out_shape):
  """f(input, out) against _narrow_ref(f(widened)) over input dtype x output dtype x layout x
  memory (a NumPy array stands in for the host tensor where NumPy has the dtype)."""
  for in_dtype in nr.DTYPES:
    values = make_input(in_dtype)
    want64 = f(values.double().numpy(), None)
    assert isinstance(want64, np.ndarray) and want64.dtype == np.float64
    assert want64.shape == out_shape
    for out_dtype in nr.DTYPES:
      want = nr.narrow_bits(want64, out_dtype)
      for layout in LAYOUTS:
        for device in ("cuda", "cpu"):
          x = placed(values, in_dtype, layout, device)
          o = holder(out_shape[0], out_shape[1], out_dtype, layout, device)
          what = "%s %s -> %s %s %s" % (in_dtype, layout, out_dtype, layout, device)
          if device == "cpu" and layout != "contiguous":  # ndarrays of the same strides
            if in_dtype != "bfloat16":
              x = x.numpy()
            if out_dtype != "bfloat16":
              o = o.numpy()
          assert f(x, o) is o, what
          nr.assert_same_bits(bits_of(o), want, out_dtype, what)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("d", [1, 7, 256])
def test_affinity_matrix(handle, d, n):
  def make_input(dtype):
    g = torch.Generator().manual_seed(100 * n + d)
    return torch.randn(n, d, generator=g, dtype=torch.float64).to(FLOAT[dtype])
  check_function(lambda x, o: utils.compute_affinity_matrix(x, out=o), make_input, (n, n))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(OPERATORS))
def test_refinement_operators(handle, name, n):
  op = OPERATORS[name]()
  check_function(lambda x, o: op.refine(x, out=o), lambda dtype: matrix(n, dtype, n), (n, n))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", list(laplacian.LaplacianType), ids=lambda k: k.name)
def test_laplacian(handle, kind, n):
  check_function(lambda x, o: laplacian.compute_laplacian(x, kind, out=o),
                 lambda dtype: matrix(n, dtype, 7 * n), (n, n))


# --- in place and aliased ------------------------------------------------------------------
@pytest.mark.parametrize("device", ["cuda", "cpu"])
@pytest.mark.parametrize("dtype", ["float64", "float32", "bfloat16"])
def test_out_may_be_the_input_its_transpose_or_overlap_it(handle, dtype, device):
  n = 130
  values = matrix(n, dtype, 5)
  wide = values.double().numpy()
  for op in (refinement.Symmetrize(), refinement.RowWiseThreshold()):
    want = nr.narrow_bits(op.refine(wide.copy()), dtype)
    # out is the input
    x = values.clone().to(device)
    assert op.refine(x, out=x) is x
    nr.assert_same_bits(bits_of(x), want, dtype, "out is input")
    # out is the input's transpose: position (i, j) of the result lands where (j, i) was read
    x = values.clone().to(device)
    o = x.t()
    assert op.refine(x, out=o) is o
    nr.assert_same_bits(bits_of(o), want, dtype, "out is input.T")
    # out begins in the middle of the input
    buf = torch.zeros(n * n + n * n // 2, dtype=FLOAT[dtype], device=device)
    x = buf[:n * n].view(n, n)
    x.copy_(values)
    o = buf[n * n // 2:].view(n, n)
    assert op.refine(x, out=o) is o
    nr.assert_same_bits(bits_of(o), want, dtype, "out overlaps half of the input")
  # the Laplacian and the affinity as well: out is the input
  x = values.clone().to(device)
  want = nr.narrow_bits(laplacian.compute_laplacian(wide), dtype)
  laplacian.compute_laplacian(x, out=x)
  nr.assert_same_bits(bits_of(x), want, dtype, "laplacian in place")
  x = values.clone().to(device)
  want = nr.narrow_bits(utils.compute_affinity_matrix(wide), dtype)
  utils.compute_affinity_matrix(x, out=x)
  nr.assert_same_bits(bits_of(x), want, dtype, "affinity in place")


def test_without_out_a_device_input_returns_the_host_paths_array(handle):
  for dtype in nr.DTYPES:
    values = matrix(65, dtype, 9)
    wide = values.double().numpy()
    for x in (values.cuda(), values.cuda().t(), values):
      w = wide.T if x.stride(0) == 1 else wide
      for f in (utils.compute_affinity_matrix, refinement.GaussianBlur(1).refine,
                refinement.Diffuse().refine, laplacian.compute_laplacian):
        got = f(x)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64
        assert got.flags.c_contiguous
        nr.assert_same_bits(bits_of(got), bits_of(f(np.ascontiguousarray(w))), "float64",
                            "%s %s" % (dtype, getattr(f, "__qualname__", f)))


# --- eigenvectors --------------------------------------------------------------------------
def eig_input(n, symmetric, seed):
  rng = np.random.default_rng(seed)
  a = rng.uniform(0.0, 1.0, (n, n))
  if symmetric:
    a = (a + a.T) / 2
  return torch.from_numpy(a)


def host_eig(m, descend, count):
  """The host path, and whether two runs of it agree bit for bit."""
  a = utils.compute_sorted_eigenvectors(m, descend, count)
  b = utils.compute_sorted_eigenvectors(m, descend, count)
  same = all(np.array_equal(bits_of(p), bits_of(q)) for p, q in zip(a, b))
  return a, same


@pytest.mark.parametrize("symmetric", [True, False], ids=["symmetric", "general"])
@pytest.mark.parametrize("count", [8, 64])
@pytest.mark.parametrize("n", [64, 65, 128, 129, 200])
def test_sorted_eigenvectors_against_the_host_path(handle, n, count, symmetric):
  values = eig_input(n, symmetric, 1000 + n)
  wide = values.numpy()
  (w64, v64), reproducible = host_eig(wide, True, count)
  assert w64.shape == (count,) and v64.shape == (n, count)
  combos = [("float64", "float64", "contiguous", "cuda"), ("float64", "bfloat16", "pitched", "cpu")]
  if count == 8:  # (a solve for 64 pairs takes a second: two destinations there)
    combos += [("float64", "float32", "pitched", "cuda"), ("float64", "float64", "transposed", "cpu"),
               ("float64", "float16", "transposed", "cuda")]
  for in_dtype, out_dtype, layout, device in combos:
    x = placed(values, in_dtype, layout, device)
    ov = torch.full((2 * count + 1,), 3.0, dtype=FLOAT[out_dtype], device=device)[1::2]
    oe = holder(n, count, out_dtype, layout, device)
    got = utils.compute_sorted_eigenvectors(x, True, out=(ov, oe))
    assert got[0] is ov and got[1] is oe
    what = "%s -> %s %s %s" % (in_dtype, out_dtype, layout, device)
    if reproducible:
      nr.assert_same_bits(bits_of(ov), nr.narrow_bits(w64, out_dtype), out_dtype, what)
      nr.assert_same_bits(bits_of(oe), nr.narrow_bits(v64, out_dtype), out_dtype, what)
    else:
      # the solvers' own tolerance (tests/test_gpu_stages.py) plus the rounding of the output
      eps = {"float64": 0.0, "float32": 2.0 ** -24, "float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}
      scale = np.abs(w64).max()
      w = ov.double().cpu().numpy()
      np.testing.assert_allclose(w, w64, rtol=eps[out_dtype], atol=1e-12 * scale, err_msg=what)
      v = oe.double().cpu().numpy()
      resid = np.abs(wide @ v - v * w).max()
      assert resid < (1e-11 + 4 * n * eps[out_dtype]) * scale, (what, resid)
  if count != 8:
    return
  # descend=False and the default count without `out`: the host path's arrays
  (w64, v64), reproducible = host_eig(wide, False, None)
  w, v = utils.compute_sorted_eigenvectors(values.cuda(), False)
  assert w.shape == w64.shape and v.shape == v64.shape and v.dtype == np.float64
  if reproducible:
    nr.assert_same_bits(bits_of(w), bits_of(w64), "float64", "default count values")
    nr.assert_same_bits(bits_of(v), bits_of(v64), "float64", "default count vectors")
  else:
    np.testing.assert_allclose(w, w64, rtol=0, atol=1e-12 * np.abs(w64).max())


def decision(handle, t) -> int:
  src = _dlpack.describe_input(t, lambda: handle)
  try:
    symmetric = ctypes.c_int(-1)
    handle.check(handle.lib.sc_stage_eig_array(handle.raw, ctypes.byref(src.array), 0, 1, None,
                                               None, ctypes.byref(symmetric)))
    return symmetric.value
  finally:
    src.release()


@pytest.mark.parametrize("n", [2, 65, 200])
def test_the_symmetric_decision_is_todays_rule_made_on_the_device(handle, n):
  a = eig_input(n, True, n).numpy().copy()
  a[n // 2, n // 2] = 3.75  # max |m|
  atol = 1e-12 * 3.75
  i, j = 0, n - 1

  def rule(m):
    scale = float(np.max(np.abs(m)))
    return int(np.allclose(m, m.T, rtol=0.0, atol=1e-12 * max(scale, 1e-300)))

  cases = {"symmetric": a.copy(), "half of atol": a.copy(), "twice atol": a.copy(),
           "one NaN": a.copy(), "NaN on the diagonal": a.copy(), "zeros": np.zeros((n, n)),
           "an infinity facing a number": a.copy(), "two equal infinities": a.copy()}
  cases["half of atol"][i, j] += 0.5 * atol
  cases["twice atol"][j, i] -= 2 * atol
  cases["one NaN"][j, i] = np.nan
  cases["NaN on the diagonal"][0, 0] = np.nan
  cases["an infinity facing a number"][i, j] = np.inf
  cases["two equal infinities"][i, j] = cases["two equal infinities"][j, i] = np.inf
  want = {"symmetric": 1, "half of atol": 1, "twice atol": 0, "one NaN": 0,
          "NaN on the diagonal": 0, "zeros": 1, "an infinity facing a number": 0,
          "two equal infinities": 1}
  for name, m in cases.items():
    with np.errstate(invalid="ignore"):
      assert rule(m) == want[name], name  # (the cases are what they claim to be)
    t = torch.from_numpy(m)
    for obj in (t.cuda(), t.cuda().t(), t, placed(t, "float64", "pitched", "cuda")):
      assert decision(handle, obj) == want[name], name
  # fp16 input: differences are multiples of 2^-24, so with max |m| = 65504 (atol 6.55e-8) one
  # step (0.91 atol) is inside the tolerance and two steps (1.82 atol) are outside it
  h = np.zeros((n, n), dtype=np.float16)
  h[n // 2, n // 2] = 65504.0
  for steps, sym in ((0, 1), (1, 1), (2, 0)):
    m = h.copy()
    m[i, j] = steps * 2.0 ** -24
    assert rule(m.astype(np.float64)) == sym
    assert decision(handle, torch.from_numpy(m).cuda()) == sym, steps
    assert decision(handle, m) == sym, steps
  m = h.copy()
  m[j, i] = np.nan
  assert decision(handle, torch.from_numpy(m).cuda()) == 0


def test_the_decision_selects_the_solver(handle):
  """Just inside the tolerance the symmetric solver's result comes back, just outside it the
  general solver's: the host path on the same matrix says which is which."""
  n, count = 65, 8
  a = eig_input(n, True, 3).numpy().copy()
  a[1, 1] = 3.75
  for factor in (0.5, 2.0):
    m = a.copy()
    m[0, n - 1] += factor * 1e-12 * 3.75
    (w64, v64), reproducible = host_eig(m, True, count)
    ov = torch.zeros(count, dtype=torch.float64, device="cuda")
    oe = torch.zeros(n, count, dtype=torch.float64, device="cuda")
    utils.compute_sorted_eigenvectors(torch.from_numpy(m).cuda(), True, out=(ov, oe))
    if reproducible:
      nr.assert_same_bits(bits_of(ov), bits_of(w64), "float64", "values, factor %g" % factor)
      nr.assert_same_bits(bits_of(oe), bits_of(v64), "float64", "vectors, factor %g" % factor)
    else:
      np.testing.assert_allclose(ov.cpu().numpy(), w64, rtol=0, atol=1e-12 * np.abs(w64).max())


def test_the_chained_example_of_the_integration_guide(handle):
  """INTEGRATION.md section 7, as written: the same chain on host float64 arrays, each
  intermediate rounded to float32 where the example keeps it in float32."""
  import os
  import re
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = open(os.path.join(root, "INTEGRATION.md")).read()
  section = text[text.index("## 7. Building blocks on device tensors"):]
  code = re.search(r"```python\n(.*?)```", section, flags=re.S).group(1)
  scope = {}
  exec(compile(code, "INTEGRATION.md section 7", "exec"), scope)
  g = torch.Generator().manual_seed(7)
  x = torch.randn(150, 24, generator=g, dtype=torch.float64).to(torch.float16)
  values, vectors = scope["spectral_embedding"](x.cuda(), 6)
  assert values.is_cuda and vectors.is_cuda and vectors.shape == (150, 6)

  def f32(m):
    return m.astype(np.float32).astype(np.float64)
  a = f32(utils.compute_affinity_matrix(x.double().numpy()))
  a = f32(refinement.CropDiagonal().refine(a))
  a = f32(refinement.RowWiseThreshold(p_percentile=0.95).refine(a))
  a = f32(refinement.Symmetrize().refine(a))
  a = f32(laplacian.compute_laplacian(a, laplacian.LaplacianType.GraphCut))
  (w, v), reproducible = host_eig(a, False, 6)
  if reproducible:
    nr.assert_same_bits(bits_of(values), bits_of(w), "float64", "values")
    nr.assert_same_bits(bits_of(vectors), bits_of(v), "float64", "vectors")
  else:
    np.testing.assert_allclose(values.cpu().numpy(), w, rtol=0, atol=1e-12 * np.abs(w).max())


# --- errors --------------------------------------------------------------------------------
def test_every_out_error_on_device_tensors_and_nothing_is_written(handle):
  x = matrix(8, "float32", 1).cuda()
  op = refinement.CropDiagonal()
  z = lambda *shape, **kw: torch.zeros(*shape, device="cuda", **kw)  # noqa: E731
  for make, exc, match in (
      (lambda: z(1, 8).expand(8, 8), ValueError, "out maps two indices to one address"),
      (lambda: z(8, 1).expand(8, 8), ValueError, "out maps two indices to one address"),
      (lambda: z(64).as_strided((8, 8), (4, 1)), ValueError, "out maps two indices"),
      (lambda: z(64).as_strided((8, 8), (1, 6)), ValueError, "out maps two indices"),
      (lambda: z(8, 9), ValueError, r"out must have shape \(8, 8\)"),
      (lambda: z(64), ValueError, "out must be 2-dimensional"),
      (lambda: z(8, 8, dtype=torch.int32), TypeError, "out must be float64, float32, float16"),
      (lambda: z(8, 8, requires_grad=True), ValueError, "out cannot be exported"),
  ):
    o = make()
    before = o.detach().clone()
    for call in (lambda: op.refine(x, out=o), lambda: utils.compute_affinity_matrix(x, out=o),
                 lambda: laplacian.compute_laplacian(x, out=o)):
      with pytest.raises(exc, match=match):
        call()
    assert torch.equal(o.detach(), before)
  with pytest.raises(ValueError, match=r"out vectors must have shape \(8, 3\)"):
    utils.compute_sorted_eigenvectors(x, out=(z(3), z(8, 4)))
  with pytest.raises(ValueError, match="out values must be 1-dimensional"):
    utils.compute_sorted_eigenvectors(x, out=(z(3, 1), z(8, 3)))
  with pytest.raises(ValueError, match="out values"):
    utils.compute_sorted_eigenvectors(x, out=(z(1).expand(3), z(8, 3)))
  with pytest.raises(ValueError, match="bad eigen request"):
    utils.compute_sorted_eigenvectors(x, out=(z(9), z(8, 9)))
  # the library's own check of a descriptor that lies about its memory
  good = z(8, 8, dtype=torch.float64)
  src = _dlpack.describe_input(x, lambda: handle)
  host = np.zeros((8, 8))
  lying = _lib.ScArray(host.ctypes.data, _lib.SC_DTYPE_F64, _lib.SC_MEM_DEVICE, 8, 8, 8, 1)
  cfg = op._config()
  assert handle.lib.sc_stage_refine_array(handle.raw, 1, cfg, ctypes.byref(src.array),
                                          ctypes.byref(lying)) == _lib.SC_ERR_INVALID
  assert "out: location is SC_MEM_DEVICE" in handle.last_error()
  src.release()
  assert op.refine(x, out=good) is good  # ... and the handle is fine afterwards


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU")
def test_out_on_another_device_is_refused(handle):
  x = matrix(8, "float32", 1).cuda()
  o = torch.zeros(8, 8, device="cuda:1")
  with pytest.raises(ValueError, match="out is on device 1"):
    refinement.CropDiagonal().refine(x, out=o)
  with pytest.raises(ValueError, match="on device 1"):
    refinement.CropDiagonal().refine(x.to("cuda:1"))


# ------------------------------------------------- bad descriptors, as recorded
def test_every_entry_point_refuses_a_bad_descriptor_as_recorded(handle):
  """Return code and sc_last_error text of every case of tools/make_descriptor_errors_golden.py
  (raw ctypes calls that all fail in validation: nothing is launched) against the recorded file."""
  spec = importlib.util.spec_from_file_location(
      "make_descriptor_errors_golden",
      os.path.join(ROOT, "tools", "make_descriptor_errors_golden.py"))
  cases = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(cases)
  with open(os.path.join(ROOT, "tests", "golden", "descriptor_errors.json")) as f:
    want = json.load(f)
  assert sorted(want) == sorted(cases.CASES)
  assert all(v["code"] == _lib.SC_ERR_INVALID and v["error"] for v in want.values())
  got = {key: cases.record(handle, key) for key in cases.CASES}
  wrong = {key: (got[key], want[key]) for key in want if got[key] != want[key]}
  assert not wrong, wrong
