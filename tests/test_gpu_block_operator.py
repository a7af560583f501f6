"""GPU: the block operator kernels of the eigensolver, one application at a time, against a
longdouble product -- k_block_matvec, k_block_matvec_sym + k_matvec_sym_reduce, the two-product
form of the matrix-free Diffuse and the grouped launch, all through the production launchers
(`sc_stage_block_operator`).

Whole solves forgive an operator that is slightly wrong: the iteration converges cleanly to the
spectrum of a slightly different matrix.  Here every output entry is held to the a-priori bound
of a correctly rounded dot product in ANY summation order (tests/_krylov_ref.py):

  one product    |W - W_ref| <= gamma_{n+4}  (|p| |V| + |c| (|M| (|s| |V|)))
  two products   |W - W_ref| <= gamma_{2n+6} (|p| |V| + |c| (|A| (|A| (|s| |V|))))

and the position probes to bit equality: every term but one is an exact zero, so a wrong k-slot,
a mis-turned patch of the mirror product or an edge tile masked a column late or early changes
the result outright.  The entry fills every padding column, the slab workspace and the result
with NaNs first, so anything outside the matrix that reaches an accumulator shows as well.

Sizes: 129 (two 128-tiles, the second with one row; fewer 32-column chunks than waves), 255 /
256 / 257 (tile boundary), 383 (n mod 32 = 31, n mod 16 != 0), 512 (pitch 528), 640 (interior),
1153 (ten tiles per side: the reduce takes its second batch of eight slabs)."""

import ctypes
import functools

import numpy as np
import pytest

import _krylov_ref as kr
from spectralcluster_amd import _lib

pytestmark = pytest.mark.gpu

SYM, TWO, GROUPED = 1, 2, 4
ROUTES = {"plain": 0, "sym": SYM}
_DP = ctypes.POINTER(ctypes.c_double)


def block_operator(handle, problems, route):
  """problems: dicts with m (n, n), v (n, 8) and optional c, p, s -- or None for an idle member.
  Returns the list of W (n, 8) (None for idle members)."""
  count = len(problems)
  ns = (ctypes.c_int32 * count)()
  arrays = {k: (_DP * count)() for k in ("m", "c", "p", "s", "v", "w")}
  keep, out = [], []
  for z, pr in enumerate(problems):
    if pr is None:
      out.append(None)
      continue
    n = pr["m"].shape[0]
    ns[z] = n
    w = np.full((n, kr.B), np.nan)
    out.append(w)
    for key, a in (("m", pr["m"]), ("c", pr.get("c")), ("p", pr.get("p")), ("s", pr.get("s")),
                   ("v", pr["v"]), ("w", w)):
      if a is None:
        continue
      a = a if key == "w" else np.ascontiguousarray(a, dtype=np.float64)
      keep.append(a)
      arrays[key][z] = _lib.as_double_p(a)
  handle.check(handle.lib.sc_stage_block_operator(
      handle.raw, count, ns, arrays["m"], arrays["c"], arrays["p"], arrays["s"], arrays["v"],
      arrays["w"], route))
  return out


def ratio(w, op, v):
  """Worst error / bound of the device result against the longdouble product."""
  assert np.all(np.isfinite(w)), "NaN padding or workspace reached the result"
  err = np.abs(w.astype(kr.LD) - op.apply_ld(v)).astype(np.float64)
  return float(np.max(err / op.bound(v)))


@functools.lru_cache(maxsize=None)
def _dense(n, seed, **kw):
  m, c, p, s, v = kr.dense_case(n, seed, **kw)
  return dict(m=m, c=c, p=p, s=s, v=v), kr.Operator(m, c, p, s)


# ------------------------------------------------------------------ (a) position probes
@pytest.mark.parametrize("n", kr.OPERATOR_SIZES)
def test_position_probes_bit_for_bit(handle, n):
  m = kr.probe_matrix(n)
  cols = kr.probe_columns(n)
  cols += cols[:(-len(cols)) % kr.B]
  for name, route in ROUTES.items():
    for k0 in range(0, len(cols), kr.B):
      ks = cols[k0:k0 + kr.B]
      v = np.zeros((n, kr.B))
      v[ks, np.arange(kr.B)] = 1.0
      w, = block_operator(handle, [dict(m=m, v=v)], route)
      bad = [(k, int(np.flatnonzero(w[:, j] != m[:, k])[0]))
             for j, k in enumerate(ks) if not np.array_equal(w[:, j], m[:, k])]
      assert not bad, "%s route, n=%d: (column, first wrong row) %s" % (name, n, bad)


# ------------------------------------------------------------------ (b) dense blocks
@pytest.mark.parametrize("n", kr.OPERATOR_SIZES)
def test_dense_block_within_bound(handle, n):
  worst = {}
  pr, op = _dense(n, 0)                               # symmetric, s = c
  for name, route in ROUTES.items():
    worst[name] = ratio(block_operator(handle, [pr], route)[0], op, pr["v"])
  pr, op = _dense(n, 1, symmetric=False, own_s=True)  # the general path's use: s != c
  worst["general"] = ratio(block_operator(handle, [pr], 0)[0], op, pr["v"])
  pr, op = _dense(n, 2, with_c=False, with_p=False)   # the NULL forms: c = 1, p = 0
  for name, route in ROUTES.items():
    worst["null-" + name] = ratio(block_operator(handle, [pr], route)[0], op, pr["v"])
  print("n=%d one product, worst error/bound:" % n,
        " ".join("%s %.3f" % kv for kv in worst.items()))
  assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------ (c) two products
@functools.lru_cache(maxsize=None)
def _two(n):
  a = kr.refined_affinity(n)
  _, c, p, _, v = kr.dense_case(n, 3)
  return dict(m=a, c=c, p=p, v=v), kr.Operator(a, c, p, two=True)


@pytest.mark.parametrize("n", kr.TWO_PRODUCT_SIZES)
def test_two_product_within_bound(handle, n):
  pr, op = _two(n)
  worst = {name: ratio(block_operator(handle, [pr], route | TWO)[0], op, pr["v"])
           for name, route in ROUTES.items()}
  print("n=%d two products, worst error/bound:" % n,
        " ".join("%s %.3f" % kv for kv in worst.items()))
  assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------ (d) one grouped launch
@pytest.mark.parametrize("name", list(ROUTES))
def test_grouped_launch(handle, name):
  route = ROUTES[name]
  members = [None if n == 0 else _dense(n, 10 + z) for z, n in enumerate(kr.GROUP_SIZES)]
  ws = block_operator(handle, [mb and mb[0] for mb in members], route | GROUPED)
  worst = []
  for z, mb in enumerate(members):
    if mb is None:
      assert ws[z] is None
      continue
    pr, op = mb
    worst.append(ratio(ws[z], op, pr["v"]))
    single, = block_operator(handle, [pr], route)
    assert np.array_equal(ws[z], single), "member %d (n=%d) differs from its single launch" % (
        z, kr.GROUP_SIZES[z])
  print("grouped %s, members n=%s, worst error/bound per member: %s" % (
      name, [n for n in kr.GROUP_SIZES if n], " ".join("%.3f" % r for r in worst)))
  assert max(worst) <= 1.0


def test_grouped_two_product_equals_single(handle):
  members = [_two(257), None, _two(640)]
  for name, route in ROUTES.items():
    ws = block_operator(handle, [mb and mb[0] for mb in members], route | TWO | GROUPED)
    for z, mb in enumerate(members):
      if mb is None:
        continue
      pr, op = mb
      assert ratio(ws[z], op, pr["v"]) <= 1.0
      single, = block_operator(handle, [pr], route | TWO)
      assert np.array_equal(ws[z], single), (name, z)


def test_rejects_bad_requests(handle):
  m, v = np.eye(4), np.zeros((4, kr.B))
  with pytest.raises(ValueError):
    block_operator(handle, [dict(m=m, v=v), None], 0)       # idle member outside a group
  with pytest.raises(ValueError):
    block_operator(handle, [dict(m=m, v=v)], 8)             # unknown route bit
  with pytest.raises(ValueError):
    block_operator(handle, [dict(m=m, v=v)] * 17, GROUPED)  # more than a group holds
