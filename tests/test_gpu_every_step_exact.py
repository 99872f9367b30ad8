"""Exact-arithmetic tests of the kernels that run on EVERY optimizer step: the float32 grouped
product and its plans (csrc/misc.hip), the statistics update (csrc/stats.hip) and the fused
_transform_grad (csrc/transform.hip).

Method (tests/_exact.py): small-integer operands make every product and partial sum exactly
representable in float32, so the result is independent of summation order, tile shape, split
count and MFMA accumulation order; the expectation is the int64 product and the assertion is
array_equal.  Precondition, asserted per case: max(|A| @ |B|) < 2^24 (|a|, |b| <= 8, k <= 50 000).
For the statistics w1, w2 in {0, 0.5, 1, 2} and an integer `old` keep the axpby exact too.

Beside every exact family one N(0, 1) case is compared with float64 under the derived bound
|c - ref| <= (k + ksplit_max + 2) u (|A| @ |B|), u = 2^-24, valid for any summation order (it
guards against a reduced-precision path taken by mistake, which integers would hide).

The fused transform is compared (a) on inputs whose norms are exact integers, with the
multiplier known a priori, to 2 ulp (one correctly rounded division and one multiplication by
lr), and (b) with the float64 restatement _exact.transform_ref64 -- pinned to the package's torch
restatement and thereby to the reference's goldens in test_every_step_references.py -- under
|got - ref| <= (D + 16) u magnitude, D = _exact.norm_depth (the summation depth of the kernel's
norms; 16 covers the elementwise roundings of pass C).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _exact as E
from tests.test_every_step_references import VARIANTS, variant_cfg

pytestmark = pytest.mark.gpu

SENT = -777.25   # sentinel: no integer (or half-integer) result can equal it


def K():
  from precondition_amd import kernels
  return kernels


def _lib():
  from precondition_amd import _lib as L
  return L.lib()


def _stream():
  return torch.cuda.current_stream().cuda_stream


def _assert_equal(got, exp, what):
  got, exp = np.asarray(got), np.asarray(exp)
  assert got.shape == exp.shape, (what, got.shape, exp.shape)
  if not np.array_equal(got, exp):
    bad = np.argwhere(got != exp)
    first = tuple(bad[0])
    raise AssertionError(
        f"{what}: {len(bad)} of {got.size} elements differ; first at {first}: got {got[first]!r}, "
        f"expected {exp[first]!r}; rows {bad[:, 0].min()}..{bad[:, 0].max()}"
        + (f", cols {bad[:, 1].min()}..{bad[:, 1].max()}" if bad.shape[1] > 1 else ""))


# ---------------------------------------------------------------------------
# 1. grouped float32 product, plans, ps_gemm_f32
# ---------------------------------------------------------------------------
def _stored(x, trans, dev, ld_pad=0, offset=0):
  """Device view of the matrix as stored (x^T when trans) with leading dimension cols + ld_pad,
  `offset` floats into a sentinel-filled buffer."""
  s = np.ascontiguousarray(x.T if trans else x).astype(np.float32)
  r, c = s.shape
  ld = c + ld_pad
  buf = torch.full((offset + r * ld,), SENT, dtype=torch.float32, device=dev)
  view = buf[offset:offset + r * ld].view(r, ld)[:, :c]
  view.copy_(torch.from_numpy(s).to(dev))
  return view


def _fails_vec(t):
  """The library's 16-byte test on a 2-D operand view (pointer and leading dimension)."""
  ld = t.stride(0) if t.shape[0] > 1 else max(int(t.shape[1]), 1)
  return t.data_ptr() % 16 != 0 or ld % 4 != 0


def _aligned_pad(cols):
  return (-cols) % 4


def _odd_pad(cols):
  return (1 - cols) % 4   # (cols + pad) % 4 == 1


@functools.lru_cache(maxsize=None)
def _int_case(m, n, k, salt):
  rng = np.random.default_rng(1000 + salt)
  a = E.int_operand(rng, m, k, salt)       # pattern for even salts ...
  b = E.int_operand(rng, k, n, salt + 1)   # ... then random, and the other way round
  E.assert_exact(E.product_abs_bound(a, b))
  return a, b, E.int_matmul(a, b)


def _framed(m, n, dev):
  """(holder, view): an m x n output as a strided view (ldc = n + 3) of a sentinel-filled holder."""
  holder = torch.full((m + 2, n + 3), SENT, dtype=torch.float32, device=dev)
  return holder, holder[1:m + 1, 2:n + 2]


def _check_framed(holder, ref, what):
  m, n = ref.shape
  exp = np.full((m + 2, n + 3), SENT, np.float64)
  exp[1:m + 1, 2:n + 2] = ref
  _assert_equal(holder.cpu().numpy().astype(np.float64), exp, what)


def _normal_bound(a, b, k):
  """(float64 product, element-wise bound) of float32 operands: any summation order of k products
  plus the split-K reduction stays within (k + ksplit_max + 2) u (|A| @ |B|)."""
  a64, b64 = a.astype(np.float64), b.astype(np.float64)
  return a64 @ b64, (k + E.KSPLIT_MAX + 2) * E.U * (np.abs(a64) @ np.abs(b64))


@pytest.mark.parametrize("transa,transb", E.GEMM_LAYOUTS)
def test_grouped_product_split_k_exact(transa, transb, device):
  """Single-task calls (total tiles < 512, k >= 512: the split is taken) on every layout, with c a
  strided view: every k remainder of the list, short last splits, one-row and one-column outputs."""
  plans = E.check_split_list()
  assert {p[0] % 4 for p in plans} == {0, 1, 2, 3}
  salt = 0
  for (m, n) in E.GEMM_MN:
    for k in E.GEMM_KS:
      salt += 1
      ksplit, kchunk, last = E.split_plan(E.tiles_of(m, n), k)
      assert ksplit > 1
      a, b, ref = _int_case(m, n, k, salt)
      holder, c = _framed(m, n, device)
      K().gemm_grouped([(_stored(a, transa, device), _stored(b, transb, device), c, transa, transb)])
      _check_framed(holder, ref, f"m {m} n {n} k {k} ta {transa} tb {transb} "
                                 f"ksplit {ksplit} kchunk {kchunk} last {last}")
  # contiguous c (ldc == n) with a split, and the N(0, 1) companion under the derived bound
  a, b, ref = _int_case(128, 128, 4096, 2)
  c = torch.full((128, 128), SENT, device=device)
  K().gemm_grouped([(_stored(a, transa, device), _stored(b, transb, device), c, transa, transb)])
  _assert_equal(c.cpu().numpy().astype(np.int64), ref, "contiguous c")
  rng = np.random.default_rng(5)
  m, n, k = 129, 257, 4100
  a = rng.standard_normal((m, k)).astype(np.float32)
  b = rng.standard_normal((k, n)).astype(np.float32)
  ref, bound = _normal_bound(a, b, k)
  holder, c = _framed(m, n, device)
  K().gemm_grouped([(_stored(a, transa, device), _stored(b, transb, device), c, transa, transb)])
  err = np.abs(c.cpu().numpy().astype(np.float64) - ref)
  print(f"split-K N(0,1) ta {transa} tb {transb}: worst err / bound {np.max(err / bound):.4f}")
  assert (err <= bound).all()


@pytest.mark.parametrize("transa,transb", E.GEMM_LAYOUTS)
def test_grouped_product_split_k_unaligned_operands(transa, transb, device):
  """Operands that fail the 16-byte test (pointer one float off, or a leading dimension that is not
  a multiple of 4) together with split-K: the guarded loads at k offsets k0 and k0 * ld."""
  salt = 40
  for (m, n, k) in ((128, 128, 1000), (129, 257, 4100), (1, 200, 1153), (96, 33, 1800)):
    assert E.split_plan(E.tiles_of(m, n), k)[0] > 1
    a, b, ref = _int_case(m, n, k, salt)
    salt += 1
    for a_bad, b_bad in ((True, False), (False, True), (True, True)):
      for kind in ("offset", "ld"):
        def put(x, trans, bad):
          cols = x.shape[0] if trans else x.shape[1]
          if not bad:
            return _stored(x, trans, device, _aligned_pad(cols), 0)
          if kind == "offset":
            return _stored(x, trans, device, _aligned_pad(cols), 1)
          return _stored(x, trans, device, _odd_pad(cols), 0)
        ta, tb = put(a, transa, a_bad), put(b, transb, b_bad)
        assert (_fails_vec(ta) or not a_bad) and (_fails_vec(tb) or not b_bad)
        holder, c = _framed(m, n, device)
        K().gemm_grouped([(ta, tb, c, transa, transb)])
        _check_framed(holder, ref, f"m {m} n {n} k {k} ta {transa} tb {transb} a_bad {a_bad} "
                                   f"b_bad {b_bad} {kind}")


def _mixed_tasks():
  # (row0, col0, m, n, k, transa, transb) inside one 302 x 203 tensor
  return [(0, 0, 128, 128, 4096, True, False), (128, 0, 172, 72, 1000, True, False),
          (0, 128, 128, 72, 209, True, False), (300, 0, 1, 200, 640, False, False),
          (301, 0, 1, 64, 64, True, False), (128, 80, 96, 33, 512, False, True),
          (128, 120, 60, 50, 300, False, True)]


def test_grouped_product_mixed_call_exact(device):
  """One call: tasks that split and tasks with k < 512, a one-row task that splits (and so leaves
  the mat-vec path) and one that does not, two layouts, all outputs blocks of one tensor."""
  tasks = _mixed_tasks()
  total = sum(E.tiles_of(t[2], t[3]) for t in tasks)
  splits = [E.split_plan(total, t[4])[0] for t in tasks]
  assert [s > 1 for s in splits] == [True, True, False, True, False, True, False], splits
  rng = np.random.default_rng(9)
  for normal in (False, True):
    big = torch.full((302, 203), SENT, dtype=torch.float32, device=device)
    exp = np.full((302, 203), SENT, np.float64)
    bnd = np.zeros((302, 203))
    items = []
    for i, (r0, c0, m, n, k, ta, tb) in enumerate(tasks):
      if normal:
        a = rng.standard_normal((m, k)).astype(np.float32)
        b = rng.standard_normal((k, n)).astype(np.float32)
        ref, bound = _normal_bound(a, b, k)
        bnd[r0:r0 + m, c0:c0 + n] = bound
      else:
        a, b, ref = _int_case(m, n, k, 60 + i)
      exp[r0:r0 + m, c0:c0 + n] = ref
      items.append((_stored(a, ta, device), _stored(b, tb, device), big[r0:r0 + m, c0:c0 + n], ta, tb))
    K().gemm_grouped(items)
    got = big.cpu().numpy().astype(np.float64)
    if normal:
      assert (np.abs(got - exp) <= bnd).all()
    else:
      _assert_equal(got, exp, "mixed call")


def test_grouped_product_above_the_tile_threshold_exact(device):
  """529 tiles, k = 4096: the other side of the split threshold (no split, fast interior tiles)."""
  m = n = 23 * 128
  k = 4096
  assert E.tiles_of(m, n) >= 512 and E.split_plan(E.tiles_of(m, n), k)[0] == 1
  assert E.split_plan(511, k)[0] > 1
  a, b, ref = E.int_pattern(m, k, 3), E.int_random(np.random.default_rng(3), (k, n)), None
  E.assert_exact(64 * k)
  ref = E.int_matmul(a, b)
  holder, c = _framed(m, n, device)
  K().gemm_grouped([(_stored(a, True, device), _stored(b, False, device), c, True, False)])
  _check_framed(holder, ref, "529 tiles, k 4096")


def test_gemm_plan_relaunch_after_operands_changed(device):
  """ps_gemm_grouped_plan_*: operand CONTENTS may change between launches, the partials in the
  workspace are reused; two plans alive at once do not disturb each other."""
  k = 4096
  shapes = [(128, 128, False, False), (96, 33, True, False), (1, 200, False, True)]

  def fresh(salt0):
    ops = []
    for i, (m, n, ta, tb) in enumerate(shapes):
      a, b, ref = _int_case(m, n, k, salt0 + i)
      ops.append((a, b, ref))
    return ops

  def build(ops):
    items, holders = [], []
    for (a, b, _), (m, n, ta, tb) in zip(ops, shapes):
      holder, c = _framed(m, n, device)
      items.append((_stored(a, ta, device), _stored(b, tb, device), c, ta, tb))
      holders.append(holder)
    return K().GemmPlan(items), items, holders

  def check(holders, ops, what):
    for h, (_, _, ref) in zip(holders, ops):
      _check_framed(h, ref, what)

  total = sum(E.tiles_of(m, n) for m, n, _, _ in shapes)
  assert E.split_plan(total, k)[0] > 1
  ops1, ops2, ops3 = fresh(80), fresh(90), fresh(100)
  plan_a, items_a, hold_a = build(ops1)
  plan_b, items_b, hold_b = build(ops3)     # a second plan on its own workspace
  plan_a.launch()
  plan_b.launch()
  check(hold_a, ops1, "plan a, first launch")
  check(hold_b, ops3, "plan b, first launch")
  for (ta_, tb_, _, ta, tb), (a, b, _) in zip(items_a, ops2):   # overwrite the operands in place
    ta_.copy_(torch.from_numpy(np.ascontiguousarray(a.T if ta else a).astype(np.float32)).to(device))
    tb_.copy_(torch.from_numpy(np.ascontiguousarray(b.T if tb else b).astype(np.float32)).to(device))
  plan_a.launch()
  check(hold_a, ops2, "plan a, second launch after the operands changed")
  second = [h.clone() for h in hold_a]
  plan_b.launch()
  plan_a.launch()
  for h, s in zip(hold_a, second):
    assert torch.equal(h, s)
  check(hold_b, ops3, "plan b after plan a relaunched")
  del plan_a, plan_b


def _flat_batched(x, ld, stride):
  """x [batch, rows, cols] -> flat float32 array, item b at b * stride, rows `ld` apart; the rest
  is the sentinel."""
  batch, rows, cols = x.shape
  buf = np.full(batch * stride, SENT, np.float32)
  for b in range(batch):
    buf[b * stride:b * stride + rows * ld].reshape(rows, ld)[:, :cols] = x[b]
  return buf


def _stride_for(rows, ld, multiple_of_4):
  base = rows * ld
  extra = (-base) % 4 if multiple_of_4 else (1 - base) % 4
  return base + extra


@pytest.mark.parametrize("transa,transb", E.GEMM_LAYOUTS)
def test_gemm_f32_leading_dimensions_and_batches_exact(transa, transb, device):
  """ps_gemm_f32 through ctypes: batch 1 / 3 / 17, leading dimensions above the extent, batch
  strides that are and are not multiples of 4 (the guarded loads of a batched call); the frame
  between rows and between batch items of c stays untouched."""
  L = _lib()
  rng = np.random.default_rng(17)
  for (m, n, k) in ((1, 1, 1), (128, 128, 2), (200, 130, 77), (513, 65, 300)):
    for batch in (1, 3, 17):
      a = E.int_random(rng, (batch, m, k))
      a[0] = E.int_pattern(m, k, batch)
      b = E.int_random(rng, (batch, k, n))
      E.assert_exact(64 * k)
      ref = np.matmul(a.astype(np.float64), b.astype(np.float64))
      a_st = np.ascontiguousarray(a.transpose(0, 2, 1)) if transa else a
      b_st = np.ascontiguousarray(b.transpose(0, 2, 1)) if transb else b
      for pad in (0, 1, 4):
        for mult4 in (True, False):
          lda, ldb, ldc = a_st.shape[2] + pad, b_st.shape[2] + pad, n + pad
          sa = _stride_for(a_st.shape[1], lda, mult4)
          sb = _stride_for(b_st.shape[1], ldb, mult4)
          sc = _stride_for(m, ldc, mult4)
          da = torch.from_numpy(_flat_batched(a_st, lda, sa)).to(device)
          db = torch.from_numpy(_flat_batched(b_st, ldb, sb)).to(device)
          dc = torch.full((batch * sc,), SENT, dtype=torch.float32, device=device)
          rc = L.ps_gemm_f32(_stream(), int(transa), int(transb), da.data_ptr(), db.data_ptr(),
                             dc.data_ptr(), m, n, k, lda, ldb, ldc, batch, sa, sb, sc)
          assert rc == 0, rc
          exp = _flat_batched(ref, ldc, sc).astype(np.float64)
          _assert_equal(dc.cpu().numpy().astype(np.float64)[:, None], exp[:, None],
                        f"m {m} n {n} k {k} batch {batch} pad {pad} stride%4==0 {mult4}")
  # N(0, 1) companion (no split here: bound (k + 2) u |A||B|, inside the common one)
  m, n, k, batch = 200, 130, 77, 3
  a = rng.standard_normal((batch, m, k)).astype(np.float32)
  b = rng.standard_normal((batch, k, n)).astype(np.float32)
  ref = np.matmul(a.astype(np.float64), b.astype(np.float64))
  bound = (k + E.KSPLIT_MAX + 2) * E.U * np.matmul(np.abs(a).astype(np.float64), np.abs(b).astype(np.float64))
  a_st = np.ascontiguousarray(a.transpose(0, 2, 1)) if transa else a
  b_st = np.ascontiguousarray(b.transpose(0, 2, 1)) if transb else b
  lda, ldb, ldc = a_st.shape[2] + 1, b_st.shape[2] + 1, n + 1
  sa, sb, sc = a_st.shape[1] * lda + 1, b_st.shape[1] * ldb + 1, m * ldc + 1
  da = torch.from_numpy(_flat_batched(a_st, lda, sa)).to(device)
  db = torch.from_numpy(_flat_batched(b_st, ldb, sb)).to(device)
  dc = torch.full((batch * sc,), SENT, dtype=torch.float32, device=device)
  assert L.ps_gemm_f32(_stream(), int(transa), int(transb), da.data_ptr(), db.data_ptr(),
                       dc.data_ptr(), m, n, k, lda, ldb, ldc, batch, sa, sb, sc) == 0
  got = dc.cpu().numpy().astype(np.float64)
  for i in range(batch):
    blk = got[i * sc:i * sc + m * ldc].reshape(m, ldc)[:, :n]
    assert (np.abs(blk - ref[i]) <= bound[i]).all()


# ---------------------------------------------------------------------------
# 2. statistics update
# ---------------------------------------------------------------------------
W_PAIRS = [(1.0, 1.0), (0.5, 2.0), (2.0, 0.5), (0.0, 1.0), (1.0, 0.5), (0.5, 0.5)]


def _gram_int(x, axis):
  """tensordot(x, x, all axes but `axis`) of an integer array, exactly."""
  xm = np.moveaxis(x, axis, 0).reshape(x.shape[axis], -1)
  E.assert_exact(E.product_abs_bound(xm, xm.T))
  return E.int_matmul(xm, xm.T)


def _stats_expected(old, gram, w1, w2):
  E.assert_exact(abs(w1) * np.abs(old).max() + abs(w2) * np.abs(gram).max())
  return w1 * old.astype(np.float64) + w2 * gram.astype(np.float64)   # exact: multiples of 1/4


def _t(x, dev):
  return torch.from_numpy(np.ascontiguousarray(x).astype(np.float32)).to(dev)


def test_stats_update_nd_blocks_exact(device):
  """The N-d block list of tools/dev_fuzz_misc.py through BlockPartitioner, every axis: segment
  loops (nseg > 1), both operand layouts, strided block views."""
  from precondition_amd.blocking import BlockPartitioner
  rng = np.random.default_rng(3)
  cases = (((70, 33), 32), ((5, 6, 7), 4), ((3, 130, 9), 64), ((2, 3, 4, 5), 3), ((260,), 100),
           ((17, 1, 19), 8), ((1, 50), 16), ((4, 4, 4, 4, 4), 4))
  for ci, (shape, bs) in enumerate(cases):
    x = E.int_random(rng, shape) if ci % 2 else \
        E.int_pattern(int(np.prod(shape[:-1])), shape[-1], ci).reshape(shape)
    t = _t(x, device)
    parts = BlockPartitioner(t, bs).partition(t)
    xt = torch.from_numpy(x)
    parts_np = BlockPartitioner(xt, bs).partition(xt)
    w1, w2 = W_PAIRS[ci % len(W_PAIRS)]
    items, refs = [], []
    for blk, blk_np in zip(parts, parts_np):
      for axis in range(blk.dim()):
        d = blk.shape[axis]
        old = E.int_pattern(d, d, ci + axis)
        refs.append(_stats_expected(old, _gram_int(blk_np.numpy(), axis), w1, w2))
        items.append((blk, axis, _t(old, device), torch.full((d, d), SENT, device=device)))
    K().stats_update_grouped(items, w1, w2)
    for j, ((_, axis, _, new), ref) in enumerate(zip(items, refs)):
      _assert_equal(new.cpu().numpy().astype(np.float64), ref, f"shape {shape} bs {bs} item {j} axis {axis}")


STATS_D = [1, 127, 128, 129, 384, 513]
STATS_K = [1, 2, 15, 16, 17, 250, 256, 4096, 50000]


def _stats_buffers(kind, old_dev, d, dev):
  """(stat_in, stat_out, holder of stat_out | None) for one of the four placements."""
  if kind == "oop":
    return old_dev, torch.full((d, d), SENT, device=dev), None
  if kind == "inplace":
    s = old_dev.clone()
    return s, s, None
  hin = torch.full((d, d + 1), SENT, device=dev)
  hin[:, :d] = old_dev
  if kind == "inplace_ld":
    return hin[:, :d], hin[:, :d], hin
  hout = torch.full((d, d + 1), SENT, device=dev)
  return hin[:, :d], hout[:, :d], hout


def test_stats_update_grid_exact(device):
  """d x k grid on both axes: edge tiles, the guarded K loop at every remainder, the vector path
  (k = 1), mirrored tiles with a non-symmetric `old`; in place and out of place, aligned and with
  lds = d + 1; w1 = 0, w2 = 1 exactly symmetric; the single-statistic entry; and finally every
  case again in ONE grouped launch per weight pair, bit for bit equal to the per-item calls."""
  L = _lib()
  records = {}
  ci = 0
  for d in STATS_D:
    for k in STATS_K:
      x = E.int_pattern(d, k, ci) if ci % 2 == 0 else E.int_random(np.random.default_rng(ci), (d, k))
      gram = _gram_int(x, 0)
      old = E.int_pattern(d, d, ci + 1)
      assert d == 1 or not np.array_equal(old, old.T)
      old_dev = _t(old, device)
      for axis in (0, 1):
        ci += 1
        w1, w2 = W_PAIRS[ci % len(W_PAIRS)]
        g = _t(x if axis == 0 else x.T, device)
        ref = _stats_expected(old, gram, w1, w2)
        what = f"d {d} k {k} axis {axis} w ({w1}, {w2})"
        out = K().gram_weighted_update(old_dev, g, axis, w1, w2)
        _assert_equal(out.cpu().numpy().astype(np.float64), ref, what + " gram_weighted_update")
        for kind in ("oop", "inplace", "oop_ld", "inplace_ld"):
          sin, sout, holder = _stats_buffers(kind, old_dev, d, device)
          K().stats_update_grouped([(g, axis, sin, sout)], w1, w2)
          _assert_equal(sout.cpu().numpy().astype(np.float64), ref, what + " " + kind)
          if holder is not None:
            assert bool((holder[:, d] == SENT).all()), what + " " + kind + ": pad column written"
          assert torch.equal(sout, out)
          records.setdefault((w1, w2), []).append((g, axis, kind, old_dev, d, sout.clone()))
        # Gram part alone: exactly symmetric, whatever `old` holds
        sym = K().gram_weighted_update(old_dev, g, axis, 0.0, 1.0)
        assert torch.equal(sym, sym.T), what
        _assert_equal(sym.cpu().numpy().astype(np.int64), gram, what + " w (0, 1)")
        # the single-statistic entry of the C ABI
        rows, cols = int(g.shape[0]), int(g.shape[1])
        single = torch.full((d, d), SENT, device=device)
        rc = L.ps_stats_update_f32(_stream(), g.data_ptr(), rows, cols, cols, axis,
                                   old_dev.data_ptr(), single.data_ptr(), d, w1, w2)
        assert rc == 0, rc
        _assert_equal(single.cpu().numpy().astype(np.float64), ref, what + " ps_stats_update_f32")
  # every case at once: one launch per weight pair, mixed tasks
  for (w1, w2), recs in records.items():
    items, outs = [], []
    for (g, axis, kind, old_dev, d, _) in recs:
      sin, sout, _h = _stats_buffers(kind, old_dev, d, device)
      items.append((g, axis, sin, sout))
      outs.append(sout)
    K().stats_update_grouped(items, w1, w2)
    for sout, rec in zip(outs, recs):
      assert torch.equal(sout, rec[5]), (w1, w2, rec[1], rec[2], rec[4])


def test_stats_update_normal_inputs_derived_bound(device):
  """N(0, 1) companion: |S - ref| <= (k + 4) u (|w1 old| + |w2| |X| |X|^T): k - 1 additions and k
  products of the contraction in any order, the two products and the addition of the axpby."""
  rng = np.random.default_rng(21)
  w1, w2 = 0.75, 0.25
  for d, k in ((513, 250), (129, 4096)):
    x = rng.standard_normal((d, k)).astype(np.float32)
    old = rng.standard_normal((d, d)).astype(np.float32)
    x64 = x.astype(np.float64)
    ref = w1 * old.astype(np.float64) + w2 * (x64 @ x64.T)
    bound = (k + 4) * E.U * (np.abs(w1 * old.astype(np.float64)) + w2 * (np.abs(x64) @ np.abs(x64).T))
    for axis in (0, 1):
      g = _t(x if axis == 0 else x.T, device)
      got = K().gram_weighted_update(_t(old, device), g, axis, w1, w2).cpu().numpy().astype(np.float64)
      err = np.abs(got - ref)
      print(f"stats N(0,1) d {d} k {k} axis {axis}: worst err / bound {np.max(err / bound):.4f}")
      assert (err <= bound).all()


# ---------------------------------------------------------------------------
# 3. fused transform
# ---------------------------------------------------------------------------
NAMES = ("upd", "diag", "mom", "dmom")   # order of transform_grads_fused's result tuples


def _run_fused(items_np, cfg, dev):
  """kernels.transform_grads_fused on NumPy inputs -> per item dict name -> flat float32 array."""
  items = [{k: (None if v is None else _t(np.asarray(v).ravel(), dev)) for k, v in it.items()}
           for it in items_np]
  res = K().transform_grads_fused(items, cfg)
  torch.cuda.synchronize()
  return [{n: t.cpu().numpy().ravel() for n, t in zip(NAMES, r) if t is not None} for r in res]


def _worst_ratio_vs_ref64(items_np, cfg, dev, got=None):
  """Largest |got - ref| / ((D + 16) u magnitude) over every output of every parameter."""
  got = _run_fused(items_np, cfg, dev) if got is None else got
  worst = {"v": 0.0, "where": None}
  depth = [E.norm_depth(np.asarray(it["grad"]).size) for it in items_np]

  def consume(i, name, lo, hi, val, mag):
    assert name in got[i], (i, name)
    r = E.bound_ratio(got[i][name][lo:hi], val, mag, depth[i] + 16.0)
    if r > worst["v"]:
      worst["v"], worst["where"] = r, (i, name, lo)

  E.transform_ref64(items_np, cfg, consume=consume)
  for i, it in enumerate(items_np):   # the kernel returned the outputs the reference has
    assert ("diag" in got[i]) == E.has_diag(cfg["graft_type"])
    assert got[i]["upd"].size == np.asarray(it["grad"]).size
  return worst["v"], worst["where"]


PROBE_SIZES = [1, 4095, 4096, 4097, 8192, 256 * 4096, 256 * 4096 + 1, 1024 * 4096]


def _probe_item(n, dense_grad, skipped=False, diag=False):
  g, groot = E.exact_norm_vector(n, dense_grad, with_twos=not dense_grad)
  pg, proot = E.exact_norm_vector(n, not dense_grad, with_twos=dense_grad)
  z = np.zeros(n, np.float32)
  it = dict(grad=g.astype(np.float32), pgrad=None if skipped else pg.astype(np.float32), param=None,
            diag_in=z if diag else None, mom_in=z, dmom_in=z)
  return it, groot, proot


def _probe_expected(it, cfg):
  """The update of the norm probe in float32 scalars: -pgrad * (sqrt(r0) * lr) / (sqrt(r1) + 1e-25)
  with exact integer r0, r1 (sums of squares below 2^24; r0 = number of non-zeros for sqrt-n)."""
  g = it["grad"].astype(np.int64)
  r0 = int(np.count_nonzero(g)) if cfg["graft_type"] == E.G_SQRT_N else int(np.sum(g * g))
  assert r0 < E.EXACT_LIMIT
  lr = np.float32(cfg["lr"])
  gnorm = np.sqrt(np.float32(r0)) * lr
  base = np.sign(it["grad"]) if cfg["graft_type"] == E.G_SQRT_N else it["grad"]
  gu = base.astype(np.float32) * lr
  if it["pgrad"] is None:
    pg, pnorm = gu, gnorm
  else:
    p = it["pgrad"].astype(np.int64)
    r1 = int(np.sum(p * p))
    assert r1 < E.EXACT_LIMIT
    pg, pnorm = it["pgrad"], np.sqrt(np.float32(r1))
  mult = gnorm / (pnorm + E.T_EPS)
  assert isinstance(mult, np.float32)
  su = pg * mult
  return {"upd": -su, "mom": su, "dmom": gu}


def _check_probe(items, cfg, dev, what):
  """2 ulp: the multiplier is one correctly rounded product (sqrt(r0) is exact or correctly rounded,
  times lr) and one correctly rounded division; the products with +-1, +-2 are exact.  A lost or
  doubled 4096-element chunk moves the multiplier by >= 1 / (2 nchunks) ~ 5e-4 at 1024 chunks."""
  got = _run_fused(items, cfg, dev)
  for i, it in enumerate(items):
    exp = _probe_expected(it, cfg)
    for name, e in exp.items():
      g = got[i][name]
      assert g.shape == e.shape and np.isfinite(g).all(), (what, i, name)
      dist = E.ulp_distance(g, e)
      assert dist.max(initial=0) <= 2, (what, i, name, int(dist.max()), int(np.argmax(dist)),
                                        g[np.argmax(dist)], e[np.argmax(dist)])


def _mixed_probe_items(diag=False):
  spec = [(4097, True, False), (0, True, False), (1, False, True), (256 * 4096 + 1, False, False),
          (8192, True, True), (1024 * 4096, True, False), (4095, False, False),
          (256 * 4096, False, False), (0, False, False)]
  return [_probe_item(n, dense, skipped, diag)[0] for n, dense, skipped in spec]


@pytest.mark.parametrize("graft", [E.G_SGD, E.G_SQRT_N])
def test_transform_norm_probes_exact_multiplier(graft, device):
  """Per-parameter norms over 1 ... 1024 chunks with exactly known values: sizes at and around the
  chunk size and the 256-chunk stride of param_sum, non-zeros only in chunks 0 / 255 / 256 / 257 /
  511 / 512 / last (each a different count) or in every chunk; then one call mixing the sizes with
  two zero-element parameters (one in the middle, one last) and skipped parameters."""
  cfg = E.make_cfg(graft_type=graft)
  for n in PROBE_SIZES:
    for dense_grad in (True, False):
      it, groot, proot = _probe_item(n, dense_grad)
      assert groot > 0 and proot > 0
      _check_probe([it], cfg, device, f"graft {graft} n {n} dense_grad {dense_grad}")
  _check_probe(_mixed_probe_items(), cfg, device, f"graft {graft} mixed call")


@pytest.mark.parametrize("graft", [E.G_ADAGRAD, E.G_RMSPROP, E.G_RMSPROP_N, E.G_ADAGRAD_N])
def test_transform_norm_probes_diagonal_grafting(graft, device):
  """The slab[.][2] norm of the Adagrad / RMSProp branch on the probe sizes: diag_in = 0 and
  gradients in {0, +-1, +-2}; expected values from the float64 restatement, bound (D + 16) u."""
  cfg = E.make_cfg(graft_type=graft, beta2_w1=0.9, beta2_w2=0.1, clip_by_scaled_gradient_norm=0.3)
  for n in PROBE_SIZES:
    if n > 8192:
      continue   # the sizes above 256 chunks are in the mixed call below (host time of the reference)
    it = _probe_item(n, n % 2 == 0, diag=True)[0]
    worst, where = _worst_ratio_vs_ref64([it], cfg, device)
    assert worst <= 1.0, (graft, n, worst, where)
  mixed = _mixed_probe_items(diag=True)
  assert {256 * 4096, 256 * 4096 + 1, 1024 * 4096} <= {it["grad"].size for it in mixed}
  worst, where = _worst_ratio_vs_ref64(mixed, cfg, device)
  print(f"transform probes graft {graft}: mixed call worst ratio {worst:.3f}")
  assert worst <= 1.0, (graft, worst, where)


def _normal_item(rng, n, skipped=False):
  f = lambda: rng.standard_normal(n).astype(np.float32)   # noqa: E731
  return dict(grad=f(), pgrad=None if skipped else f(), param=f(), diag_in=np.square(f()),
              mom_in=f(), dmom_in=f())


def _for_cfg(items, cfg):
  """Drops the inputs a configuration does not take (the wrapper derives diag from diag_in)."""
  out = []
  for it in items:
    it = dict(it)
    if not E.has_diag(cfg["graft_type"]):
      it["diag_in"] = None
    if cfg["weight_decay"] == 0.0:
      it["param"] = None
    out.append(it)
  return out


TREE = [(1048577, False), (9000, False), (24, True), (1, False), (0, False), (4097, True)]


@pytest.mark.parametrize("graft", [0, 1, 2, 3, 4, 5, 6])
def test_transform_vs_float64_restatement(graft, device):
  """Every output of the fused transform against _exact.transform_ref64 for the three option
  variants of test_fused_transform_grad_vs_elementwise_restatement x run_shampoo in {0, 1}.
  Bound, derived: |got - ref| <= (D + 16) u magnitude; D = norm_depth(numel) is the summation depth
  of the kernel's per-parameter norm (every addend non-negative, so each norm is within (D + 1) u
  relative), 16 covers the elementwise roundings of pass C; `magnitude` is the formula with every
  addend replaced by its absolute value.

  Worst observed |got - ref| / bound on an MI355X, grafting types 0 ... 6 (1 048 577-element tree):
  0.083, 0.080, 0.092, 0.086, 0.082, 0.083, 0.084; the 38 597 376-element case below: 0.048."""
  rng = np.random.default_rng(graft)
  items = [_normal_item(rng, n, sk) for n, sk in TREE]
  worst_all = 0.0
  for variant in range(len(VARIANTS)):
    for run in (0, 1):
      cfg = variant_cfg(graft, variant, run)
      worst, where = _worst_ratio_vs_ref64(_for_cfg(items, cfg), cfg, device)
      worst_all = max(worst_all, worst)
      assert worst <= 1.0, (graft, variant, run, worst, where)
  print(f"transform vs float64, graft {graft}: worst |got - ref| / bound = {worst_all:.3f}")


def test_transform_vs_float64_restatement_production_embedding(device):
  """A 50 257 x 768 embedding (38 597 376 elements, 9423 chunks: param_sum's loop runs 37 times per
  thread), once: SGD grafting with weight decay and the moving-average momentum, run_shampoo = 1.
  The other grafting types run at 1 048 577 elements above (this one case costs as much host time
  as all of them together)."""
  n = 50257 * 768
  gen = torch.Generator(device=device)
  gen.manual_seed(7)
  dev_items = {k: torch.randn(n, generator=gen, device=device, dtype=torch.float32)
               for k in ("grad", "pgrad", "param", "mom_in", "dmom_in")}
  small = _normal_item(np.random.default_rng(8), 9000)
  cfg = variant_cfg(E.G_SGD, 1, 1)
  items_np = _for_cfg([{**{k: v.cpu().numpy() for k, v in dev_items.items()}, "diag_in": None}, small], cfg)
  dev_list = [{**dev_items, "diag_in": None},
              {k: (None if v is None else _t(v, device)) for k, v in items_np[1].items()}]
  res = K().transform_grads_fused(dev_list, cfg)
  torch.cuda.synchronize()
  got = [{nm: t.cpu().numpy().ravel() for nm, t in zip(NAMES, r) if t is not None} for r in res]
  del res, dev_items, dev_list
  worst, where = _worst_ratio_vs_ref64(items_np, cfg, device, got=got)
  print(f"transform vs float64, 38 597 376 elements (D = {E.norm_depth(n)}): worst ratio {worst:.3f}")
  assert worst <= 1.0, (worst, where)


@pytest.mark.parametrize("graft", [1, 2, 3, 4, 5, 6])
def test_transform_zero_gradient_gives_zero_update(graft, device):
  rng = np.random.default_rng(graft)
  items = []
  for n in (1, 4097, 70000):
    it = _normal_item(rng, n)
    it["grad"] = np.zeros(n, np.float32)
    it["mom_in"] = np.zeros(n, np.float32)
    it["dmom_in"] = np.zeros(n, np.float32)
    it["diag_in"] = np.zeros(n, np.float32)
    items.append(it)
  for variant in (0, 2):   # variant 1's coupled weight decay adds wd * param by design
    cfg = dict(variant_cfg(graft, variant, 1), weight_decay=0.0)
    got = _run_fused(_for_cfg(items, cfg), cfg, device)
    for g in got:
      for name, v in g.items():
        assert np.isfinite(v).all() and not v.any(), (graft, variant, name)


class _NoFusedBackend:
  """The HIP kernels minus transform_grads_fused: the optimizer's float32 torch restatement."""

  def __getattr__(self, name):
    if name == "transform_grads_fused":
      raise AttributeError(name)
    return getattr(K(), name)


def test_transform_zero_preconditioned_gradient_nonfinite_pattern(device):
  """All-zero preconditioned gradient with a non-zero gradient: multiplier = ||g|| / 1e-25.  For an
  ordinary gradient that is finite and the update 0 * big = 0; for a gradient of norm ~1e17 it
  overflows and 0 * inf = NaN.  The pattern of non-finite values must be that of the float32 torch
  restatement (zeroed preconditioners give both paths pgrad = 0)."""
  import precondition_amd as pa
  rng = np.random.default_rng(31)
  shapes = [(40, 24), (64,), (24, 40)]
  params = [_t(rng.standard_normal(s), device) for s in shapes]
  kw = dict(graft_type=pa.GraftingType.SGD, start_preconditioning_step=1,
            preconditioning_compute_steps=1000, beta1=0.0)
  opts = [pa.distributed_shampoo(0.05, 32, **kw),
          pa.distributed_shampoo(0.05, 32, _backend_for_testing=_NoFusedBackend(), **kw)]
  g1 = [_t(rng.standard_normal(s), device) for s in shapes]
  g2 = [_t(rng.standard_normal(s), device) for s in shapes]
  g2[2] = g2[2] * 1e15
  ups = []
  for opt in opts:
    st = opt.init(params)
    _, st = opt.update(g1, st, params)
    assert int(st.count) == 1
    zeroed = [s._replace(preconditioners=[torch.zeros_like(p) for p in s.preconditioners])
              for s in st.stats]
    assert all(len(s.preconditioners) > 0 for s in zeroed)
    st = type(st)(count=st.count, stats=zeroed)
    up, st = opt.update(g2, st, params)
    ups.append(up)
  for i, (a, b) in enumerate(zip(*ups)):
    assert torch.equal(torch.isnan(a), torch.isnan(b)), i
    assert torch.equal(torch.isinf(a), torch.isinf(b)), i
    fin = torch.isfinite(b)
    assert torch.equal(a[fin], b[fin]) or (a[fin] - b[fin]).norm() <= 2e-6 * b[fin].norm() + 1e-12
  assert bool(torch.isfinite(ups[0][0]).all()) and not bool(ups[0][0].any())   # 0 * big = 0
  assert bool(torch.isnan(ups[0][2]).all())                                      # 0 * inf


def _transform_direct(arrs, cfg, ws):
  """ps_transform_grads_f32 on explicit descriptors (device tensors; outputs given by the caller)."""
  from precondition_amd._lib import TransformConfig, TransformDesc
  L = _lib()
  n = len(arrs)
  descs = (TransformDesc * n)()
  for d, a in zip(descs, arrs):
    for name in ("grad", "pgrad", "param", "diag_in", "diag_out", "mom_in", "mom_out", "dmom_in",
                 "dmom_out", "upd_out"):
      t = a.get(name)
      setattr(d, name, None if t is None or t.numel() == 0 else t.data_ptr())
    d.numel = a["grad"].numel()
  c = TransformConfig()
  for k, v in cfg.items():
    setattr(c, k, v)
  need = L.ps_transform_grads_workspace_bytes(descs, n)
  assert ws.numel() >= need, (ws.numel(), need)
  rc = L.ps_transform_grads_f32(_stream(), descs, n, C.byref(c), ws.data_ptr(), ws.numel())
  assert rc == 0, rc
  torch.cuda.synchronize()


def _direct_arrays(sizes, dev, seed, alias):
  rng = np.random.default_rng(seed)
  arrs = []
  for i, n in enumerate(sizes):
    it = _normal_item(rng, n, skipped=(i == 1))
    a = {k: (None if v is None else _t(v, dev)) for k, v in it.items()}
    if alias:
      a.update(upd_out=a["grad"], mom_out=a["mom_in"], dmom_out=a["dmom_in"], diag_out=a["diag_in"])
    else:
      for name in ("upd_out", "mom_out", "dmom_out", "diag_out"):
        a[name] = torch.full((n,), SENT, device=dev)
    arrs.append(a)
  return arrs


OUTS = ("upd_out", "mom_out", "dmom_out", "diag_out")


def test_transform_outputs_may_alias_inputs(device):
  """upd_out / mom_out / dmom_out / diag_out aliasing grad / mom_in / dmom_in / diag_in of the same
  parameter (allowed by ps_api.h): bit for bit the non-aliased call."""
  sizes = [9000, 4097, 1, 70000, 0]
  ws = torch.zeros(1 << 20, dtype=torch.uint8, device=device)
  for graft, variant in ((E.G_RMSPROP_N, 1), (E.G_SGD, 2), (E.G_ADAGRAD, 0)):
    cfg = variant_cfg(graft, variant, 1)
    plain = _direct_arrays(sizes, device, 5, alias=False)
    alias = _direct_arrays(sizes, device, 5, alias=True)
    _transform_direct(plain, cfg, ws)
    _transform_direct(alias, cfg, ws)
    for p, a in zip(plain, alias):
      for name in OUTS:
        if name == "diag_out" and not E.has_diag(graft):
          continue
        assert torch.equal(p[name], a[name]), (graft, variant, name, p["grad"].numel())
        assert not bool((p[name] == SENT).any())


def test_transform_workspace_reuse_with_other_sizes(device):
  """A second call on the same workspace with other sizes (stale slab and descriptor contents), and
  one on a workspace full of NaN bit patterns, equal a call on a zeroed one."""
  cfg = variant_cfg(E.G_RMSPROP_N, 1, 1)
  ws = torch.zeros(1 << 20, dtype=torch.uint8, device=device)
  _transform_direct(_direct_arrays([50000, 3, 12289], device, 1, alias=False), cfg, ws)
  sizes = [4097, 9000, 24, 0, 8192]
  stale = _direct_arrays(sizes, device, 2, alias=False)
  _transform_direct(stale, cfg, ws)
  fresh = _direct_arrays(sizes, device, 2, alias=False)
  _transform_direct(fresh, cfg, torch.zeros(1 << 20, dtype=torch.uint8, device=device))
  nans = _direct_arrays(sizes, device, 2, alias=False)
  _transform_direct(nans, cfg, torch.full((1 << 20,), 0xFF, dtype=torch.uint8, device=device))
  for f, s, q in zip(fresh, stale, nans):
    for name in OUTS:
      assert torch.equal(f[name], s[name]) and torch.equal(f[name], q[name]), name
      assert bool(torch.isfinite(f[name]).all())
