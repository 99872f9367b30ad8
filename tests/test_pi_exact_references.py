"""CPU gate of test_gpu_pi_exact.py: the float64 reference, the bounds and the case lists of
tests/_pi_exact.py are checked here against the float32 oracle (oracle.shampoo_oracle.power_iteration,
the reference's loop statement by statement), without a GPU.  The oracle is one more float32
evaluation in an order of its own (NumPy's einsum), so it has to satisfy the same order-independent
bounds as the kernels; a bound that the oracle misses is wrong, and a stop-rule case without a
margin never reaches the GPU file."""
import numpy as np
import pytest

from oracle import shampoo_oracle as orc
from tests import _pi_exact as P


def one_step_cases():
  cases = [c for b in P.DENSE_BATCHES + P.PROBE_BATCHES for c in b]
  return ([(k, n, None) for k, n in cases] + [c for c in P.PAD_CASES if c[2] > 0] +
          list(P.OUT_V_CASES) + [("sym", 300, 128)])


def assert_within(tag, lam, vec, ref, es, bv):
  assert abs(float(lam) - ref.lam) <= es, (tag, float(lam), ref.lam, es)
  bad = P.first_mismatch(vec, ref.vec, bv)
  assert bad is None, (tag, "first mismatch (row, tile, error, bound)", bad)


def test_one_step_oracle_within_bounds():
  worst = 0.0
  for kind, n, pad in one_step_cases():
    ref = P.one_step_ref(kind, n, pad)
    es, bv = P.one_step_bounds(kind, ref)
    a = P.matrix(kind, n)
    if pad is not None:   # the reference's padding is zero
      a = a.copy()
      a[pad:, :] = 0
      a[:, pad:] = 0
    v, s, it = orc.power_iteration(a, num_iters=1, error_tolerance=0.0, padding_start=pad)
    assert it == ref.iters == 1
    n_eff = n if pad is None else pad
    assert_within((kind, n, pad), s, v[:n_eff], ref, es, bv)
    assert not np.any(v[n_eff:])
    worst = max(worst, abs(float(s) - ref.lam) / es, P.ratio(v[:n_eff], ref.vec, bv))
  assert worst < 1.0
  print(f"oracle one-step error / bound, worst: {worst:.3g}")


def test_single_defect_oracle_within_bounds():
  cases = [(n, i, j, n) for n, i, j, _ in P.DEFECT_CASES]
  n, pad, i, j = P.DEFECT_BEHIND_PADDING
  for n, i, j, pad in cases + [(n, i, j, pad)]:
    a = P.single_defect(n, i, j)
    ref = P.reference64(a, pad, 1, 0.0)
    a[pad:, :] = 0
    a[:, pad:] = 0
    v, s, it = orc.power_iteration(a, num_iters=1, error_tolerance=0.0, padding_start=pad)
    assert it == 1
    assert_within((n, i, j, pad), s, v[:pad], ref, *P.dense_bounds(ref))


def test_all_padding_block():
  ref = P.reference64(P.matrix("sym", 300), 0, 1, 0.0)
  v, s, it = orc.power_iteration(np.zeros((4, 4), np.float32), num_iters=1, padding_start=0)
  assert np.isnan(ref.lam) and ref.iters == 1 and np.isnan(s) and it == 1


def test_probe_matvec_is_exact_in_float32():
  """A v in float32 (NumPy's order) equals the float64 product rounded once, bit for bit, for the
  one-step probes and the dominant-fixed-point ones."""
  mats = [P.matrix(k, n) for b in P.PROBE_BATCHES for k, n in b]
  mats += [P.stop_case(k, n, tol)[0] for b, tol in P.STOP_BATCHES for k, n in b]
  for a in mats:
    n = a.shape[0]
    assert (np.count_nonzero(a, axis=0) <= 1).all() and (np.count_nonzero(a, axis=1) <= 1).all()
    nz = np.abs(a[a != 0])
    assert np.array_equal(np.log2(nz), np.round(np.log2(nz))) and nz.max() <= 4
    v = P.v0_f32(n)
    v = v / np.linalg.norm(v)
    for x in (a, a.T):
      want = (x.astype(np.float64) @ v.astype(np.float64)).astype(np.float32)
      assert np.array_equal(x @ v, want)
      assert np.array_equal(want.astype(np.float64), x.astype(np.float64) @ v.astype(np.float64))


def test_probe_structure():
  for n in P.SIZES:
    inv = P.matrix("inv", n)
    assert np.array_equal(inv, inv.T) and np.count_nonzero(np.diag(inv)) >= 1
    if n > 129:
      for kind in ("shift_odd", "shift129"):
        a = P.matrix(kind, n)
        assert not np.array_equal(a, a.T) and np.count_nonzero(a) == n
  for (batch, tol) in P.STOP_BATCHES:
    for kind, n in batch:
      a, _ = P.stop_case(kind, n, tol)
      assert np.abs(a).max() == 4 and np.count_nonzero(np.abs(a) > 1) == 1
      assert np.array_equal(a, a.T) == (kind == "inv" or n <= 2)


def test_stop_cases_have_a_margin_and_match_the_oracle():
  """The gate of the GPU stop-rule tests: every step's float64 |ds| is further than 2 E from tol,
  so any float32 evaluation takes the float64 run's decisions -- the oracle does."""
  counts = set()
  for batch, tol in P.STOP_BATCHES:
    for kind, n in batch:
      a, ref = P.stop_case(kind, n, tol)
      E = P.probe_s_bounds(ref)
      assert P.stop_margin_ok(ref.steps, tol, E), (kind, n, tol)
      assert ref.iters < 100 and (n < 5 or 4 <= ref.iters <= 8), (kind, n, ref.iters)
      counts.add(ref.iters)
      for m in sorted({100, ref.iters, max(ref.iters - 1, 1), min(2, ref.iters)}):
        want = P.truncated(ref, min(m, ref.iters))
        v, s, it = orc.power_iteration(a, num_iters=m, error_tolerance=tol)
        assert it == want.iters, (kind, n, m, it, want.iters)
        assert_within((kind, n, m), s, v, want, *P.probe_bounds(want))
  assert len(counts) >= 3
  cases, tol, k = P.NEVER_BATCH
  for kind, n in cases:
    ref = P.reference64(P.matrix(kind, n), n, k, tol)
    assert ref.iters == k and P.stop_margin_ok(ref.steps, tol, P.probe_s_bounds(ref)), (kind, n)
    assert all(st["ds"] > tol for st in ref.steps)
    v, s, it = orc.power_iteration(P.matrix(kind, n), num_iters=k, error_tolerance=tol)
    assert it == k
    assert_within((kind, n), s, v, ref, *P.probe_bounds(ref))


def test_stop_margin_rejects_a_step_near_tol():
  steps = [dict(ds=1.0), dict(ds=0.25), dict(ds=0.01)]
  assert P.stop_margin_ok(steps, 0.1, 0.01)
  assert not P.stop_margin_ok(steps, 0.26, 0.01)
  assert not P.stop_margin_ok(steps, 0.1, [0.0, 0.08, 0.0])    # the predecessor's bound counts
  assert P.stop_margin_ok(steps, 0.1, [0.0, 0.0, 0.04])


def test_defect_cases_defeat_the_symmetric_reading():
  """One-step reference of the matrix as an execution that missed the defect would read it (upper
  triangle mirrored): at least 100 bounds away from the true one, so a missed detection fails."""
  for n, i, j, where in P.DEFECT_CASES:
    a = P.single_defect(n, i, j)
    assert a[i, j] != a[j, i] and np.count_nonzero(a != a.T) == 2
    ref = P.reference64(a, n, 1, 0.0)
    wrong = P.reference64(P.symmetric_reading(a), n, 1, 0.0)
    _, bv = P.dense_bounds(ref)
    assert P.ratio(wrong.vec, ref.vec, bv) > 100.0, (n, i, j, where)
  n, pad, i, j = P.DEFECT_BEHIND_PADDING
  assert pad <= i < n and j < pad


def test_case_lists_reach_every_structure():
  sizes = {n for b in P.DENSE_BATCHES for _, n in b}
  assert sizes == set(P.SIZES) and max(P.SIZES) == 1024
  assert all(len(b) <= 16 for b in P.DENSE_BATCHES + P.PROBE_BATCHES) and len(P.PAD_CASES) <= 16
  for kind in ("sym", "gen"):   # every size as a symmetric and as a general block
    assert {n for b in P.DENSE_BATCHES for k, n in b if k == kind} == set(P.SIZES)
  effective = list(P.SIZES) + [pad for _, _, pad in P.PAD_CASES]
  assert {P.tiles_of(n) for n in effective} >= set(range(0, 9))
  assert any(n % 4 and n % P.TILE for n in P.SIZES if n > P.TILE)          # ragged last tile
  # contiguous blocks: vec_ok = (n % 4 == 0); the strided layouts add both values again
  assert {P.vec_ok(0, n) for n in P.SIZES} == {True, False}
  seen = set()
  for name, (lda_of, off) in P.LAYOUTS.items():
    for _, n, _ in P.PAD_CASES:
      assert lda_of(n) >= n
      seen.add(P.vec_ok(off, lda_of(n)))
  assert seen == {True, False}
  assert not any(P.vec_ok(P.LAYOUTS["misaligned_base"][1], P.LAYOUTS["misaligned_base"][0](n))
                 for _, n, _ in P.PAD_CASES)
  assert all(P.LAYOUTS["misaligned_base"][0](n) % 4 == 0 for _, n, _ in P.PAD_CASES)
  pads300 = {pad for _, n, pad in P.PAD_CASES if n == 300}
  assert pads300 >= {0, 1, 64, 128, 129, 299, 300}
  assert sorted(P.SHUFFLE) == list(range(len(P.SIZES))) and list(P.SHUFFLE) != sorted(P.SHUFFLE)
  wheres = {(n, w) for n, _, _, w in P.DEFECT_CASES}
  assert len(P.DEFECT_CASES) == 11 and (129, "interior off-diagonal sub-block") not in wheres
