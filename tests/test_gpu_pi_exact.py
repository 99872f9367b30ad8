"""The batched power iteration (precondition_amd/csrc/power_iter.hip.h) against a float64 reference of the same loop,
within derived worst-case float32 bounds (tests/_pi_exact.py: derivation, matrix families and case
lists; tests/test_pi_exact_references.py gates them on the CPU).  Every family runs on the streaming
kernels (pi_mv_kernel / pi_red_kernel) and on the default execution (pi_block_kernel for n <= 512,
pi_resident_kernel teams above), the latter with the count of expired waits at zero before and after.

What the existing suite cannot see and this file can: the eigenvector output separates A from A^T
and a single misplaced element from none (one step from the fixed seed vector forgets nothing), the
probe matrices make the mat-vec exact so that only two norms and a division may round, NaN behind
padding_start and around strided views turns any leak into a NaN, and the stop rule is checked
against float64 step counts on cases whose decisions float32 provably shares.

out_v contract (include/ps_api.h): the first n_eff[b] floats of a row are written, everything behind
them keeps the caller's values -- pinned by test_out_v_contract."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _pi_exact as P

pytestmark = pytest.mark.gpu

STREAMING = {"power_iteration": "streaming"}


def L():
  from precondition_amd import _lib
  return _lib.lib()


def health():
  e, c, r = C.c_uint(), C.c_int(), C.c_int()
  assert L().ps_power_iteration_health(C.addressof(e), C.addressof(c), C.addressof(r)) == 0
  return e.value, c.value, r.value


@pytest.fixture(params=["streaming", "auto"])
def execution(request, device):
  """options of the call; the resident executions run with the health counter watched."""
  if request.param == "streaming":
    yield STREAMING
    return
  L().ps_power_iteration_reset_health()
  assert health() == (0, 0, 1)
  yield None
  assert health()[0] == 0


def upload(a, device, lda=None, offset=0):
  """The float32 matrix on the device: contiguous, or an [n, n] view (leading dimension lda,
  `offset` floats into the allocation) of a NaN-filled parent that it lies wholly inside."""
  a = np.array(a, dtype=np.float32)
  if lda is None:
    return torch.from_numpy(a).to(device)
  n = a.shape[0]
  parent = torch.full((offset + n * lda + 8,), float("nan"), dtype=torch.float32, device=device)
  view = parent.as_strided((n, n), (lda, 1), offset)
  view.copy_(torch.from_numpy(a).to(device))
  assert offset + (n - 1) * lda + n <= parent.numel()
  return view


def check_block(tag, lam, its, V, b, ref, es, bv):
  """iters, lam and the leading part of V[b] against `ref` within (es, bv); the rest of the row must
  still hold the sentinel."""
  n_eff = ref.vec.shape[0]
  assert its[b] == ref.iters, (tag, int(its[b]), ref.iters)
  assert np.isfinite(lam[b]), (tag, lam[b])
  err = abs(float(lam[b]) - ref.lam)
  assert err <= es, (tag, "lambda", float(lam[b]), ref.lam, "error", err, "bound", es)
  bad = P.first_mismatch(V[b, :n_eff], ref.vec, bv)
  assert bad is None, (tag, "first mismatch (row, tile, error, bound)", bad)
  assert (V[b, n_eff:] == P.SENTINEL).all(), (tag, "written behind n_eff")


# ---- a. one dense step ----------------------------------------------------------------------
@pytest.mark.parametrize("order", ["ascending", "shuffled"])
@pytest.mark.parametrize("flip", [0, 1])
def test_one_step_dense(device, execution, flip, order):
  batch = P.DENSE_BATCHES[flip]
  idx = list(range(len(batch))) if order == "ascending" else list(P.SHUFFLE)
  cases = [batch[i] for i in idx]
  mats = [upload(P.matrix(k, n), device) for k, n in cases]
  lam, its, V = P.run_pi(mats, None, 1, 0.0, "verify", execution)
  for b, (kind, n) in enumerate(cases):
    ref = P.one_step_ref(kind, n)
    check_block((kind, n, order), lam, its, V, b, ref, *P.dense_bounds(ref))
    if kind == "gen" and n >= 5:   # the same check against A^T must fail: V tells A from A^T
      ref_t = P.reference64(np.ascontiguousarray(P.matrix(kind, n).T), n, 1, 0.0)
      _, bv_t = P.dense_bounds(ref_t)
      assert P.first_mismatch(V[b, :n], ref_t.vec, bv_t) is not None, (kind, n)
      assert P.ratio(V[b, :n], ref_t.vec, bv_t) > 100.0, (kind, n)


# ---- b. one step on probes: the mat-vec is exact --------------------------------------------
@pytest.mark.parametrize("which", range(len(P.PROBE_BATCHES)))
def test_one_step_probes(device, execution, which):
  cases = P.PROBE_BATCHES[which]
  mats = [upload(P.matrix(k, n), device) for k, n in cases]
  lam, its, V = P.run_pi(mats, None, 1, 0.0, "verify", execution)
  for b, (kind, n) in enumerate(cases):
    ref = P.one_step_ref(kind, n)
    check_block((kind, n), lam, its, V, b, ref, *P.probe_bounds(ref))


# ---- c. symmetry detection ------------------------------------------------------------------
def test_single_defect_is_detected(device, execution):
  """Every defect position in one batch; rows are 16-byte aligned (lda % 4 == 0) so that whole
  64 x 64 sub-blocks take sym_check_kernel's float4 path."""
  mats = [upload(P.single_defect(n, i, j), device, lda=(n + 3) // 4 * 4)
          for n, i, j, _ in P.DEFECT_CASES]
  assert all(m.data_ptr() % 16 == 0 for m in mats)
  got = P.run_pi(mats, None, 1, 0.0, "verify", execution)
  for b, (n, i, j, where) in enumerate(P.DEFECT_CASES):
    ref = P.reference64(P.single_defect(n, i, j), n, 1, 0.0)
    check_block((n, i, j, where), *got, b, ref, *P.dense_bounds(ref))
  gen = P.run_pi(mats, None, 1, 0.0, "general", execution)
  for x, y in zip(got, gen):
    assert np.array_equal(x, y)


def test_defect_behind_padding_is_ignored(device, execution):
  n, pad, i, j = P.DEFECT_BEHIND_PADDING
  clean = P.run_pi([upload(P.dense_sym(n), device)], [pad], 1, 0.0, "verify", execution)
  hurt = P.run_pi([upload(P.single_defect(n, i, j), device)], [pad], 1, 0.0, "verify", execution)
  for x, y in zip(clean, hurt):
    assert np.array_equal(x, y)
  ref = P.reference64(P.dense_sym(n), pad, 1, 0.0)
  check_block((n, pad, i, j), *hurt, 0, ref, *P.dense_bounds(ref))


# ---- d. padding and strides, NaN everywhere else --------------------------------------------
@pytest.mark.parametrize("layout", sorted(P.LAYOUTS))
def test_padding_and_strides_with_poison(device, execution, layout):
  lda_of, off = P.LAYOUTS[layout]
  mats = [upload(P.padded(k, n, pad), device, lda=lda_of(n), offset=off) for k, n, pad in P.PAD_CASES]
  for m, (_, n, _) in zip(mats, P.PAD_CASES):
    assert (m.data_ptr() % 16 == 0 and P.ld_of(m) % 4 == 0) == P.vec_ok(off, lda_of(n))
  lam, its, V = P.run_pi(mats, [pad for _, _, pad in P.PAD_CASES], 1, 0.0, "verify", execution)
  for b, (kind, n, pad) in enumerate(P.PAD_CASES):
    if pad == 0:   # all padding: 0 / 0 in the reference
      assert np.isnan(lam[b]) and its[b] == 1 and (V[b] == P.SENTINEL).all()
      continue
    ref = P.one_step_ref(kind, n, pad)
    check_block((layout, kind, n, pad), lam, its, V, b, ref, *P.dense_bounds(ref))


# ---- e. out_v --------------------------------------------------------------------------------
def test_out_v_contract(device, execution):
  cases = P.OUT_V_CASES
  mats = [upload(P.matrix(k, n), device) for k, n, _ in cases]
  pads = [pad for _, _, pad in cases]
  n_max = max(n for _, n, _ in cases)
  lam, its, V = P.run_pi(mats, pads, 1, 0.0, "verify", execution, ldv=n_max + 5)
  assert V.shape == (len(cases), n_max + 5)
  for b, (kind, n, pad) in enumerate(cases):
    ref = P.one_step_ref(kind, n, pad)
    # check_block: V[b, :n_eff] is the vector, [n_eff, n_max) and [n_max, ldv) keep the sentinel
    check_block((kind, n, pad), lam, its, V, b, ref, *P.dense_bounds(ref))


def test_ldv_is_checked_against_the_effective_size(device, execution):
  """n = 300 cut to 128 by padding_start: ldv = 200 is enough, ldv = 127 is not."""
  mats = [upload(P.matrix("sym", 300), device)]
  lam, its, V = P.run_pi(mats, [128], 1, 0.0, "verify", execution, ldv=200)
  ref = P.one_step_ref("sym", 300, 128)
  check_block(("sym", 300, 128, "ldv", 200), lam, its, V, 0, ref, *P.dense_bounds(ref))
  lam, its, V = P.run_pi(mats, [128], 1, 0.0, "verify", execution, ldv=127, expect_rc=P.PS_EINVAL)
  assert (lam == P.SENTINEL).all() and (its == P.SENTINEL_IT).all() and (V == P.SENTINEL).all()


@pytest.mark.parametrize("what", ["ldv < n_max", "num_iters < 1"])
def test_invalid_arguments_touch_nothing(device, execution, what):
  mats = [upload(P.matrix("sym", n), device) for n in (129, 300)]
  num_iters, ldv = (1, 299) if what == "ldv < n_max" else (0, None)
  lam, its, V = P.run_pi(mats, None, num_iters, 0.0, "verify", execution, ldv=ldv,
                         expect_rc=P.PS_EINVAL)
  assert (lam == P.SENTINEL).all() and (its == P.SENTINEL_IT).all() and (V == P.SENTINEL).all()


# ---- f. stop rule and trajectories -----------------------------------------------------------
@pytest.mark.parametrize("which", range(len(P.STOP_BATCHES)))
def test_stop_rule_matches_float64_step_counts(device, execution, which):
  cases, tol = P.STOP_BATCHES[which]
  built = [P.stop_case(k, n, tol) for k, n in cases]
  mats = [upload(a, device) for a, _ in built]
  counts = sorted({r.iters for _, r in built})
  budgets = sorted({100, 2} | set(counts) | {c - 1 for c in counts if c > 1})
  for m in budgets:   # num_iters = the count itself, count - 1 (forced last step), 2, 100
    lam, its, V = P.run_pi(mats, None, m, tol, "verify", execution)
    for b, ((kind, n), (_, ref)) in enumerate(zip(cases, built)):
      want = P.truncated(ref, min(m, ref.iters))
      check_block((kind, n, "num_iters", m), lam, its, V, b, want, *P.probe_bounds(want))


def test_cyclic_shift_runs_out_of_steps(device, execution):
  cases, tol, k = P.NEVER_BATCH
  mats = [upload(P.matrix(kind, n), device) for kind, n in cases]
  lam, its, V = P.run_pi(mats, None, k, tol, "verify", execution)
  for b, (kind, n) in enumerate(cases):
    ref = P.reference64(P.matrix(kind, n), n, k, tol)
    assert ref.iters == k
    check_block((kind, n, "never"), lam, its, V, b, ref, *P.probe_bounds(ref))


# ---- g. one NaN element ----------------------------------------------------------------------
@pytest.mark.parametrize("n,i,j", P.NAN_CASES)
def test_one_nan_stays_in_its_block(device, execution, n, i, j):
  num_iters, tol = 5, 2.0 ** -12
  hurt = P.dense_sym(n).copy()
  hurt[i, j] = np.nan
  others = [("sym", 128), ("gen", 300), ("sym", 512), ("sym", 384)]   # all n <= 512: one kernel
  def run(x):
    mats = [upload(P.matrix(*others[0]), device), upload(x, device)]
    mats += [upload(P.matrix(k, m), device) for k, m in others[1:]]
    return P.run_pi(mats, None, num_iters, tol, "verify", execution)
  lam, its, V = run(hurt)
  lam0, its0, V0 = run(P.dense_sym(n))
  assert np.isnan(lam[1]) and 1 <= its[1] <= num_iters
  keep = [0, 2, 3, 4]
  assert np.isfinite(lam0).all() and np.isfinite(V0[keep]).all()
  assert np.array_equal(lam[keep], lam0[keep]) and np.array_equal(its[keep], its0[keep])
  assert np.array_equal(V[keep], V0[keep])
