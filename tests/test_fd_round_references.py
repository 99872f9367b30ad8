"""CPU gate of test_gpu_fd_round.py: the restatements, float64 references, case lists, measured constants and
comparisons of tests/_fd_round.py are checked here without a GPU -- against their own float64 twins, against the
float32-LAPACK oracle (oracle.shampoo_oracle.fd_update_root, the reference statement by statement), and against
seeded faults of the restatements: a comparison that a mutant passes here would let the same fault of a kernel
pass on the GPU."""
import numpy as np
import pytest

from oracle import shampoo_oracle as orc
from tests import _fd_round as R
from tests.test_optimizer_host_logic import packed_matches

F32, F64 = np.float32, np.float64


def _as_got(ref):
  return dict(params=np.asarray(ref["params"], F32), converged=ref["converged"], summary=ref["summary"])


# ---------------------------------------------------------------------------------------------------
# A. the stop rule
# ---------------------------------------------------------------------------------------------------
def test_control_ref_float32_and_float64_take_every_decision_alike():
  """Every listed case passes the decision checker, and the float32 restatement and its float64 twin then agree:
  converged, degree and summary equal, ctr / e / sigma1 within 4 float32 ulp."""
  cases = R.control_cases()
  assert len(cases) >= 4 * len(R.CONTROL_SHAPES)
  shapes = {(c[1].shape[0], c[1].shape[1], c[3]) for c in cases}
  assert shapes == {(s[0], s[1], s[2]) for s in R.CONTROL_SHAPES}
  plain, conv_all, degs = set(), set(), set()
  for tag, th, rs, k, n, tol, degree in cases:
    R.assert_control_decisions_safe(th, rs, k, n, tol, degree)
    a = R.control_ref(th, rs, k, n, tol, degree)
    b = R.control_ref(th, rs, k, n, tol, degree, dtype=F64)
    assert np.array_equal(a["converged"], b["converged"]), tag
    assert np.array_equal(a["summary"], b["summary"]), tag
    assert np.array_equal(a["params"][:, 3], b["params"][:, 3]), tag
    d = np.abs(a["params"][:, :3].astype(F64) - b["params"][:, :3])
    assert np.all(d <= 4 * R.ulp32(b["params"][:, :3])), (tag, float(np.max(d / R.ulp32(b["params"][:, :3]))))
    R.check_control(_as_got(b), a)
    plain.add(int(a["summary"][3])); conv_all.add(int(a["summary"][0]))
    degs.update(a["params"][:, 3].astype(int).tolist())
  assert plain == {0, 1} and conv_all == {0, 1}          # the plain flag and the all-converged word both ways
  assert {1, R.CONTROL_DEGREE} <= degs and len(degs) >= 6  # both clamps and degrees between them


def test_control_cases_hold_every_family_at_every_shape():
  for tag, th, rs, k, n, tol, degree in R.control_cases():
    batch, b = th.shape
    if batch >= len(R.CONTROL_FAMILIES):
      r = R.control_ref(th, rs, k, n, tol, degree)
      assert set(r["converged"].tolist()) == {0, 1}, tag        # converged and unconverged side by side
      assert np.any(th[:, b - 1] < 0) and np.any(th[:, 0] <= 0) and np.any(np.isnan(rs[:, :k])), tag
  one = [c for c in R.control_cases() if c[1].shape[0] == 1]
  assert len(one) == 2 * len(R.CONTROL_FAMILIES)               # every family alone in the single-factor shape


@pytest.mark.parametrize("mutation", ["noise_1.2e-7", "round_degree", "stride_256"])
def test_control_comparison_catches_a_mutant(mutation):
  caught = []
  for tag, th, rs, k, n, tol, degree in R.control_cases():
    ref = R.control_ref(th, rs, k, n, tol, degree)
    bad = R.control_ref(th, rs, k, n, tol, degree, mutate=(mutation,))
    try:
      R.check_control(_as_got(bad), ref)
    except AssertionError:
      caught.append(tag)
  assert caught, mutation
  if mutation == "stride_256":
    assert all(t.startswith("300x") for t in caught) and len(caught) == 4
  print(mutation, "caught in", len(caught), "of", len(R.control_cases()), "cases")


# ---------------------------------------------------------------------------------------------------
# B. one round
# ---------------------------------------------------------------------------------------------------
def test_round_float32_evaluation_gives_the_recorded_ritz_figure_and_passes_the_checks():
  """The NumPy float32 round against ritz_ref over ROUND_CASES: its worst Ritz error is the recorded figure (the
  GPU bound is 4 x that), and as a stand-in for the device it passes every assertion of check_round -- the
  derived residual bound included, on the case whose residuals are at rounding level too."""
  worst, small = 0.0, []
  for bsz, n, b, _x6, spans in R.ROUND_CASES:
    c, x0 = R.round_case(bsz, n, b, spans)
    for j in range(bsz):
      th = R.round_f32(c[j], x0[j]).astype(F64)
      want = R.ritz_ref(c[j], x0[j])
      worst = max(worst, float(np.max(np.abs(th - want)) / want[0]))
      fig = R.check_round(c[j], x0[j], *R.round_outputs_f32(c[j], x0[j]))
      if spans:
        small.append(fig["rho_rel"])
  print(f"float32 round, worst Ritz error / theta_1: {worst:.3g} (recorded {R.ROUND_RITZ_F32_MEASURED:.3g})")
  assert R.ROUND_RITZ_F32_MEASURED / 4 <= worst <= 1.5 * R.ROUND_RITZ_F32_MEASURED
  assert R.ROUND_RITZ_BOUND == 4 * R.ROUND_RITZ_F32_MEASURED
  assert small and max(small) < 1e-5          # the spanning start block: residuals at rounding level


@pytest.mark.parametrize("mutation", ["residual_skips_ragged_rows", "theta_ascending", "cx_two_planes"])
def test_round_comparison_catches_a_mutant(mutation):
  caught = 0
  for bsz, n, b, _x6, spans in R.ROUND_CASES:
    c, x0 = R.round_case(bsz, n, b, spans)
    try:
      R.check_round(c[0], x0[0], *R.round_outputs_f32(c[0], x0[0], mutate=(mutation,)))
    except AssertionError:
      caught += 1
  assert caught >= 2, (mutation, caught)


# ---------------------------------------------------------------------------------------------------
# C. prepare and finish
# ---------------------------------------------------------------------------------------------------
def test_prepare_ref_is_the_oracles_weighting_and_catches_its_mutants():
  cases = R.prepare_cases()
  assert len(cases) == 4 * len(R.PREPARE_SHAPES)
  caught = {"ridge_ignores_relative": 0, "ridge_without_tolerance": 0}
  for tag, prev, r, eps, tol, relative in cases:
    got = R.prepare_ref(prev, r, eps, tol, relative)
    for j in range(prev.shape[0]):
      # the oracle's statements (DS:1160-1172) on the same float32 values
      sketch, fwd = prev[j][:, :r], prev[j][-r:, -1]
      lead = fwd[0] if relative else F32(1.0)
      ridge = F32(F32(eps) * np.maximum(F32(lead), F32(tol)))
      want = (sketch * np.sqrt(fwd + ridge)).astype(F32)
      assert np.array_equal(R.bits32(got[j]), R.bits32(want)), tag
    for m in caught:
      caught[m] += not np.array_equal(R.bits32(R.prepare_ref(prev, r, eps, tol, relative, mutate=(m,))), R.bits32(got))
  assert all(v > 0 for v in caught.values()), caught


def test_finish_cases_cover_every_branch_with_margins():
  cases = R.finish_cases()
  assert len(cases) == 8 * len(R.FINISH_SHAPES)
  seen = dict(tail_pos=0, tail_zero=0, dropped_unsafe=0, kept_safe=0, below_noise=0, zero_deflated=0, negative=0)
  for tag, th, x, prev, p, r, decay in cases:
    for j in range(th.shape[0]):
      ref = R.finish_ref(th[j], x[j], prev[j], p, r, decay)
      assert R.finish_margins_ok(ref), tag
      seen["tail_pos"] += ref["tail"] > 0
      seen["tail_zero"] += ref["tail"] == 0 and ref["const64"] == 0
      seen["dropped_unsafe"] += int(np.sum(ref["positive"][:2] & ~ref["keep"][:2])) == 2
      seen["kept_safe"] += bool(ref["keep"][2] and ref["keep"][3])
      seen["below_noise"] += bool(np.any((th[j, :r + 1] > 0) & (th[j, :r + 1] <= ref["noise"])))
      seen["zero_deflated"] += bool(np.any(~ref["positive"]))
      seen["negative"] += bool(np.any(th[j, :r + 1] < 0))
      R.check_finish(R.finish_packed(ref, x[j]), ref, x[j])
  assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("mutation", ["wide_safe", "no_noise_floor", "deflated_e2"])
def test_finish_comparison_catches_a_mutant(mutation):
  caught = 0
  cases = R.finish_cases()
  for tag, th, x, prev, p, r, decay in cases:
    ref = R.finish_ref(th[0], x[0], prev[0], p, r, decay)
    bad = R.finish_ref(th[0], x[0], prev[0], p, r, decay, mutate=(mutation,))
    try:
      R.check_finish(R.finish_packed(bad, x[0]), ref, x[0])
    except AssertionError:
      caught += 1
  assert caught >= len(cases) // 2, (mutation, caught)


# ---------------------------------------------------------------------------------------------------
# D. whole update; the oracle
# ---------------------------------------------------------------------------------------------------
def _oracle(prev, gram, rank, relative):
  return orc.fd_update_root(R.gram_factor(gram), R.UPDATE_P, rank, ridge_epsilon=R.UPDATE_RIDGE,
                            error_tolerance=1e-6, relative_matrix_epsilon=bool(relative), decay=R.UPDATE_DECAY,
                            padding_start=gram.shape[0], prev=prev)


def _ideal_finish(prev, gram, rank, relative):
  """A float32 stand-in for the device: exact leading eigenpairs (float64 eigh) rounded to float32, then
  finish_ref's arithmetic."""
  ref, info = R.update_ref(prev, gram, R.UPDATE_P, rank, relative=relative)
  sketch, fwd = np.asarray(prev, F64)[:, :rank], np.asarray(prev, F64)[-rank:, -1]
  ridge = float(F32(R.UPDATE_RIDGE)) * max(fwd[0] if relative else 1.0, 1e-6)
  w = sketch * np.sqrt(fwd + ridge)[None, :]
  c = float(F32(R.UPDATE_DECAY)) * (w @ w.T) + np.asarray(gram, F64)
  lam, vec = np.linalg.eigh(0.5 * (c + c.T))
  b = rank + 1
  return lam[::-1][:b].astype(F32), np.ascontiguousarray(vec[:, ::-1][:, :b]).astype(F32), ref, info


def test_finish_ref_and_update_ref_agree_with_the_oracle_on_a_full_rank_case():
  """The first factor of the chained case at d = 256: finish_ref fed the oracle's own s^2 and u (float32 sgesdd)
  gives the oracle's packed result (packed_matches), and update_ref agrees with the oracle at float32 level."""
  d, r, bsz = R.UPDATE_SHAPES[0]
  case = R.update_case("chained", d, r, bsz)
  gram, prev = case["steps"][0][0], case["prev0"][0]
  want = _oracle(prev, gram, r, case["relative"])
  from oracle import lapack32
  sketch, fwd = prev[:, :r], prev[-r:, -1]
  ridge = F32(F32(R.UPDATE_RIDGE) * np.maximum(F32(1.0), F32(1e-6)))
  updated = np.concatenate([F32(np.sqrt(R.UPDATE_DECAY)) * (sketch * np.sqrt(fwd + ridge)).astype(F32),
                            R.gram_factor(gram)], axis=1).astype(F32)
  u, s, _ = lapack32.svd32(updated)
  fin = R.finish_ref((s * s).astype(F32)[:r + 1], u[:, :r + 1], prev, R.UPDATE_P, r, R.UPDATE_DECAY)
  mine = R.finish_packed(fin, u[:, :r + 1])
  assert packed_matches(mine, want, r, tol=1e-5)
  assert np.array_equal(mine[-1, -2], want[-1, -2])
  ref, info = R.update_ref(prev, gram, R.UPDATE_P, r, relative=case["relative"])
  scalar, proj = R.update_errors(want, ref, r)
  assert scalar <= 1.5 * R.UPDATE_ORACLE_SCALAR and proj <= 1.5 * R.UPDATE_ORACLE_PROJECTOR, (scalar, proj)
  assert packed_matches(ref.astype(F32), want, r, tol=1e-5)


def test_update_cases_margins_oracle_figures_and_mutants():
  """Over every case of section D: the true eigenvalues are 100 x away from the noise floor; the oracle's worst
  error against update_ref is the recorded pair of figures; an ideal float32 device (exact eigenpairs rounded,
  then finish_ref) passes the exact checks and the bound; two mutants of finish_ref do not."""
  worst_s = worst_p = 0.0
  caught = {"no_noise_floor": 0, "deflated_e2": 0}
  for kind in R.UPDATE_KINDS:
    for d, r, bsz in R.UPDATE_SHAPES:
      case = R.update_case(kind, d, r, bsz)
      prev = case["prev0"]
      for grams in case["steps"]:
        nxt = []
        for j in range(bsz if kind == "chained" else 1):
          theta, x, ref, info = _ideal_finish(prev[j], grams[j], r, case["relative"])
          assert info["margin"] >= 100.0, (kind, d, info["margin"])
          es, ep = R.update_errors(_oracle(prev[j], grams[j], r, case["relative"]), ref, r,
                                   tail_fields=kind != "rank_deficient")
          worst_s, worst_p = max(worst_s, es), max(worst_p, ep)
          fin = R.finish_ref(theta, x, prev[j], R.UPDATE_P, r, R.UPDATE_DECAY)
          got = R.finish_packed(fin, x)
          R.check_update_exact(got, ref, r)
          gs, gp = R.update_errors(got, ref, r)
          assert gs <= R.update_bound(R.UPDATE_ORACLE_SCALAR, info), (kind, d, gs)
          assert gp <= R.update_bound(R.UPDATE_ORACLE_PROJECTOR, info), (kind, d, gp)
          for m in caught:
            bad = R.finish_packed(R.finish_ref(theta, x, prev[j], R.UPDATE_P, r, R.UPDATE_DECAY, mutate=(m,)), x)
            try:
              R.check_update_exact(bad, ref, r)
              bs, _ = R.update_errors(bad, ref, r)
              assert bs <= R.update_bound(R.UPDATE_ORACLE_SCALAR, info)
            except AssertionError:
              caught[m] += 1
          nxt.append(ref.astype(F32))
        if kind == "chained":
          prev = np.stack(nxt)
      if kind == "rank_deficient":
        keep = R.update_ref(case["prev0"][0], case["steps"][0][0], R.UPDATE_P, r)[1]["keep"]
        assert keep.tolist() == [True] * case["q"] + [False] * 3
  print(f"oracle against update_ref, worst: scalar {worst_s:.3g} (recorded {R.UPDATE_ORACLE_SCALAR:.3g}), "
        f"projector {worst_p:.3g} (recorded {R.UPDATE_ORACLE_PROJECTOR:.3g})")
  assert R.UPDATE_ORACLE_SCALAR / 4 <= worst_s <= 1.5 * R.UPDATE_ORACLE_SCALAR
  assert R.UPDATE_ORACLE_PROJECTOR / 4 <= worst_p <= 1.5 * R.UPDATE_ORACLE_PROJECTOR
  assert caught["no_noise_floor"] >= 2 and caught["deflated_e2"] >= 2, caught


# ---------------------------------------------------------------------------------------------------
def test_generators_are_deterministic_and_lists_non_empty():
  for gen in (R.control_cases, R.prepare_cases, R.finish_cases):
    a = gen()
    gen.cache_clear()
    b = gen()
    assert len(a) == len(b) > 0
    for ca, cb in zip(a, b):
      for va, vb in zip(ca, cb):
        if isinstance(va, np.ndarray):
          assert np.array_equal(va, vb, equal_nan=True), ca[0]
        else:
          assert va == vb
  assert R.ROUND_CASES and R.UPDATE_SHAPES and R.UPDATE_KINDS
  c1, x1 = R.round_case(1, 100, 33, False)
  R.round_case.cache_clear()
  c2, x2 = R.round_case(1, 100, 33, False)
  assert np.array_equal(c1, c2) and np.array_equal(x1, x2)
  u1 = R.update_case("rank_deficient", 256, 8, 3)
  R.update_case.cache_clear()
  u2 = R.update_case("rank_deficient", 256, 8, 3)
  assert np.array_equal(u1["steps"][0], u2["steps"][0]) and np.array_equal(u1["x0"], u2["x0"])
