"""CPU pins of tests/_newton_exact.py, the expectations of test_gpu_newton_exact.py, to
oracle.matrix_inverse_pth_root (itself pinned to the reference's goldens):

  * the scalar emulator of Family 1 equals the oracle on np.diag(d) bit for bit (diagonal, the
    metrics, exactly zero off-diagonals), for every spectrum kind;
  * the step-limited float32 oracle run of Family 2 equals the NumPy restatement bit for bit and
    lies inside the derived bound around the float64 reference (observed worst err / bound over
    the grid below: 0.26);
  * injected faults lie outside the bound at every size, by two to six orders of magnitude: one
    transposed 32 x 32 sub-block, one dropped 16-wide K-slab (each in the H update and in the M
    update), and a transposed right operand on the non-symmetric block.

A swapped operand order (B A for A B) is NOT outside the bound and cannot be: every iterate is a
polynomial in the input block, so the operands of every product of the iteration commute in exact
arithmetic and B A is the same matrix up to rounding (observed err / bound <= 0.26, the same as
the unfaulted run).  test_swapped_order_is_not_a_fault records that; the detectable form of an
operand mix-up -- reading the right operand transposed, the mn- against the k-contiguous
staging of gemm_core.hip.h -- is what the non-symmetric block is for.
"""
import numpy as np
import pytest

from oracle import shampoo_oracle as orc
from tests import _newton_exact as N
from tests._exact import ulp_distance

DENSE_SIZES = [96, 128, 129, 257, 384, 512, 1024]
DENSE_PS = [1, 2, 3, 4, 8]


def dense_ps(n):
  return [4] if n == 1024 else DENSE_PS


@pytest.mark.parametrize("kind", ["full", "equal", "spread", "retry"])
def test_scalar_emulator_equals_oracle_on_diagonal_blocks(kind):
  for n in (1, 2, 5, 129, 300):
    if kind == "retry" and n < 2:
      continue
    for p in (1, 2, 3, 4, 6, 8, 16):
      d = N.diag_spectrum(n, kind, salt=n + p)
      got, m = N.diag_root_emulate(d, p, N.DIAG_RIDGE)
      ref, mr = orc.matrix_inverse_pth_root(np.diag(d), p, ridge_epsilon=N.DIAG_RIDGE,
                                            relative_matrix_epsilon=False)
      what = (kind, n, p)
      assert ulp_distance(np.diag(ref), got).max() == 0, what
      assert np.count_nonzero(ref - np.diag(np.diag(ref))) == 0, what
      assert mr["inverse_pth_root_errors"] == float(m["error"]), what
      assert mr["final_error_ratio"] == float(m["ratio"]), what
      assert mr["inverse_pth_root_iters"] == m["iters"], what
      assert mr["total_retries"] == m["retries"], what
      if kind == "retry":
        assert m["retries"] == 2 and m["total_iters"] > m["iters"], what


def test_spectra_cover_what_they_are_for():
  # exactness of sumsq holds up to the largest size of the GPU grid, in every try
  for kind in ("full", "equal", "spread", "retry"):
    for p in (1, 4, 16):
      N.diag_root_emulate(N.diag_spectrum(1025, kind, salt=p), p, N.DIAG_RIDGE)
  its = [N.diag_root_emulate(N.diag_spectrum(1025, "spread", salt=p), p, N.DIAG_RIDGE)[1]["iters"]
         for p in (1, 2)]
  assert min(its) > 10, its
  with pytest.raises(AssertionError):    # the precondition is a real check
    N.exact_sumsq(np.full(1025, 200.0625, np.float32))
  # the three h0 candidates are distinct neighbours
  z = np.float32(0.3)
  c = sorted(float(N.pth_root_candidate(z, 4, s)) for s in N.H0_SHIFTS)
  assert c[0] < c[1] < c[2] and ulp_distance(np.float32(c[0]), np.float32(c[2])) == 2


def test_chain_is_the_reference_order():
  for p in (1, 2, 3, 4, 5, 6, 7, 8, 16):
    chain, power = N.chain_products(p)
    assert len(chain) == orc.mat_power_products(p), p
    rng = np.random.default_rng(p)
    mi = (np.eye(7) + 0.1 * rng.standard_normal((7, 7))).astype(np.float32)
    buf = {"mi": mi}
    for a, b, c in chain:
      buf[c] = np.matmul(buf[a], buf[b])
    assert np.array_equal(buf[power], orc.mat_power(mi, p)), p


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("n", DENSE_SIZES)
def test_step_limited_oracle_inside_derived_bound(n, symmetric):
  worst = 0.0
  for p in dense_ps(n):
    a = N.dense_case(n, 100 * n + p, symmetric)
    init = N.dense_init(a, p)
    hs, errs = N.dense_steps_f32(init, 3)
    bound = N.dense_bound(init, 3, symmetric=False)   # full products: the tighter bound
    for k in (1, 2, 3):
      ref, m = orc.matrix_inverse_pth_root(a.astype(np.float32), p, num_iters=k, ridge_epsilon=0.0,
                                           relative_matrix_epsilon=False)
      what = (n, p, k, symmetric)
      assert np.array_equal(ref, hs[k - 1]), what
      assert m["inverse_pth_root_iters"] == k, what
      assert m["inverse_pth_root_errors"] == float(errs[k - 1]), what
      # every try is the same computation (ridge 0); it is retried while the error is above 0.05
      assert m["total_retries"] == (6 if errs[k - 1] > 0.05 else 1), what
      r = N.worst_ratio(ref, *bound[k - 1])
      assert r <= 1.0, (what, r)
      if k == 1:
        assert r == 0.0, what
      worst = max(worst, r)
  print(f"n={n} symmetric={symmetric}: worst err / bound of the float32 oracle {worst:.3f}")


def _faults(n):
  k0 = (n // 2) // 16 * 16
  return {
      "transpose32 in H": N.fault_transpose32((1, "h"), 0, 32),
      "transpose32 in M": N.fault_transpose32((0, "m"), n - 64, n - 32),
      "dropped K-slab in H": N.fault_drop_slab((1, "h"), k0),
      "dropped K-slab in M": N.fault_drop_slab((0, "m"), k0),
  }


@pytest.mark.parametrize("n", DENSE_SIZES)
def test_injected_faults_exceed_the_bound(n):
  """Against the WIDER bound of the symmetric path, for k = 2 and 3."""
  for symmetric in (True, False):
    for p in dense_ps(n):
      a = N.dense_case(n, 100 * n + p, symmetric)
      init = N.dense_init(a, p)
      bound = N.dense_bound(init, 3, symmetric=symmetric)
      faults = _faults(n)
      if not symmetric:
        faults["transposed right operand in H"] = N.fault_transposed_operand((1, "h"))
        faults["transposed right operand in M"] = N.fault_transposed_operand((0, "m"))
      for name, hook in faults.items():
        hs, _ = N.dense_steps_f32(init, 3, hook)
        for k in (2, 3):
          r = N.worst_ratio(hs[k - 1], *bound[k - 1])
          assert r > 1.0, (n, p, k, symmetric, name, r)


@pytest.mark.parametrize("n", [96, 257])
def test_swapped_order_is_not_a_fault(n):
  """The operands of every product are polynomials in the input block: they commute, B A is
  A B up to rounding, and a valid bound must hold it (module docstring)."""
  for symmetric in (True, False):
    for p in DENSE_PS:
      init = N.dense_init(N.dense_case(n, 100 * n + p, symmetric), p)
      bound = N.dense_bound(init, 3, symmetric=symmetric)
      for tag in ((1, "h"), (0, "m")):
        hs, _ = N.dense_steps_f32(init, 3, N.fault_swap(tag))
        for k in (2, 3):
          assert N.worst_ratio(hs[k - 1], *bound[k - 1]) <= 1.0, (n, p, k, symmetric, tag)


def test_mat_power_integer_cases_are_exact():
  for n, p, density in N.MAT_POWER_CASES:
    a, ref = N.mat_power_int_case(n, p, density)    # asserts max |A|^q < 2^24, q <= p
    assert np.abs(a).max() <= 1 and ref.shape == (n, n)
    if n <= 130:
      assert np.array_equal(ref, np.linalg.matrix_power(a, p)), (n, p)
  ns = {c[0] for c in N.MAT_POWER_CASES}
  assert {127, 128, 129, 255, 256, 257} <= ns and any(c[1] == 4 and c[0] > 256 for c in N.MAT_POWER_CASES)
