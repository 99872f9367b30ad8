"""CPU gate of test_gpu_eigh_solvers.py: the case list, the metrics and the floors of tests/_eigh_cases.py
are checked here without a GPU.  Every family builds the structure it is named after and keeps it through
the float32 rounding; float32 LAPACK (ssyevd) itself meets every floor on every finite case (a floor below
what a correct float32 solver achieves would be wrong); and the metrics notice the wrong answers a Jacobi
solver can produce, above all "V = I, lambda = diag(A)", the answer of a one-sided solver that never
rotates."""
import numpy as np
import pytest

from oracle.lapack32 import eigh32
from tests import _eigh_cases as E

ALL_SIZES = sorted(set(E.SMALL_SIZES) | set(E.BIG_SIZES))


def finite_pairs():
  return [(name, n) for n in ALL_SIZES for name in E.names_for(n, E.FINITE)]


def test_size_lists_cross_every_branch_of_the_small_kernel_and_the_block_solvers():
  assert {1, 2, 3, 63, 64, 65, 96, 97, 127, 128} <= set(E.SMALL_SIZES) and max(E.SMALL_SIZES) == 128
  assert {129, 192, 257} <= set(E.BIG_SIZES) and min(E.BIG_SIZES) > 128
  assert set(E.SMALL_ROOT_SIZES) == {1, 2, 64, 65, 97, 128} and set(E.ROOT_PS) == {1, 2, 4, 8}


def test_exclusions_are_only_the_undefined_pairs():
  left_out = {(name, n) for n in ALL_SIZES for name in E.ALL if not E.defined(name, n)}
  hadamard = {("symmetric_hadamard", n) for n in ALL_SIZES if n < 2 or n & (n - 1)}
  assert left_out == hadamard | {("bipartite_random", 1)}
  assert {n for n in ALL_SIZES if E.defined("symmetric_hadamard", n)} == {2, 64, 128}


@pytest.mark.parametrize("n", ALL_SIZES)
def test_families_build_what_they_are_named_after(n):
  for name in E.names_for(n, E.FINITE):
    a = E.case(name, n)
    assert a.dtype == np.float32 and a.shape == (n, n), name
    assert np.isfinite(a).all() and np.array_equal(a, a.T), name
    assert np.array_equal(a, E.case(name, n)), name   # deterministic
  for name in E.NON_FINITE:
    a = E.case(name, n)
    assert not np.isfinite(a).all() and np.isfinite(a).sum() >= n * n - 2, name
  w = {name: E.truth(E.case(name, n)) for name in E.names_for(n, E.FINITE)}
  assert np.array_equal(E.case("identity", n), np.eye(n, dtype=np.float32)) and not E.case("zero", n).any()
  d = np.diag(E.case("diag_descending", n))
  assert (np.diff(d) < 0).all() and not (E.case("diag_descending", n) - np.diag(d)).any()
  assert (w["negative_definite"] < 0).all()
  for name in E.POSITIVE_DEFINITE:
    assert (w[name] > 0).all(), name
  assert np.abs(w["two_I_plus_1e-6_noise"] - 2).max() < 1e-4
  if n >= 2:
    assert np.abs(w["rank1"][:-1]).max() <= 1e-6 * w["rank1"][-1]
    assert w["goe_indefinite"][0] < 0 < w["goe_indefinite"][-1]
  if n >= 8:
    rank = max(1, n // 4)
    assert np.abs(w["psd_rank_deficient"][:n - rank]).max() <= 1e-5 * w["psd_rank_deficient"][-1]
    assert w["psd_rank_deficient"][n - rank] > 1e-3 * w["psd_rank_deficient"][-1]
  if n >= 17:
    # graded over about eight decades, positive definite after the rounding too
    assert 1e7 < w["graded_1e8"][-1] / w["graded_1e8"][0] < 1e11
  for name, (_, ex) in E.UNSCALED.items():
    base, ex2 = E.unscaled_case(name, n)
    assert ex == ex2 and np.array_equal(E.case(name, n).astype(np.float64), base.astype(np.float64) * 2.0 ** ex), name
  assert np.abs(E.case("wishart_x2^34", n)).max() > 2.0 ** 34
  assert 0 < np.abs(E.case("wishart_x2^-50", n)).max() < 2.0 ** -38


@pytest.mark.parametrize("n", [k for k in ALL_SIZES if k >= 2])
def test_pm_families_have_degenerate_eigenvalues_of_both_signs(n):
  for name in E.names_for(n, E.PM_MIXING):
    a = E.case(name, n)
    w = E.truth(a)
    nrm = np.abs(w).max()
    neg, pos = -w[w < 0], w[w > 0]
    assert len(neg) and len(pos), name
    # some -x sits within rounding of a +x: the singular subspace of |x| holds both eigenvectors
    gap = np.abs(neg[:, None] - pos[None, :]).min()
    assert gap <= 1e-6 * nrm, (name, gap / nrm)
    d = np.diag(a)
    if name in ("bipartite_random", "path_graph"):
      assert not d.any(), name
    if name == "exchange":   # the centre of an odd exchange matrix is its one diagonal entry
      assert not np.delete(d, n // 2).any() if n % 2 else not d.any()
    if name == "householder_uniform":
      assert (d == np.float32(1 - 2 / n)).all()
    if name == "path_graph":
      assert np.abs(w - np.sort(2 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1)))).max() < 1e-12
    if name == "symmetric_hadamard":
      assert np.abs(np.abs(w) - np.sqrt(n)).max() < 1e-12


@pytest.mark.parametrize("n", ALL_SIZES)
def test_ssyevd_meets_every_floor_on_every_finite_case(n):
  floors = E.floors_for(n)
  for name in E.names_for(n, E.FINITE):
    y = E.yardstick(E.case(name, n))
    for k, f in floors.items():
      assert y[k] <= f, (name, n, k, y[k], f)
    assert y["sorted"], name


def test_bound_rule():
  assert E.bound("resid", 1e-7, 2e-5) == 2e-5 and E.bound("resid", 1e-5, 2e-5) == 4e-5
  assert E.YARDSTICK_FACTOR == 4.0
  assert E.FLOORS_SMALL == {"eig_err": 2e-6, "resid": 2e-5, "orth": 2e-5}
  assert E.FLOORS_BIG == {"eig_err": 3e-6, "resid": 3e-6, "orth": 5e-6}


def _fails(name, n, mutant):
  a = E.case(name, n)
  e, v = eigh32(a)
  _, bad_ok = E.check(a, e, v, E.floors_for(n))
  assert not bad_ok, (name, n, bad_ok)
  _, bad = E.check(a, *E.MUTANTS[mutant](a, e, v), E.floors_for(n))
  return bool(bad)


@pytest.mark.parametrize("mutant", sorted(E.MUTANTS))
def test_metrics_catch_the_mutants_on_plain_families(mutant):
  caught = [name for name in E.PLAIN if _fails(name, 17, mutant)]
  assert caught, mutant
  if mutant == "scaled_vector":
    assert len(caught) == len(E.PLAIN)       # orth sees it whatever the matrix
  if mutant == "swapped_values":
    assert "goe_indefinite" in caught and "identity" not in caught   # equal values may swap


@pytest.mark.parametrize("n", [2, 17, 64, 97, 128])
def test_never_rotating_solver_fails_every_pm_family_and_the_scaled_wishart(n):
  """The predicted failure of a one-sided Jacobi whose rotation test never fires: V = I and diag(A)."""
  for name in E.names_for(n, E.PM_MIXING) + ["wishart_x2^34"]:
    assert _fails(name, n, "diagonal"), (name, n)
