"""Edge inputs for the three Jacobi eigensolvers against float64, with float32 LAPACK as the yardstick:

* eigh_small_kernel (n <= 128, one-sided Jacobi in LDS): every family of tests/_eigh_cases.py at the sizes
  around the 64 / 96 / 128 row branches and the odd-n dummy column, as ONE batched call per size; non-finite
  batch mates; bit-independence from the rest of the batch; roots with padding;
* the blocked two-sided Jacobi (plain eigenpairs, n > 128) on the same families;
* the one-sided Cholesky-Jacobi (roots, n > 128) and its fallback.

A solver passes a metric below max(4 x ssyevd's value on the same input, the floor the suite already asserts
for that solver): _eigh_cases.bound.  Every figure is printed before it is asserted (pytest -s): the table
in profiles/eigh_solver_accuracy.md is that output.  A (solver, family, size) with a bound of its own is in
EXCEPTIONS with the mechanism; nothing else departs from the rule."""
import functools

import numpy as np
import pytest
import torch

from oracle import shampoo_oracle as orc
from tests import _eigh_cases as E

pytestmark = pytest.mark.gpu

# (solver, family, n, metric) -> (bound, mechanism): plain eigenpairs with a bound of their own.  None so far.
EXCEPTIONS = {}

# Sweeps (metrics column 5) of the small kernel on the positive semi-definite root inputs at the commit before
# the mixing detector, (family, n) -> sweeps (the same for every p): the detector must not send such inputs
# into the second, shifted attempt, which would show up as about twice the count.
PARENT_SWEEPS = {("wishart", 1): 1, ("wishart", 2): 2, ("wishart", 64): 9, ("wishart", 65): 9, ("wishart", 97): 10,
                 ("wishart", 128): 10, ("psd_rank_deficient", 1): 1, ("psd_rank_deficient", 2): 5,
                 ("psd_rank_deficient", 64): 23, ("psd_rank_deficient", 65): 22, ("psd_rank_deficient", 97): 23,
                 ("psd_rank_deficient", 128): 26}

# The one-sided Cholesky-Jacobi solver ends its sweeps once the largest scaled Gram entry |g_i . g_j| /
# (|g_i| |g_j|) of a sweep is below eigh_sweep_tol (default 2e-6, include/ps_api.h).  On 2 I + 1e-6 noise every
# such entry is below it from the start: one sweep, and the left singular vectors U are orthogonal to the
# tolerance only, U^T U = I + E with |E_ij| <= tol.  All eigenvalues coincide, so the root is c U U^T and its
# relative Frobenius error is ||E||_F / sqrt(n) <= tol sqrt(n - 1) on top of the rounding the rule allows
# (measured 4.6e-6 / 5.5e-6 / 6.4e-6 at n = 129 / 192 / 257 against 4.1e-6 from the plain rule).
ONE_SIDED_SWEEP_TOL = 2e-6
ROOT_EXTRA = {("one_sided two_I_plus_1e-6_noise", n): ONE_SIDED_SWEEP_TOL * np.sqrt(n - 1) for n in (129, 192, 257)}

# Finding, not fixed here (the pivots of eigh_cj.hip.h are its own subject): the one-sided solver has no input
# scaling.  Its pivot runs the shared LDS Jacobi on the 128 x 128 Gram matrix P of two block columns, whose
# rotation test multiplies two squared column norms of P, i.e. the fourth power of the entries of A: with
# entries of 6e12 that product is inf, no pair of a pivot rotates, and the solver runs its 24 sweeps without
# converging (root error 0.87 at every size).  What the call does report is asserted instead: a NaN root or an
# error metric at or above the reference's failure threshold 0.1 (DS:1017-1021) -- never a small metric.
ONE_SIDED_OUT_OF_RANGE = ("wishart_x2^34",)


def K():
  from precondition_amd import kernels
  return kernels


@functools.lru_cache(maxsize=None)
def reference(name, n):
  """(float32 input, float64 eigenvalues, ssyevd's metrics): computed once, shared, never written to."""
  a = E.case(name, n)
  a.setflags(write=False)
  if name in E.NON_FINITE:
    return a, None, None
  w = E.truth(a)
  return a, w, E.yardstick(a, w)


def eigh_call(mats, device, options=None):
  es, vs = K().eigh_batched([torch.tensor(m, device=device) for m in mats], options=options)
  torch.cuda.synchronize()
  return [e.cpu().numpy() for e in es], [v.cpu().numpy() for v in vs]


def judge(solver, name, n, e, v, bad):
  a, w, y = reference(name, n)
  floors = E.floors_for(n)
  m = E.metrics(a, e, v, w)
  print(f"EIGH {solver} {name} n={n} eig_err {m['eig_err']:.2e} ({y['eig_err']:.2e}) resid {m['resid']:.2e} "
        f"({y['resid']:.2e}) orth {m['orth']:.2e} ({y['orth']:.2e}) rel_eig_err {m['rel_eig_err']:.2e} "
        f"({y['rel_eig_err']:.2e}) sorted {m['sorted']}")
  for k in ("eig_err", "resid", "orth"):
    b = EXCEPTIONS.get((solver, name, n, k), (E.bound(k, y[k], floors[k]),))[0]
    if not m[k] <= b:
      bad.append((solver, name, n, k, m[k], b))
  if not m["sorted"]:
    bad.append((solver, name, n, "sorted"))
  if name in E.GRADED:
    # at least as close to every eigenvalue, relative to itself, as the reference's solver (x 1.5)
    if not m["rel_eig_err"] <= 1.5 * y["rel_eig_err"]:
      bad.append((solver, name, n, "rel_eig_err", m["rel_eig_err"], 1.5 * y["rel_eig_err"]))


# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.SMALL_SIZES)
def test_small_kernel_every_family_in_one_batch(n, device):
  """One workgroup per matrix, non-finite inputs in the same batch.  n <= ps_eigh_sorted_max_n(): eigh_batched
  returns the kernel's own order untouched, so `sorted` judges the kernel, not a Python argsort."""
  from precondition_amd._lib import lib
  assert n <= lib().ps_eigh_sorted_max_n()
  names = E.names_for(n, E.ALL)
  assert set(E.names_for(n, E.FINITE)) | set(E.NON_FINITE) == set(names)
  es, vs = eigh_call([reference(k, n)[0] for k in names], device)
  bad = []
  for name, e, v in zip(names, es, vs):
    if name in E.NON_FINITE:
      print(f"EIGH small {name} n={n} eigenvalues {e[:4]}")
      if not np.isnan(e).all():
        bad.append(("small", name, n, "eigenvalues of a non-finite input are NaN", e[:4]))
      continue
    judge("small", name, n, e, v, bad)
  assert not bad, bad


def test_small_kernel_blocks_do_not_depend_on_their_batch_mates(device):
  """The n = 97 batch again, interleaved with n = 128 and n = 3 matrices and one n = 200 matrix (the call then
  runs the blocked solvers and their finish kernels past the small blocks): same bits as alone."""
  n = 97
  names = E.names_for(n, E.ALL)
  solo_e, solo_v = eigh_call([reference(k, n)[0] for k in names], device)
  mates = ([reference(k, 128)[0] for k in ("goe_indefinite", "exchange", "nan_entry", "wishart_x2^34")] +
           [reference(k, 3)[0] for k in ("path_graph", "ones")] + [reference("goe_indefinite", 200)[0]])
  mixed, where = [], []
  for i, name in enumerate(names):
    where.append(len(mixed))
    mixed.append(reference(name, n)[0])
    mixed.append(mates[i % len(mates)])
  es, vs = eigh_call(mixed, device)
  for name, at, e0, v0 in zip(names, where, solo_e, solo_v):
    assert e0.tobytes() == es[at].tobytes() and v0.tobytes() == vs[at].tobytes(), name
  # the mates themselves are still solved
  bad = []
  judge("two_sided", "goe_indefinite", 200, es[2 * 6 + 1], vs[2 * 6 + 1], bad)
  judge("small", "goe_indefinite", 128, es[1], vs[1], bad)
  assert not bad, bad


# ---------------------------------------------------------------------------------------------------------
def rel_fro(h, truth):
  return float(np.linalg.norm(h.astype(np.float64) - truth) / np.linalg.norm(truth))


def judge_root(tag, a, p, pad, h, met_row, bad):
  """The suite's root rule (test_eigh_root_hip_vs_reference_golden): at least as close to the float64 root
  as the reference over ssyevd, x 1.5 + 3e-6; symmetric to 1e-6 max|h|; DS:1017-1022 metrics."""
  with np.errstate(all="ignore"):   # the zero matrix: the power iteration normalises a zero vector
    truth = orc.eigh_root_float64(a, p, padding_start=pad)
    h_ref, m_ref = orc.matrix_inverse_pth_root_eigh(a, p, padding_start=pad)
  e_ref, e_hip = rel_fro(h_ref, truth), rel_fro(h, truth)
  print(f"EIGHROOT {tag} p={p} pad={pad} e_hip {e_hip:.2e} e_ref {e_ref:.2e} metric {met_row[0]:.2e} "
        f"(oracle {m_ref['inverse_pth_root_errors']:.2e}) sweeps {met_row[5]:.0f}")
  if not e_hip < 1.5 * e_ref + 3e-6 + ROOT_EXTRA.get((tag.split(" n=")[0], h.shape[0]), 0.0):
    bad.append((tag, p, "root error", e_hip, e_ref))
  if not np.abs(h - h.T).max() <= 1e-6 * np.abs(h).max():
    bad.append((tag, p, "asymmetry", float(np.abs(h - h.T).max() / np.abs(h).max())))
  if m_ref["inverse_pth_root_errors"] < 0.1 and not met_row[0] < 0.1:
    bad.append((tag, p, "error metric", float(met_row[0]), m_ref["inverse_pth_root_errors"]))
  if not (met_row[1:5] == 0).all():
    bad.append((tag, p, "metrics 1..4", met_row[1:5].tolist()))
  if pad is not None and pad < h.shape[0] and (h[pad:, :].any() or h[:, pad:].any()):
    bad.append((tag, p, "mass in the padded frame"))


SWEEP_FAMILIES = ("wishart", "psd_rank_deficient")


@functools.lru_cache(maxsize=None)
def plain_wishart(n):
  a = E.unscaled_case("wishart_x2^34", n)[0]
  a.setflags(write=False)
  return a


@pytest.mark.parametrize("n", E.SMALL_ROOT_SIZES)
def test_small_kernel_roots(n, device):
  """matrix_inverse_pth_root_batched(eigh=True) at n <= 128: families x p in one call, one padded block per
  size >= 64, the unscaled Wishart matrix as the control of the sweep count."""
  cases = [(name, reference(name, n)[0], p, None) for name in E.ROOT_FAMILIES_SMALL for p in E.ROOT_PS]
  cases += [("wishart", plain_wishart(n), p, None) for p in E.ROOT_PS]
  if n >= 64:
    ps = n - 7
    a = np.array(plain_wishart(n))
    a[ps:, :] = 0
    a[:, ps:] = 0
    cases.append(("wishart_padded", a, 4, ps))
  roots, met = K().matrix_inverse_pth_root_batched(
      [torch.tensor(np.array(a), device=device) for _, a, _, _ in cases], [p for _, _, p, _ in cases],
      [n if pad is None else pad for *_, pad in cases], eigh=True)
  met = met.cpu().numpy()
  bad = []
  for i, (name, a, p, pad) in enumerate(cases):
    judge_root(f"small {name} n={n}", a, p, pad, roots[i].cpu().numpy(), met[i], bad)
    key = ("wishart" if name == "wishart_padded" else name, n)
    if key[0] in SWEEP_FAMILIES and not met[i, 5] <= PARENT_SWEEPS[key]:
      bad.append((name, n, p, "sweeps", float(met[i, 5]), PARENT_SWEEPS[key]))
  assert not bad, bad


# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.BIG_SIZES)
def test_two_sided_solver_every_finite_family(n, device):
  names = E.names_for(n, E.FINITE)
  es, vs = eigh_call([reference(k, n)[0] for k in names], device, options={"eigh_solver": "two_sided"})
  bad = []
  for name, e, v in zip(names, es, vs):
    judge("two_sided", name, n, e, v, bad)
  assert not bad, bad


@pytest.mark.parametrize("n", E.BIG_SIZES)
def test_one_sided_solver_roots(n, device):
  """The Cholesky-Jacobi path and, where the factorisation breaks down, its two-sided fallback in the same
  call: the result is asserted, not the route; metrics column 5 > 0 says a Jacobi solver ran."""
  cases = [(name, reference(name, n)[0], E.ROOT_PS[i % len(E.ROOT_PS)])
           for i, name in enumerate(E.ROOT_FAMILIES_ONE_SIDED)]
  cases.append(("singular_psd", E.singular_psd(n), 2))
  roots, met = K().matrix_inverse_pth_root_batched(
      [torch.tensor(np.array(a), device=device) for _, a, _ in cases], [p for _, _, p in cases], eigh=True,
      options={"eigh_solver": "one_sided"})
  met = met.cpu().numpy()
  bad = []
  for i, (name, a, p) in enumerate(cases):
    h = roots[i].cpu().numpy()
    if name in ONE_SIDED_OUT_OF_RANGE:
      print(f"EIGHROOT one_sided {name} n={n} p={p} out of range: metric {met[i, 0]:.2e} "
            f"finite {bool(np.isfinite(h).all())} sweeps {met[i, 5]:.0f}")
      if not (np.isnan(h).any() or met[i, 0] >= 0.1):
        bad.append((name, n, "neither a NaN root nor a failure metric", float(met[i, 0])))
    else:
      judge_root(f"one_sided {name} n={n}", a, p, None, h, met[i], bad)
    if not met[i, 5] > 0:
      bad.append((name, n, "no Jacobi sweep ran", float(met[i, 5])))
  assert not bad, bad
