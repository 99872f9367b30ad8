"""Float64-referenced tests of the small kernels that decide whether a Frequent-Directions sketch update is right
(csrc/fd.hip: fd_round_control_kernel, fd_resnorm_part / fd_resnorm_sum / fd_bb; csrc/fd_update.hip: fd_prep_kernel,
fd_colnorm_part_kernel, fd_finish_kernel), which the suite compared only with themselves or through whole updates
on well-separated full-rank inputs.

Method (tests/_fd_round.py, gated on the CPU by test_fd_round_references.py): the stop rule, the preparation and
the finish are compared with NumPy float32 restatements of their expressions -- decisions, masks, zeros and every
correctly rounded field bit for bit, the powers and sums at derived ulp bounds -- on cases whose decisions float32
and float64 share by construction; one round and whole updates are compared with float64 references from the
definition, at bounds that are derived or measured on the CPU and recorded as constants there.  The preparation
and the finish run through ps_fd_prepare_f32 / ps_fd_finish_f32, the entry points ps_fd_update_batched_f32
itself calls.  Outputs live in NaN- / sentinel-framed holders where the wrapper takes an output.

Sensitivity: the comparisons used here are run on the CPU against seeded faults of the restatements (the floor
2.4e-7 halved, floorf -> roundf in the degree, the stride loop stopped after 256 factors, the ridge's two
branches, 0.99 / 1.01 widened to 0.9 / 1.1, the noise floor removed, deflated taken as e^2, the residual's ragged
rows skipped, theta not flipped, a dropped plane of C); each is caught on the cases listed.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _fd_round as R

pytestmark = pytest.mark.gpu

GUARD = 64
I32_SENT = -1515870811     # 0xA5A5A5A5
F32, F64 = np.float32, np.float64


def K():
  from precondition_amd import kernels
  return kernels


def _lib():
  from precondition_amd import _lib as L
  return L.lib()


def _stream():
  return torch.cuda.current_stream().cuda_stream


def _guarded_f32(shape, dev):
  n = int(np.prod(shape))
  holder = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
  return holder, holder[GUARD:GUARD + n].view(*shape)


def _guarded_i32(n, dev):
  holder = torch.full((n + 2 * GUARD,), I32_SENT, dtype=torch.int32, device=dev)
  return holder, holder[GUARD:GUARD + n]


def _guards_ok(holder, what):
  if holder.dtype == torch.float32:
    ok = bool(torch.isnan(holder[:GUARD]).all()) and bool(torch.isnan(holder[-GUARD:]).all())
  else:
    ok = bool((holder[:GUARD] == I32_SENT).all()) and bool((holder[-GUARD:] == I32_SENT).all())
  assert ok, f"{what}: written outside the output"


def _dev(a, dev):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------------------------------------------------------------------------------------------
# A. the stop rule: ps_fd_round_control_f32 against its restatement
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.CONTROL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_round_control_equals_the_restatement(device, shape):
  """converged, degree and the four summary words equal; ctr and e bit for bit; sigma1 within 2 ulp; nothing
  written outside the outputs.  Families mixed within each batch (tests/_fd_round.py control_cases); batch = 300
  runs the kernel's stride loop twice."""
  cases = [c for c in R.control_cases() if (c[1].shape[0], c[1].shape[1], c[3], c[4]) == tuple(shape)]
  assert cases
  for tag, th, rs, k, n, tol, degree in cases:
    batch, b = th.shape
    hp, params = _guarded_f32((batch, 4), device)
    hc, conv = _guarded_i32(batch, device)
    hs, summ = _guarded_i32(4, device)
    theta_d, res_d = _dev(th, device), _dev(rs, device)
    rc = _lib().ps_fd_round_control_f32(_stream(), theta_d.data_ptr(), res_d.data_ptr(), batch, b, k, n,
                                        float(tol), degree, params.data_ptr(), conv.data_ptr(), summ.data_ptr())
    assert rc == 0, (tag, rc)
    torch.cuda.synchronize()
    got = dict(params=params.cpu().numpy(), converged=conv.cpu().numpy(), summary=summ.cpu().numpy())
    try:
      R.check_control(got, R.control_ref(th, rs, k, n, tol, degree))
    except AssertionError as e:
      raise AssertionError((tag,) + e.args) from None
    for h, what in ((hp, "params"), (hc, "converged"), (hs, "summary")):
      _guards_ok(h, f"{tag} {what}")


# ---------------------------------------------------------------------------------------------------
# B. one round: ps_fd_round_f32 through subspace._Planned.round_call
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ROUND_CASES,
                         ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-{'x6' if c[3] else 'f32'}{'-spans' if c[4] else ''}")
def test_one_round_against_float64(device, case):
  """From the device's own x, z, theta of one round on C = Q diag(lambda) Q^T: orthonormality and z = C x at the
  bounds of the chol_rinv and six-product tests, theta against the float64 Rayleigh-Ritz values of span(x0) at
  4 x the float32 LAPACK round's own error, res against || z - theta x || at the derived rounding bound (the
  spanning start block puts the residuals themselves at rounding level), and the round's control outputs against
  the restatement evaluated on the device's theta and res."""
  from precondition_amd import subspace
  bsz, n, b, x6, spans = case
  c_np, x0_np = R.round_case(bsz, n, b, spans)
  k = max(b - 31, 1)
  cs = [_dev(c_np[j], device) for j in range(bsz)]
  hx, x = _guarded_f32((bsz, n, b), device)
  hz, z = _guarded_f32((bsz, n, b), device)
  x.copy_(_dev(x0_np, device))
  tmp = torch.empty_like(x)
  c16 = None
  if x6:
    assert K().fd_frag_supported(bsz, n, b)
    c16 = [K().to_bf16(c, split=True, tiled="frag3") for c in cs]
  pl = subspace._Planned(cs, x, z, tmp, c16x6=c16)
  rc = pl.round_call(k, R.ROUND_TOL, R.ROUND_DEGREE)
  assert rc is not None, "ps_fd_round_f32 must take this shape"
  torch.cuda.synchronize()
  theta, res, params, conv, summ = (t.cpu().numpy() for t in rc)
  xs, zs = x.cpu().numpy(), z.cpu().numpy()
  _guards_ok(hx, "x")
  _guards_ok(hz, "z")
  assert np.all(np.isfinite(xs)) and np.all(np.isfinite(zs)) and np.all(np.isfinite(theta))
  for j in range(bsz):
    try:
      fig = R.check_round(c_np[j], x0_np[j], xs[j], zs[j], theta[j], res[j])
    except AssertionError as e:
      raise AssertionError((f"factor {j}",) + e.args) from None
    print(f"factor {j}: " + "  ".join(f"{key} {val:.3g}" for key, val in fig.items()))
    if spans:
      assert fig["rho_rel"] < 1e-5       # residuals at rounding level: the first term of the bound decides
  unsafe = R.control_decisions_unsafe(theta, res, k, n, R.ROUND_TOL, R.ROUND_DEGREE)
  safe = np.array([w is None for w in unsafe])
  assert int((~safe).sum()) <= 1, unsafe
  R.check_control(dict(params=params, converged=conv, summary=summ),
                  R.control_ref(theta, res, k, n, R.ROUND_TOL, R.ROUND_DEGREE), factors=safe)


# ---------------------------------------------------------------------------------------------------
# C. prepare and finish through the entry points the update calls
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.PREPARE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_prepare_equals_the_restatement_bit_for_bit(device, shape):
  """ps_fd_prepare_f32: W = sketch * sqrt(eigs + ridge), every operation correctly rounded -> every bit; both
  `relative` modes, zero eigenvalues, a leading eigenvalue below error_tolerance."""
  cases = [c for c in R.prepare_cases() if c[1].shape[:2] + (c[2],) == tuple(shape)]
  assert len(cases) == 4
  for tag, prev, r, eps, tol, relative in cases:
    bsz, d = prev.shape[:2]
    holder, out = _guarded_f32((bsz, d, r), device)
    K().fd_prepare(_dev(prev, device), r, eps, tol, relative, out=out)
    torch.cuda.synchronize()
    want = R.prepare_ref(prev, r, eps, tol, relative)
    got = out.cpu().numpy()
    bad = np.argwhere(R.bits32(got) != R.bits32(want))
    assert not len(bad), (tag, len(bad), "first", tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    _guards_ok(holder, tag)


@pytest.mark.parametrize("shape", R.FINISH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_finish_equals_the_restatement(device, shape):
  """ps_fd_finish_f32 on Ritz values with a pair under the noise floor, a pair at the cutoff, negative values and
  a gap, Ritz vectors with unsafe (0.98, 1.02) and safe (0.992, 1.008) column norms, previous tails that make
  new_tail positive and zero, p = 2 and 4: deflated values, tail, has_zeros and every structural zero bit for
  bit; dropped columns exactly zero; kept entries within (d / 2 + 3) u of x / ||x_c||; inverted and const within
  2 ulp of the float64 power."""
  cases = [c for c in R.finish_cases() if c[2].shape + (c[5],) == tuple(shape)]
  assert len(cases) == 8
  for tag, th, x, prev, p, r, decay in cases:
    bsz, d, b = x.shape
    holder, out = _guarded_f32((bsz, d, r + 2), device)
    K().fd_finish(_dev(th, device), _dev(x, device), _dev(prev, device), p, r, decay, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for j in range(bsz):
      ref = R.finish_ref(th[j], x[j], prev[j], p, r, decay)
      assert R.finish_margins_ok(ref)
      try:
        R.check_finish(got[j], ref, x[j])
      except AssertionError as e:
        raise AssertionError((tag, f"factor {j}") + e.args) from None
    _guards_ok(holder, tag)


def test_prepare_and_finish_refuse_bad_arguments(device):
  """PS_EINVAL for nulls, rank + 1 > b and rank + 2 >= d; the scratch query is batch * 32 * rank floats."""
  L = _lib()
  t = torch.zeros((4096,), dtype=torch.float32, device=device)
  p, s = t.data_ptr(), _stream()
  assert L.ps_fd_finish_scratch_bytes(3, 7) == 3 * 32 * 7 * 4
  assert L.ps_fd_prepare_f32(s, None, p, 1, 16, 4, 1e-6, 1e-6, 1) == -1
  assert L.ps_fd_prepare_f32(s, p, None, 1, 16, 4, 1e-6, 1e-6, 1) == -1
  assert L.ps_fd_prepare_f32(s, p, p, 1, 6, 4, 1e-6, 1e-6, 1) == -1            # rank + 2 >= d
  assert L.ps_fd_prepare_f32(s, p, p, 0, 16, 4, 1e-6, 1e-6, 1) == -1
  for missing in range(5):
    args = [p] * 5
    args[missing] = None
    assert L.ps_fd_finish_f32(s, *args, 1, 16, 8, 4, 2, 0.999) == -1
  assert L.ps_fd_finish_f32(s, p, p, p, p, p, 1, 16, 4, 4, 2, 0.999) == -1     # rank + 1 > b
  assert L.ps_fd_finish_f32(s, p, p, p, p, p, 1, 6, 8, 4, 2, 0.999) == -1      # rank + 2 >= d
  assert L.ps_fd_finish_f32(s, p, p, p, p, p, 1, 16, 8, 4, 0, 0.999) == -1     # p < 1
  torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# D. whole updates at the fused path's smallest shapes against the definition in float64
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.UPDATE_SHAPES, ids=lambda s: f"d{s[0]}r{s[1]}x{s[2]}")
@pytest.mark.parametrize("kind", R.UPDATE_KINDS)
def test_whole_update_against_the_definition(device, kind, shape):
  """ps_fd_update_batched_f32 against update_ref (DS:1123-1290 in float64 with the kernel's noise floor): a
  full-rank separated spectrum chained twice under the absolute ridge, a Gram matrix of rank r - 3 from a zero
  sketch (the last three columns exactly zero, has_zeros 1), an all-zero block on a zero sketch (finite, all
  zero, has_zeros 1) and on a non-zero one (pure decay).  Masks, zeros and flags exactly; scalar fields and the
  projector on the kept columns within max(4 x the float32-LAPACK oracle's own error, tol * top / gap)."""
  d, r, bsz = shape
  case = R.update_case(kind, d, r, bsz)
  prev = _dev(case["prev0"], device)
  x0 = _dev(case["x0"], device)
  for step, grams in enumerate(case["steps"]):
    res = K().fd_update_batched([_dev(grams[j], device) for j in range(bsz)], prev, R.UPDATE_P, r, R.UPDATE_DECAY,
                                R.UPDATE_RIDGE, 1e-6, case["relative"], x0, tol=R.UPDATE_TOL)
    assert res is not None, "the fused path must take this shape"
    out, conv, info = res
    torch.cuda.synchronize()
    got, prev_np = out.cpu().numpy(), prev.cpu().numpy()
    assert conv.cpu().numpy().tolist() == [1] * bsz, (step, conv.cpu().numpy(), info)
    for j in range(bsz):
      ref, rinfo = R.update_ref(prev_np[j], grams[j], R.UPDATE_P, r, relative=case["relative"])
      assert rinfo["margin"] >= 100.0, ("an eigenvalue near the noise floor", rinfo["margin"])
      what = (kind, f"step {step}", f"factor {j}")
      try:
        R.check_update_exact(got[j], ref, r)
      except AssertionError as e:
        raise AssertionError(what + e.args) from None
      scalar, proj = R.update_errors(got[j], ref, r)
      bs = R.update_bound(R.UPDATE_ORACLE_SCALAR, rinfo)
      bp = R.update_bound(R.UPDATE_ORACLE_PROJECTOR, rinfo)
      print(f"{what}: scalar {scalar:.3g} (bound {bs:.3g})  projector {proj:.3g} (bound {bp:.3g})  "
            f"rounds {info['outer_iterations']}")
      assert scalar <= bs, what + ("scalar fields", scalar, bs)
      assert proj <= bp, what + ("projector", proj, bp)
      if kind == "rank_deficient":
        assert not np.any(got[j][:, r - 3:r]) and got[j][-1, -2] == 1.0
        assert not np.any(got[j][-3:, -1]) and not np.any(got[j][r - 3:r, -2])
      if kind == "zero_zero":
        assert not np.any(got[j][:-1]) and not np.any(got[j][-1, :-2]) and got[j][-1, -1] == 0
        assert got[j][-1, -2] == 1.0
      if kind in ("chained", "pure_decay"):
        assert got[j][-1, -2] == 0.0 and got[j][1, -1] > 0
    prev = out
