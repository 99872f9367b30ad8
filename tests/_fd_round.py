"""References, case lists and comparisons shared by test_fd_round_references.py (CPU) and test_gpu_fd_round.py
(GPU) for the small kernels that decide whether a Frequent-Directions sketch update is right:

  fd_round_control_kernel                       csrc/fd.hip          stop rule, Chebyshev interval and degree
  fd_resnorm_part / fd_resnorm_sum / fd_bb      csrc/fd.hip          residual norms, symmetrisation, flip
  fd_prep_kernel, fd_colnorm_part_kernel,       csrc/fd_update.hip   W = sketch sqrt(eigs + ridge); deflation,
  fd_finish_kernel                                                   masks, inverted eigenvalues, packing

Nothing here imports precondition_amd.  Every reference is NumPy; the float32 restatements round after every
operation like the kernels' explicit __fmul_rn / __fadd_rn / sqrtf / division (all correctly rounded under the
build's flags), the float64 references follow the definition (DS:1123-1290).

Comparisons live here too (`check_*`), so that the CPU file can run them on MUTANTS of the restatements
(`mutate=` below): a comparison that lets a mutant through on the listed cases would let the same fault of a
kernel through.  u = 2^-24 throughout.
"""
import functools

import numpy as np

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24

# seeded faults of the restatements (the CPU file shows that every comparison below catches its own)
MUTATIONS = ("noise_1.2e-7", "round_degree", "stride_256",                      # control_ref
             "ridge_ignores_relative", "ridge_without_tolerance",                # prepare_ref
             "wide_safe", "no_noise_floor", "deflated_e2",                       # finish_ref
             "residual_skips_ragged_rows", "theta_ascending", "cx_two_planes")   # round_outputs_f32


def ulp32(x):
  """Spacing of float32 at |x| (the smallest subnormal at 0)."""
  return np.spacing(np.abs(np.asarray(x, F64)).astype(F32)).astype(F64)


def bits32(x):
  return np.ascontiguousarray(x, F32).view(np.uint32)


# =====================================================================================================
# A. fd_round_control_kernel
# =====================================================================================================
def _acosh(v, dt):
  """fd_acosh: v clamped to [1, 1e30] (fmaxf / fminf drop a NaN operand), log(v) + log1p(sqrt(max(1 - 1/v^2, 0)))."""
  one = dt(1.0)
  v = np.fmin(np.fmax(v, one), dt(F32(1e30)))
  with np.errstate(over="ignore"):
    vv = dt(v * v)
  return dt(np.log(v)) + dt(np.log1p(dt(np.sqrt(np.fmax(dt(one - dt(one / vv)), dt(0.0))))))


def _range32(x, dt):
  """The float64 twin keeps float32's exponent range: a product below half the smallest subnormal is 0 (the
  kernel's results for theta[0] <= 0, where 1e-30 * 1e-30 underflows, are defined by it)."""
  if dt is F64 and abs(x) < 2.0 ** -150:
    return dt(0.0)
  return x


def control_ref(theta, res, k, n, tol, degree, dtype=F32, mutate=()):
  """fd_round_control_kernel, expression by expression, in `dtype` (float32: the restatement; float64: its twin
  on the same float32 inputs and the same float32 constants).  theta, res: [batch, b].  Returns a dict:
  params [batch, 4] = {ctr, e, sigma1, degree}, converged [batch] int32, summary [4] int32 = {all converged,
  max degree, min degree, any res[i] / top > 2e-2 among the first k}, and q [batch] = 4.6 / spread (what the
  degree is the clamped floor of) for the decision checker."""
  dt = dtype
  theta = np.asarray(theta, F32)
  res = np.asarray(res, F32)
  batch, b = theta.shape
  c = lambda v: dt(F32(v))           # a float literal of the kernel
  nfloor = c(1.2e-7) if "noise_1.2e-7" in mutate else c(2.4e-7)
  params = np.zeros((batch, 4), dt)
  conv = np.zeros((batch,), np.int32)
  q = np.zeros((batch,), dt)
  s_all, s_max, s_min, s_plain = 1, 1, int(degree), 0
  written = np.ones((batch,), bool)
  with np.errstate(all="ignore"):
    for j in range(batch):
      if "stride_256" in mutate and j >= 256:
        written[j] = False
        continue
      th = theta[j].astype(dt)
      rs = res[j].astype(dt)
      top = np.fmax(th[0], c(1e-30))
      wanted_above = dt(dt(dt(n) * nfloor) * top)
      tol_top = dt(dt(F32(tol)) * top)
      cv, plain = True, False
      for i in range(k):
        wanted = bool(th[i] > wanted_above)
        cv = cv and (bool(rs[i] <= tol_top) or not wanted)
        plain = plain or bool(dt(rs[i] / top) > c(2e-2))
      cut = np.fmax(th[b - 1], dt(0.0))
      tiny = _range32(dt(c(1e-30) * top), dt)
      e = np.fmax(dt(c(0.5) * cut), tiny)
      ctr = dt(c(0.5) * cut)
      a0 = dt(top * dt(F32(F32(1.0) + F32(1e-6))))
      sigma1 = dt(e / dt(a0 - ctr))
      xk = np.fmax(th[k - 1], tiny)
      spread = np.fmax(dt(_acosh(dt(dt(top - ctr) / e), dt) - _acosh(dt(dt(xk - ctr) / e), dt)), c(1e-6))
      qj = dt(c(4.6) / spread)
      whole = np.round(qj) if "round_degree" in mutate else np.floor(qj)
      deg = np.fmin(np.fmax(whole, dt(1.0)), dt(degree))
      params[j] = (ctr, e, sigma1, deg)
      conv[j] = 1 if cv else 0
      q[j] = qj
      s_all &= int(cv)
      s_max = max(s_max, int(deg))
      s_min = min(s_min, int(deg))
      s_plain |= int(plain)
  return dict(params=params, converged=conv, summary=np.array([s_all, s_max, s_min, s_plain], np.int32), q=q,
              written=written)


def control_decisions_unsafe(theta, res, k, n, tol, degree):
  """Per factor: None where float32 and float64 must take every decision of the kernel alike, else the reason.
  Evaluated in float64 on the float32 inputs:
    each res[i] (i < k) is off tol * top by a relative 1e-3 or more       (converged)
    each theta[i] (i < k) is off n * 2.4e-7 * top by a relative 1e-3      (wanted)
    res[i] / top is off 2e-2 by a relative 1e-3                           (plain flag)
    q = 4.6 / spread is off every integer by 1e-3 of q's value            (degree = clamp(floor(q), 1, degree))
  The float32 evaluation of each left side is good to a few ulp (1e-6), the device's logf / log1pf to a few more.
  A NaN residual compares false in both precisions and is safe.  Of the integers only 2 .. degree can change the
  clamped degree (below 2 the clamp at 1 decides, above `degree` the clamp at `degree`), so those are the
  integers q is held off: a factor with q = 4.6e6 (spread at its floor 1e-6, k = 1) has no decision left."""
  theta = np.asarray(theta, F32)
  res = np.asarray(res, F32)
  r64 = control_ref(theta, res, k, n, tol, degree, dtype=F64)
  out = []
  for j in range(theta.shape[0]):
    th, rs = theta[j, :k].astype(F64), res[j, :k].astype(F64)
    top = max(float(theta[j, 0]), float(F32(1e-30)))
    why = None

    def off(vals, mark):
      vals = vals[~np.isnan(vals)]
      return bool(np.all(np.abs(vals - mark) >= 1e-3 * abs(mark)))
    if not off(rs, float(F32(tol)) * top):
      why = "a residual at tol * top"
    elif not off(th, n * float(F32(2.4e-7)) * top):
      why = "a Ritz value at the noise floor"
    elif not off(rs / top, float(F32(2e-2))):
      why = "a relative residual at 2e-2"
    else:
      qj = float(r64["q"][j])
      ints = np.arange(2, int(degree) + 1, dtype=F64)
      if not np.isfinite(qj) or (ints.size and np.min(np.abs(qj - ints)) < 1e-3 * abs(qj)):
        why = "4.6 / spread at an integer"
    out.append(why)
  return out


def assert_control_decisions_safe(theta, res, k, n, tol, degree):
  bad = [(j, w) for j, w in enumerate(control_decisions_unsafe(theta, res, k, n, tol, degree)) if w]
  assert not bad, bad


def check_control(got, ref, factors=None):
  """got / ref: dicts like control_ref's.  converged, degree and the summary words equal; ctr and e bit for bit
  (only exact halvings and maxima); sigma1 within 2 float32 ulp (fd.hip is built with contraction on: a0 - ctr
  may be one fused operation).  factors: mask of the factors to compare (the summary is compared only when all
  are)."""
  gp, rp = np.asarray(got["params"], F32), np.asarray(ref["params"], F32)
  m = np.ones(len(rp), bool) if factors is None else np.asarray(factors, bool)
  assert gp.shape == rp.shape
  gc, rc = np.asarray(got["converged"]), np.asarray(ref["converged"])
  assert np.array_equal(gc[m], rc[m]), ("converged", np.flatnonzero((gc != rc) & m)[:8])
  assert np.array_equal(bits32(gp[m, 3]), bits32(rp[m, 3])), \
      ("degree", np.flatnonzero((gp[:, 3] != rp[:, 3]) & m)[:8], gp[m, 3][:8], rp[m, 3][:8])
  assert np.array_equal(bits32(gp[m, 0:2]), bits32(rp[m, 0:2])), "ctr / e differ in a bit"
  ds = np.abs(gp[m, 2].astype(F64) - rp[m, 2].astype(F64))
  assert np.all(ds <= 2 * ulp32(rp[m, 2])), ("sigma1", float(np.max(ds / ulp32(rp[m, 2]))))
  if m.all():
    assert np.array_equal(np.asarray(got["summary"]), np.asarray(ref["summary"])), \
        ("summary", list(got["summary"]), list(ref["summary"]))


# (batch, b, k, n): k == b once; batch > 256 runs the kernel's stride loop twice
CONTROL_SHAPES = ((1, 32, 1, 100), (3, 64, 33, 256), (16, 96, 96, 1024), (300, 40, 9, 131))
CONTROL_TOL = 1e-5
CONTROL_DEGREE = 12
CONTROL_FAMILIES = ("converged", "unconverged", "unwanted_large", "negative_tail", "nonpositive_top", "nan_residual",
                    "degree_1", "degree_max")


def _control_factor(family, b, k, n, big, rng):
  """(theta [b], res [b]) of one factor.  `big`: the relative size of the residuals that are not small (0.5: above
  2e-2, sets the plain flag; 1e-2: below it, still far above tol)."""
  top = float(2.0 ** rng.integers(-6, 7) * rng.uniform(1.0, 2.0))
  g = {"degree_max": 0.97}.get(family, float(rng.uniform(0.05, 0.5)))
  i = np.arange(b) / max(b - 1, 1)
  theta = top * g ** i * (1.0 - 0.2 / b * rng.uniform(0, 1, b))
  if family == "degree_1":     # a drop of 1e3 behind the first value: the spread of top against theta[k - 1] exceeds 4.6
    theta[1:] = top * 1e-3 * 0.5 ** i[1:]
  theta = np.sort(theta)[::-1].copy()
  res = CONTROL_TOL * top * rng.uniform(0.05, 0.5, b)
  floor = n * 2.4e-7 * top
  if family == "unconverged":
    res[int(rng.integers(0, k))] = CONTROL_TOL * top * 10.0
    res[k:] = big * top
  elif family == "unwanted_large":
    # from i0 on the pairs sit in the noise floor (the first at 0.75 of it: wanted under a floor of half the
    # size); their residuals are large and must not block convergence
    i0 = max(1, k - 2)
    theta[i0:] = floor * 0.75 * 0.5 ** np.arange(b - i0)
    res[i0:] = big * top
  elif family == "negative_tail":
    m = max(1, b // 8)
    theta[b - m:] = -top * np.linspace(0.01, 0.05, m)
    res[b - m:] = big * top
  elif family == "nonpositive_top":
    theta = -top * np.linspace(0.0 if rng.integers(0, 2) else 0.1, 1.0, b)
    res[:] = 0.0 if big < 2e-2 else 1e-3 * top      # top is 1e-30 here: any non-zero residual sets the plain flag
  elif family == "nan_residual":
    res[int(rng.integers(0, k))] = np.nan
  return theta.astype(F32), res.astype(F32)


@functools.lru_cache(maxsize=None)
def control_cases():
  """[(tag, theta [batch, b], res, k, n, tol, degree)]: every shape with the families mixed within the batch
  (factor j of variant v is family (v + j) mod 8), with large residuals above (plain flag 1) and below 2e-2
  (plain flag 0).  A factor is redrawn until assert_control_decisions_safe accepts it and its family's property
  holds, so no case is left out."""
  cases = []
  nf = len(CONTROL_FAMILIES)
  for si, (batch, b, k, n) in enumerate(CONTROL_SHAPES):
    variants = range(nf) if batch < nf else range(2)
    for v in variants:
      for big in (0.5, 1e-2):
        rng = np.random.default_rng([1729, si, v, int(big * 100)])
        th, rs = np.zeros((batch, b), F32), np.zeros((batch, b), F32)
        for j in range(batch):
          fam = CONTROL_FAMILIES[(v + j) % nf]
          for _ in range(200):
            t1, r1 = _control_factor(fam, b, k, n, big, rng)
            if control_decisions_unsafe(t1[None], r1[None], k, n, CONTROL_TOL, CONTROL_DEGREE)[0] is None and \
               _family_holds(fam, t1, r1, k, n):
              break
          else:
            raise AssertionError(("no safe factor", fam, batch, b, k))
          th[j], rs[j] = t1, r1
        cases.append((f"{batch}x{b}k{k}-v{v}-big{big}", th, rs, k, n, CONTROL_TOL, CONTROL_DEGREE))
  return cases


def _family_holds(fam, th, rs, k, n):
  r = control_ref(th[None], rs[None], k, n, CONTROL_TOL, CONTROL_DEGREE, dtype=F64)
  conv, deg = int(r["converged"][0]), float(r["params"][0, 3])
  if fam in ("converged", "unwanted_large", "nonpositive_top"):
    return conv == 1
  if fam in ("unconverged", "nan_residual"):
    return conv == 0
  if fam == "negative_tail":
    return float(r["params"][0, 0]) == 0.0 and float(r["params"][0, 1]) > 0.0
  if fam == "degree_1":
    # with k == 1 the wanted value is the top one: the spread is at its floor and the degree at its cap
    return deg == (1.0 if k > 1 else float(CONTROL_DEGREE))
  if fam == "degree_max":
    return deg == float(CONTROL_DEGREE)
  return True


# =====================================================================================================
# B. one round: known spectra, Ritz reference, residual bound
# =====================================================================================================
# (bsz, n, b, three-plane path, start block spans the leading invariant subspace)
ROUND_CASES = ((2, 131, 40, False, False), (1, 100, 33, False, False), (3, 256, 96, False, False),
               (2, 256, 64, True, False), (1, 384, 96, True, False), (1, 100, 33, False, True),
               (2, 256, 64, True, True))
ROUND_TOL = 1e-5
ROUND_DEGREE = 12

# Orthonormality of the round's x, max |x^T x - I|: tests/test_gpu_round4.py
# test_chol_rinv_against_float64_cholesky holds R^-T G R^-1 - I to 5e-5 sqrt(cond G); the Newton-Schulz polish
# that follows CholeskyQR in a round squares that deviation (I + D -> I + O(D^2)), which leaves the float32
# products' own rounding: the figure at cond = 1.
ROUND_ORTH_BOUND = 5e-5
# || z - C x ||_F / ||C||_2: tests/test_gpu_round4.py test_six_product_cx_has_float32_accuracy holds
# || z - C x ||_F <= 3e-7 || C x ||_F <= 3e-7 ||C||_2 ||x||_F for one product.  The round's x and z are both
# rotated by the Ritz basis afterwards (x <- x y, z <- z y: two more float32 products of the same class), so
# z - C x carries three such errors; ||x||_F = sqrt(b) for orthonormal columns.
ROUND_CX_REL = 3 * 3e-7          # times sqrt(b)

# Ritz values: worst |theta32 - ritz_ref| / theta_ref[0] of `round_f32` (a NumPy float32 evaluation of the same
# round with LAPACK ssyevd) over ROUND_CASES, measured on the CPU (test_fd_round_references.py re-measures it and
# holds it within [1/4, 3/2] of this figure: the BLAS blocking moves it).  The GPU gets 4 x: the margin covers the
# three bf16 planes and another summation order.
ROUND_RITZ_F32_MEASURED = 3.2e-7
ROUND_RITZ_BOUND = 4 * ROUND_RITZ_F32_MEASURED


def round_spectrum(n):
  """Graded: 0.85^i over a floor of 1e-4 (positive definite, ||C||_2 = 1 + 1e-4)."""
  return 0.85 ** np.arange(n) + 1e-4


@functools.lru_cache(maxsize=None)
def round_case(bsz, n, b, spans):
  """(C [bsz, n, n] float32 = Q diag(lambda) Q^T rounded, x0 [bsz, n, b] float32).  spans: x0 = Q[:, :b] M with a
  well-conditioned b x b mixing M, so the first Rayleigh-Ritz already finds eigenvectors."""
  rng = np.random.default_rng([99, bsz, n, b, int(spans)])
  cs, xs = [], []
  for _ in range(bsz):
    q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    c = (q * round_spectrum(n)) @ q.T
    cs.append((0.5 * (c + c.T)).astype(F32))
    if spans:
      m = np.linalg.qr(rng.standard_normal((b, b)))[0] * rng.uniform(0.5, 2.0, b)
      xs.append((q[:, :b] @ m).astype(F32))
    else:
      xs.append(rng.standard_normal((n, b)).astype(F32))
  return np.stack(cs), np.stack(xs)


def ritz_ref(c, x0):
  """Float64 Rayleigh-Ritz of C on span(x0): eigenvalues of Q^T C Q, Q from a QR of x0, descending."""
  c = np.asarray(c, F64)
  q = np.linalg.qr(np.asarray(x0, F64))[0]
  t = q.T @ (0.5 * (c + c.T)) @ q
  return np.linalg.eigvalsh(0.5 * (t + t.T))[::-1].copy()


def round_f32(c, x0):
  """The round of ps_fd_round_f32 in NumPy float32: G = x^T x, M = R^-1 of its Cholesky factor (float64 inside,
  like the device), x <- (x M)(1.5 I - 0.5 (xM)^T (xM)), z = C x, T = x^T z, ssyevd of (T + T^T) / 2.  Returns
  theta descending (float32)."""
  from oracle import lapack32
  c, x = np.asarray(c, F32), np.asarray(x0, F32)
  b = x.shape[1]
  g = (x.T @ x).astype(F64)
  m = np.linalg.inv(np.linalg.cholesky(0.5 * (g + g.T))).T.astype(F32)
  t = x @ m
  pol = (F32(1.5) * np.eye(b, dtype=F32) + F32(-0.5) * (t.T @ t)).astype(F32)
  x = t @ pol
  z = c @ x
  tt = x.T @ z
  w, _ = lapack32.eigh32(np.ascontiguousarray(tt))
  return w[::-1].copy()


def round_outputs_f32(c, x0, mutate=()):
  """(x, z, theta, res) of round_f32's round, all float32, as the device leaves them: Ritz vectors x <- x y,
  z <- z y, theta descending, res_c = || z_c - theta_c x_c ||.  The CPU stand-in for the device in check_round."""
  from oracle import lapack32
  c, x = np.asarray(c, F32), np.asarray(x0, F32)
  n, b = x.shape
  g = (x.T @ x).astype(F64)
  m = np.linalg.inv(np.linalg.cholesky(0.5 * (g + g.T))).T.astype(F32)
  t = x @ m
  x = t @ (F32(1.5) * np.eye(b, dtype=F32) + F32(-0.5) * (t.T @ t)).astype(F32)
  cc = c
  if "cx_two_planes" in mutate:    # C to 16 bits of significand instead of 24: a dropped bf16 plane
    cc = (c.view(np.uint32) & np.uint32(0xFFFFFF00)).view(F32)
  z = cc @ x
  tt = x.T @ z
  w, v = lapack32.eigh32(np.ascontiguousarray(tt))
  theta, y = w[::-1].copy(), np.ascontiguousarray(v[:, ::-1])
  x, z = x @ y, z @ y
  dlt = z - x * theta[None, :]
  rows = (n // 32) * 32 if "residual_skips_ragged_rows" in mutate else n
  res = np.sqrt(np.sum(dlt[:rows] * dlt[:rows], axis=0, dtype=F32))
  if "theta_ascending" in mutate:
    theta = theta[::-1].copy()
  return x, z, theta, res


def check_round(c, x0, x, z, theta, res):
  """One factor of a round, in float64 from the device's own x, z, theta (see the constants above):
  orthonormality, z = C x, theta against ritz_ref, res against the derived residual bound."""
  c64, x64, z64 = np.asarray(c, F64), np.asarray(x, F64), np.asarray(z, F64)
  n, b = x64.shape
  orth = float(np.max(np.abs(x64.T @ x64 - np.eye(b))))
  assert orth <= ROUND_ORTH_BOUND, ("orthonormality", orth)
  norm_c = float(np.linalg.norm(c64, 2))
  cx = float(np.linalg.norm(z64 - c64 @ x64) / norm_c)
  assert cx <= ROUND_CX_REL * np.sqrt(b), ("z - C x", cx, ROUND_CX_REL * np.sqrt(b))
  want = ritz_ref(c, x0)
  et = float(np.max(np.abs(np.asarray(theta, F64) - want)) / want[0])
  assert et <= ROUND_RITZ_BOUND, ("theta against the float64 Ritz values", et, ROUND_RITZ_BOUND)
  rho, bound = residual_bound(x, z, theta, n)
  er = np.abs(np.asarray(res, F64) - rho)
  assert np.all(er <= bound), ("residual norms", int(np.argmax(er / bound)), float(np.max(er / bound)))
  return dict(orth=orth, cx=cx, theta=et, res=float(np.max(er / bound)), rho_rel=float(np.max(rho) / want[0]))


def residual_bound(x, z, theta, n):
  """Per column c the bound on |res_c - rho_c|, rho_c = || z_c - theta_c x_c ||_2 in float64 from the float32 x, z
  and theta that the kernel read:

      |res - rho| <= u (||z_c|| + 2 |theta_c| ||x_c||) + ((n + 4) / 2) u rho

  First term: the kernel forms d_i = fl(z_i - x_i theta).  Uncontracted that is (z_i - x_i theta (1 + e1))(1 + e2),
  |e| <= u: off the exact difference by at most u |x_i theta| + u |z_i - x_i theta| <= u (|z_i| + 2 |x_i theta|);
  one fused operation is off by less.  As vectors: || d - (z - theta x) ||_2 <= u (||z|| + 2 |theta| ||x||), and
  the norm of d is within that of rho.  Second term: the sum of the n squares in ANY order (per thread, per row
  group, per chunk; fused or not) puts at most n + 1 roundings on a term, a relative (n + 1) u on the sum and half
  of it on the root; the square root rounds once more: ((n + 1) / 2 + 1) u <= ((n + 4) / 2) u with the second-order
  terms.  Where the start block already spans an invariant subspace rho is itself at rounding level and only the
  first term keeps the assertion honest."""
  x, z, theta = np.asarray(x, F64), np.asarray(z, F64), np.asarray(theta, F64)
  rho = np.linalg.norm(z - x * theta[None, :], axis=0)
  first = U * (np.linalg.norm(z, axis=0) + 2 * np.abs(theta) * np.linalg.norm(x, axis=0))
  return rho, first + (n + 4) / 2 * U * rho


# =====================================================================================================
# C. prepare and finish
# =====================================================================================================
def unpack(packed, r):
  """(sketch [d, r], deflated [r], inverted [r], const, tail, has_zeros) of the [d, r + 2] layout (DS:555-592)."""
  p = np.asarray(packed)
  return p[:, :r], p[-r:, -1], p[:r, -2], p[0, -1], p[1, -1], p[-1, -2]


def pack(sketch, deflated, inverted, const, tail, has_zeros, dtype=F32):
  d, r = sketch.shape
  p = np.zeros((d, r + 2), dtype)
  p[:, :r] = sketch
  p[:r, -2] = inverted
  p[-1, -2] = 1.0 if has_zeros else 0.0
  p[0, -1] = const
  p[1, -1] = tail
  p[-r:, -1] = deflated
  return p


def prepare_ref(prev, rank, ridge_epsilon, error_tolerance, relative, mutate=()):
  """fd_prep_kernel term for term in float32: ridge = ridge_epsilon * max(relative ? fwd[0] : 1, error_tolerance),
  W[:, c] = sketch[:, c] * sqrt(fwd[c] + ridge).  prev [B, d, r + 2] -> [B, d, r]."""
  prev = np.asarray(prev, F32)
  r = rank
  out = np.zeros(prev.shape[:2] + (r,), F32)
  for j in range(prev.shape[0]):
    fwd = prev[j, -r:, -1]
    lead = fwd[0] if relative else F32(1.0)
    if "ridge_ignores_relative" in mutate:
      lead = F32(1.0)
    ridge = F32(F32(ridge_epsilon) * np.fmax(lead, F32(error_tolerance)))
    if "ridge_without_tolerance" in mutate:
      ridge = F32(F32(ridge_epsilon) * lead)
    out[j] = prev[j, :, :r] * np.sqrt((fwd + ridge).astype(F32))[None, :]
  return out


def finish_ref(theta, x, prev, p, rank, decay, mutate=()):
  """fd_colnorm_part_kernel + fd_finish_kernel for ONE factor, term for term in float32 (theta [b], x [d, b],
  prev [d, r + 2]); the column norms are summed in float64.  Returns a dict: the bit-exact fields
  (deflated [r], tail, has_zeros, up [r] = the argument of the inverted power, new_tail_arg), the norms
  (nrm [r] float64, the value the kernel's float32 sum approximates), keep [r] (columns that stay), and
  inverted64 [r] / const64: the float64 power with the float32 exponent alpha = float32(-1 / p)."""
  theta, x, prev = np.asarray(theta, F32), np.asarray(x, F32), np.asarray(prev, F32)
  d, r = x.shape[0], rank
  emax = np.max(theta[:r + 1])
  noise = F32(F32(F64(d) * 1.2e-7) * np.fmax(emax, F32(0.0)))
  if "no_noise_floor" in mutate:
    v = theta[:r + 1].copy()
  else:
    v = np.where(theta[:r + 1] <= noise, F32(0.0), theta[:r + 1]).astype(F32)
  e = np.sqrt(np.fmax(v, F32(0.0))).astype(F32)
  cutoff = e[r]
  rho = F32(cutoff * cutoff)
  tail = F32(prev[1, -1] * F32(decay))
  new_tail_arg = F32(tail + rho)
  alpha = F32(-1.0 / F64(p))
  new_tail = F32(0.0) if new_tail_arg <= 0 else new_tail_arg
  with np.errstate(all="ignore"):
    const64 = 0.0 if new_tail_arg <= 0 else float(np.power(F64(new_tail_arg), F64(alpha)))
  if "deflated_e2" in mutate:
    dv = (e[:r] * e[:r]).astype(F32)
  else:
    dv = ((e[:r] - cutoff).astype(F32) * (e[:r] + cutoff).astype(F32)).astype(F32)
  defl = np.where(dv <= 0, F32(0.0), dv).astype(F32)
  nrm64 = np.sqrt(np.sum(x[:, :r].astype(F64) ** 2, axis=0))
  nrm = np.where(defl > 0, nrm64.astype(F32), F32(0.0)).astype(F32)
  lo, hi = (F32(0.9), F32(1.1)) if "wide_safe" in mutate else (F32(0.99), F32(1.01))
  safe = (lo <= nrm) & (nrm <= hi)
  keep = (defl > 0) & safe
  defl_out = np.where(safe, defl, F32(0.0)).astype(F32)
  up = ((e[:r] * e[:r]).astype(F32) + tail).astype(F32)
  up = np.where(defl_out > 0, up, F32(0.0)).astype(F32)
  up = np.where(up <= 0, F32(0.0), up).astype(F32)
  with np.errstate(all="ignore"):
    inv64 = np.where(up <= 0, 0.0, np.power(np.where(up <= 0, 1.0, up.astype(F64)), F64(alpha)))
  zeros = bool(new_tail <= 0) or bool(np.any(defl_out <= 0))
  return dict(deflated=defl_out, tail=new_tail, has_zeros=F32(1.0 if zeros else 0.0), up=up, keep=keep,
              positive=defl > 0, nrm=nrm64, inverted64=inv64, const64=const64, noise=noise, rank=r, d=d)


def finish_margins_ok(ref):
  """The column norms of columns with a positive deflated value sit 2e-3 or more from 0.99 and 1.01: the float32
  norm of the kernel (another summation order, (d / 2 + 3) u off) takes the same decision."""
  n = ref["nrm"][ref["positive"]]
  # (0.992 and 1.008 are 2e-3 off by construction; the float32 rounding of the columns moves them by 1e-7)
  return bool(np.all(np.minimum(np.abs(n - 0.99), np.abs(n - 1.01)) >= 2e-3 * (1 - 1e-3)))


def finish_packed(ref, x):
  """The packed float32 output of a kernel that evaluates finish_ref's values correctly rounded (what check_finish
  accepts with no error at all): the CPU file feeds MUTANTS of finish_ref through it."""
  r = ref["rank"]
  nrm = np.where(ref["keep"], ref["nrm"], 1.0)
  sketch = np.where(ref["keep"][None, :], np.asarray(x, F64)[:, :r] / nrm[None, :], 0.0)
  return pack(sketch, ref["deflated"], ref["inverted64"], ref["const64"], ref["tail"], bool(ref["has_zeros"]))


def check_finish(got, ref, x):
  """got: one factor's packed output [d, r + 2] (float32); ref: finish_ref's dict; x: the Ritz vectors given.
  - the last column but const, the has_zeros word and every structural zero: bit for bit;
  - dropped columns exactly zero; kept entries within (d / 2 + 3) u relative of x / ||x_c||_2: d squares summed in
    another order (d u on the sum, half on the root), a square root and a division (u each), second order below u;
  - inverted and const within 2 float32 ulp of the float64 power with the float32 exponent (device powf: 1 ulp,
    documented; one more for the rounding of the result)."""
  got = np.asarray(got, F32)
  r, d = ref["rank"], ref["d"]
  assert got.shape == (d, r + 2)
  exp_last = np.zeros((d,), F32)
  exp_last[1] = ref["tail"]
  exp_last[d - r:] = ref["deflated"]
  rows = np.arange(d) != 0
  assert np.array_equal(bits32(got[rows, -1]), bits32(exp_last[rows])), \
      ("last column", np.flatnonzero(bits32(got[:, -1]) != bits32(exp_last))[:8])
  assert bits32(got[-1, -2]) == bits32(ref["has_zeros"]), ("has_zeros", got[-1, -2], ref["has_zeros"])
  assert not np.any(bits32(got[r:d - 1, -2])), "structural zeros of the inverted column"
  for name, g, w in (("inverted", got[:r, -2].astype(F64), ref["inverted64"]),
                     ("const", np.array([got[0, -1]], F64), np.array([ref["const64"]]))):
    zero = w == 0
    assert not np.any(bits32(g.astype(F32)[zero])), (name, "must be +0 where the reference is")
    assert np.all(np.abs(g - w)[~zero] <= 2 * ulp32(w[~zero])), \
        (name, float(np.max(np.abs(g - w)[~zero] / ulp32(w[~zero]))))
  keep = ref["keep"]
  assert not np.any(bits32(got[:, :r][:, ~keep])), ("a dropped column is not zero", np.flatnonzero(~keep))
  want = np.asarray(x, F64)[:, :r][:, keep] / ref["nrm"][keep][None, :]
  err = np.abs(got[:, :r][:, keep].astype(F64) - want)
  bound = (d / 2 + 3) * U * np.abs(want)
  assert np.all(err <= bound), ("kept sketch entries", float(np.max(err / np.maximum(bound, 1e-300))))


# (B, d, b, r): ragged 32-way / 16-way row slices at d = 100; r = 260 takes the second 256-column pass of the norms
FINISH_SHAPES = ((2, 128, 64, 8), (1, 100, 40, 7), (3, 256, 96, 64), (1, 520, 288, 260))
PREPARE_SHAPES = ((2, 128, 8), (1, 100, 7), (3, 256, 64), (1, 520, 260))
FINISH_DECAY = 0.999
THETA_KINDS = ("cutoff_pair", "below_noise")


def _packed_prev(rng, d, r, tail, zero_eigs=False, small_lead=False):
  """A valid packed sketch: orthonormal columns, graded deflated eigenvalues."""
  q = np.linalg.qr(rng.standard_normal((d, r)))[0]
  eigs = 2.0 * 0.9 ** np.arange(r) + 0.1
  if small_lead:
    eigs = eigs * 1e-8           # fwd[0] < error_tolerance = 1e-6
  if zero_eigs:
    eigs[r // 2:] = 0.0
  inv = np.where(eigs > 0, np.where(eigs > 0, eigs, 1.0) ** -0.25, 0.0)
  return pack(q, eigs, inv, tail ** -0.25 if tail > 0 else 0.0, tail, zero_eigs, F64).astype(F32)


@functools.lru_cache(maxsize=None)
def prepare_cases():
  """[(tag, prev [B, d, r + 2], r, ridge_epsilon, error_tolerance, relative)]: both modes; factor 0 of the variant
  'zeros' has zero eigenvalues, of 'small' a leading eigenvalue below error_tolerance."""
  cases = []
  for si, (bsz, d, r) in enumerate(PREPARE_SHAPES):
    for relative in (0, 1):
      for variant in ("zeros", "small"):
        rng = np.random.default_rng([7, si, relative, variant == "small"])
        prev = np.stack([_packed_prev(rng, d, r, 0.3, zero_eigs=(variant == "zeros" and j == 0),
                                      small_lead=(variant == "small" and j == 0)) for j in range(bsz)])
        cases.append((f"{bsz}x{d}r{r}-rel{relative}-{variant}", prev, r, 1e-6, 1e-6, relative))
  return cases


def _finish_theta(kind, d, b, r, rng):
  """theta [b] descending.  Both kinds have a gap after the leading third.
  cutoff_pair: theta[r - 1] == theta[r] > noise: the last pair's deflated value is exactly 0, rho > 0.
  below_noise: theta[r - 2] is 100 x under the noise floor, theta[r - 1] smaller, theta[r] negative: cutoff 0."""
  top = float(2.0 ** rng.integers(-3, 4) * rng.uniform(1.0, 2.0))
  lead = max(2, r // 3)
  th = np.empty(b)
  th[:lead] = top * np.linspace(1.0, 0.6, lead)
  th[lead:] = top * 0.05 * 0.98 ** np.arange(b - lead)        # the gap: 0.6 -> 0.05
  noise = float(F32(d * 1.2e-7)) * top
  if kind == "cutoff_pair":
    th[r - 1] = th[r]
  else:
    th[r - 2] = noise / 100.0
    th[r - 1] = noise / 400.0
    th[r:] = -top * np.linspace(0.001, 0.01, b - r)
  return th.astype(F32)


@functools.lru_cache(maxsize=None)
def finish_cases():
  """[(tag, theta [B, b], x [B, d, b], prev [B, d, r + 2], p, r, decay)].  x: orthonormal columns scaled per
  column, most within 1 +- 1e-4, columns 0 .. 3 at 0.98, 1.02 (unsafe), 0.992, 1.008 (safe).  Factor j of variant
  v has theta kind (v + j) mod 2 and a previous tail of 0.3 for even v + j // 2, else 0: with a zero tail the
  below_noise kind gives new_tail <= 0."""
  cases = []
  for si, (bsz, d, b, r) in enumerate(FINISH_SHAPES):
    for p in (2, 4):
      for v in (0, 1, 2, 3):
        rng = np.random.default_rng([11, si, p, v])
        th, xs, prevs = [], [], []
        for j in range(bsz):
          kind = THETA_KINDS[(v + j) % 2]
          th.append(_finish_theta(kind, d, b, r, rng))
          q = np.linalg.qr(rng.standard_normal((d, b)))[0]
          scale = 1.0 + 1e-4 * rng.uniform(-1, 1, b)
          scale[:4] = (0.98, 1.02, 0.992, 1.008)
          xs.append((q * scale).astype(F32))
          prevs.append(_packed_prev(rng, d, r, 0.3 if ((v + j) // 2) % 2 == 0 else 0.0))
        cases.append((f"{bsz}x{d}b{b}r{r}-p{p}-v{v}", np.stack(th), np.stack(xs), np.stack(prevs), p, r,
                      FINISH_DECAY))
  return cases


# =====================================================================================================
# D. whole update at the fused path's smallest shapes
# =====================================================================================================
UPDATE_SHAPES = ((256, 8, 3), (512, 64, 2))     # (d, rank, bsz): b = 64 and 96
UPDATE_KINDS = ("chained", "rank_deficient", "zero_zero", "pure_decay")
UPDATE_TOL = 1e-5                               # the iteration's residual tolerance (ps_fd_update_desc.tol)
UPDATE_P = 4
UPDATE_DECAY = 0.999
UPDATE_RIDGE = 1e-6


def update_ref(prev, gram, p, rank, decay=UPDATE_DECAY, ridge_epsilon=UPDATE_RIDGE, error_tolerance=1e-6,
               relative=True):
  """DS:1123-1290 by its definition in float64 for one factor: W = sketch sqrt(eigs + ridge),
  C = sym(decay W W^T + G), eigh, the leading rank + 1 pairs, deflation by the cutoff, masks, packing -- with
  the kernel's documented noise floor (eigenvalues at or below float32(d 1.2e-7) max(lambda_1, 0) are 0) applied to
  the exact eigenvalues.  Exact eigenvectors have unit norm, so the 1 % mask keeps every column with a positive
  deflated value.  Returns (packed [d, r + 2] float64, info: lam [r + 1], top, gap = the distance of the kept
  eigenvalues from the rest, noise, margin = how many times the leading eigenvalues are away from the floor)."""
  prev, gram = np.asarray(prev, F64), np.asarray(gram, F64)
  d, r = gram.shape[0], rank
  sketch, fwd, _, _, tail0, _ = unpack(prev, r)
  lead = fwd[0] if relative else 1.0
  ridge = float(F32(ridge_epsilon)) * max(lead, float(F32(error_tolerance)))
  w = sketch * np.sqrt(fwd + ridge)[None, :]
  c = float(F32(decay)) * (w @ w.T) + gram
  lam_all, vec = np.linalg.eigh(0.5 * (c + c.T))
  lam_all, vec = lam_all[::-1], vec[:, ::-1]
  lam = lam_all[:r + 1].copy()
  noise = float(F32(d * 1.2e-7)) * max(lam[0], 0.0)
  with np.errstate(all="ignore"):
    ratio = np.where(lam > noise, lam / max(noise, 1e-300), np.where(lam > 0, noise / lam, np.inf))
  margin = float(np.min(ratio)) if noise > 0 else np.inf
  lam = np.where(lam <= noise, 0.0, lam)
  s = np.sqrt(np.maximum(lam, 0.0))
  cutoff = s[r]
  tail = tail0 * float(F32(decay))
  new_tail = tail + cutoff * cutoff
  alpha = float(F32(-1.0 / p))
  const = 0.0 if new_tail <= 0 else new_tail ** alpha
  new_tail = max(new_tail, 0.0)
  defl = np.maximum((s[:r] - cutoff) * (s[:r] + cutoff), 0.0)
  keep = defl > 0
  up = np.where(keep, s[:r] ** 2 + tail, 0.0)
  inv = np.where(up > 0, np.where(up > 0, up, 1.0) ** alpha, 0.0)
  zeros = bool(new_tail <= 0) or bool(np.any(~keep))
  nk = int(keep.sum())
  below = lam_all[nk] if nk < d else 0.0
  gap = float(lam_all[nk - 1] - below) if nk else np.inf
  packed = pack(vec[:, :r] * keep[None, :], defl, inv, const, new_tail, zeros, F64)
  return packed, dict(lam=lam_all[:r + 1].copy(), top=float(max(lam_all[0], 0.0)), gap=gap, noise=noise,
                      margin=margin, keep=keep)


def update_errors(got, ref, rank, cols=None, tail_fields=True):
  """(scalar, projector): the largest error of the scalar fields (deflated, inverted, const, tail), each relative
  to the largest entry of its field in `ref`, and || P_got - P_ref ||_2 of the projectors on the kept columns.
  cols: the columns to compare (default: those `ref` keeps); tail_fields=False leaves const and tail out (the
  oracle has no noise floor: on a rank-deficient block its cutoff is a rounding-level positive number and its
  const = tail^(-1/p) noise, where update_ref and the kernels have exact zeros)."""
  r = rank
  g, w = unpack(np.asarray(got, F64), r), unpack(np.asarray(ref, F64), r)
  keep = (w[1] > 0) if cols is None else np.asarray(cols, bool)
  scalar = 0.0
  fields = [(g[1][keep], w[1][keep]), (g[2][keep], w[2][keep])]
  if tail_fields:
    fields += [(np.array([g[3]]), np.array([w[3]])), (np.array([g[4]]), np.array([w[4]]))]
  for a, b_ in fields:
    if b_.size and np.max(np.abs(b_)) > 0:
      scalar = max(scalar, float(np.max(np.abs(a - b_)) / np.max(np.abs(b_))))
    elif a.size:
      scalar = max(scalar, float(np.max(np.abs(a))))
  va, vb = g[0][:, keep], w[0][:, keep]
  proj = float(np.linalg.norm(va @ va.T - vb @ vb.T, 2)) if keep.any() else 0.0
  return scalar, proj


def check_update_exact(got, ref, rank):
  """Masks, zeros and flags exactly: the same columns kept, dropped columns and their deflated / inverted entries
  +0, the structural zeros, has_zeros; const and tail 0 where the reference's are; everything finite."""
  got = np.asarray(got, F32)
  r, d = rank, got.shape[0]
  assert np.all(np.isfinite(got)), "non-finite entries"
  g, w = unpack(got, r), unpack(ref, r)
  keep = w[1] > 0
  assert np.array_equal(g[1] > 0, keep), ("kept columns", np.flatnonzero(g[1] > 0), np.flatnonzero(keep))
  assert not np.any(bits32(got[:, :r][:, ~keep])), "a dropped sketch column is not zero"
  assert not np.any(bits32(g[1][~keep])) and not np.any(bits32(g[2][~keep])), "dropped deflated / inverted entries"
  assert np.all(g[2][keep] > 0)
  assert float(g[5]) == float(w[5]), ("has_zeros", float(g[5]), float(w[5]))
  for name, a, b_ in (("const", g[3], w[3]), ("tail", g[4], w[4])):
    assert (float(a) == 0.0) == (float(b_) == 0.0), (name, float(a), float(b_))
  assert not np.any(bits32(got[r:d - 1, -2])) and not np.any(bits32(got[2:d - r, -1])), "structural zeros"


def update_bound(oracle_err, info):
  """The larger of 4 x the float32-LAPACK oracle's own error against update_ref and tol * top / gap: the
  eigenvector (sin theta) bound of a residual converged to tol * top."""
  second = UPDATE_TOL * info["top"] / info["gap"] if info["gap"] > 0 and np.isfinite(info["gap"]) else 0.0
  return max(4.0 * oracle_err, second)


def _update_spectrum(d, r):
  """The leading r + 1 graded from 1 to 0.2, the rest in [0.008, 0.02]: 100 x above the noise floor of d = 512."""
  lam = np.empty(d)
  lam[:r + 1] = np.geomspace(1.0, 0.2, r + 1)
  lam[r + 1:] = np.linspace(0.02, 0.008, d - r - 1)
  return lam


@functools.lru_cache(maxsize=None)
def update_case(kind, d, rank, bsz):
  """dict(steps = [grams [bsz, d, d] float32, ...], prev0 [bsz, d, r + 2] float32, relative, x0 [bsz, d, b])."""
  rng = np.random.default_rng([23, UPDATE_KINDS.index(kind), d, rank])
  r = rank
  b = min(d, ((r + 1 + 31 + 31) // 32) * 32)
  zero_prev = np.zeros((bsz, d, r + 2), F32)
  x0 = rng.standard_normal((bsz, d, b)).astype(F32)

  def sym32(c):
    return (0.5 * (c + c.T)).astype(F32)
  if kind == "chained":
    steps = []
    for t in range(2):
      gs = []
      for _ in range(bsz):
        q = np.linalg.qr(rng.standard_normal((d, d)))[0]
        gs.append(sym32((1.0 + 0.3 * t) * (q * _update_spectrum(d, r)) @ q.T))
      steps.append(np.stack(gs))
    return dict(steps=steps, prev0=zero_prev, relative=False, x0=x0)
  if kind == "rank_deficient":
    q_rank = r - 3
    gs = []
    for _ in range(bsz):
      q = np.linalg.qr(rng.standard_normal((d, q_rank)))[0]
      gs.append(sym32((q * np.geomspace(1.0, 0.2, q_rank)) @ q.T))
    return dict(steps=[np.stack(gs)], prev0=zero_prev, relative=True, x0=x0, q=q_rank)
  zero_g = np.zeros((bsz, d, d), F32)
  if kind == "zero_zero":
    return dict(steps=[zero_g], prev0=zero_prev, relative=True, x0=x0)
  prev = np.stack([_packed_prev(rng, d, r, 0.3) for _ in range(bsz)])
  return dict(steps=[zero_g], prev0=prev, relative=True, x0=x0)


def gram_factor(gram):
  """A float32 factor R with R R^T = gram (what the oracle's fd_update_root takes)."""
  w, v = np.linalg.eigh(np.asarray(gram, F64))
  return (v * np.sqrt(np.maximum(w, 0.0))).astype(F32)


# Worst error of the float32-LAPACK oracle (oracle.shampoo_oracle.fd_update_root, sgesdd) against update_ref on the
# cases above, (scalar, projector) as update_errors measures them, on the columns update_ref keeps; measured on the
# CPU, re-measured by test_fd_round_references.py and held within [1/4, 3/2] of these figures.  The GPU gets the
# larger of 4 x the figure and tol * top / gap (update_bound); with tol = 1e-5 and the gaps of these cases
# (0.005 .. 0.2 of top) the second term is 5e-5 .. 2e-3 and decides.
UPDATE_ORACLE_SCALAR = 1.5e-6
UPDATE_ORACLE_PROJECTOR = 1.2e-5
