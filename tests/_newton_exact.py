"""Helpers shared by test_newton_exact_references.py (CPU) and test_gpu_newton_exact.py (GPU): two
input families on which the output of the coupled-Newton inverse p-th root (csrc/newton.hip) is
known PER ELEMENT, independent of tile shape, K-loop variant, summation order and execution.

Family 1 -- diagonal blocks, bit for bit.  Every product of the iteration has at most one
non-zero term per output element, which a float32 multiply-accumulate chain returns as fl(a * b)
(zeros add exactly), and (X + X^T) / 2 is exact on a diagonal matrix.  The whole root is then a
scalar float32 recursion per diagonal element (`diag_root_emulate`) plus shared scalars:
  * relative_matrix_epsilon = False: no power iteration, ridge = ridge_epsilon;
  * sumsq = sum (d_i + ridge)^2 is exact in any summation order when every square is a multiple of
    one power of two q and the total stays below 2^24 q (`exact_sumsq` asserts it);
  * z = fl((1 + p) / fl(2 sqrt(sumsq))) is then reproducible (correctly rounded operations);
  * h0 = powf(z, 1/p) is the one value the host cannot promise to round like the device: the
    emulator takes a shift in float32 neighbours (`H0_SHIFTS`), and a run is accepted if ONE
    candidate reproduces EVERY element (p = 1: only h0 = z).

Family 2 -- dense integer blocks A = 64 I + E, |E| <= 1, ridge_epsilon = 0, num_iters = k in
{1, 2, 3}.  sumsq is an exact integer below 2^24, so z, M0 = fl(A z), Mi0 and H1 = fl(h0 Mi0) are
reproduced in float32 exactly (`dense_init`; k = 1 is bit for bit).  For k >= 2 `dense_bound`
carries a float64 reference and an elementwise bound through the step graph of newton.hip.  For a
product C = A B of computed operands with reference values A64, B64 and bounds EA, EB

    EC = EA |B64| + |A64| EB + EA EB + (K + 2) u (|A64| + EA)(|B64| + EB),  u = 2^-24, K = npad,

valid for any summation order (gamma_K <= (K + 2) u for K <= 2^12).  The elementwise
Mi = fl(fl(oma I) + fl(alpha M)) adds |alpha| EM + 3 u (|oma| I + |alpha| (|M64| + EM)).  On the
symmetric path element (j, i) is a copy of the computed (i, j), or (diagonal tiles, averaged M
update) the rounded mean of the two: E <- max(E, E^T) + |C64 - C64^T| + 2 u (|C64| + E).

Nothing here imports the package's host code; `chain_products` restates build_chain of newton.hip
(= the multiplication order of the reference's mat_power).
"""
import numpy as np

from tests._exact import EXACT_LIMIT, U

F32 = np.float32
TILE = 128
H0_SHIFTS = (0, -1, 1)       # host powf, then its lower and upper float32 neighbour
MAX_ERROR_RATIO = F32(1.2)


def npad_of(n):
  return (int(n) + TILE - 1) // TILE * TILE


def shift_f32(x, k):
  """x moved by k float32 neighbours."""
  x = F32(x)
  for _ in range(abs(int(k))):
    x = np.nextafter(x, F32(np.inf) if k > 0 else F32(-np.inf), dtype=F32)
  return x


def pth_root_candidate(z, p, shift):
  """h0 = z^(1/p) as the host's float32 powf gives it, moved by `shift` neighbours."""
  if p == 1 and shift != 0:
    raise ValueError("p = 1: z^(1/1) = z is exact, no other candidate")
  return shift_f32(np.power(F32(z), F32(1.0 / p)), shift)


def h0_shifts(p):
  return (0,) if p == 1 else H0_SHIFTS


def exact_sumsq(values):
  """sum of squares of the float32 values, asserted exact in float32 in ANY summation order:
  every square is an integer multiple of one power of two q and the total is below 2^24 q, so
  every partial sum is such a multiple too and representable."""
  v = np.asarray(values, F32).astype(np.float64).ravel()
  sq = v * v                                   # exact: 48 bits
  nz = sq[sq != 0.0]
  if nz.size == 0:
    return F32(0.0)
  mant, exp = np.frexp(nz)
  m = (mant * 2.0 ** 53).astype(np.int64)      # 53-bit integer mantissa
  lowbit = exp.astype(np.int64) - 53 + np.round(np.log2((m & -m).astype(np.float64))).astype(np.int64)
  q = 2.0 ** int(lowbit.min())                 # the finest grid any square needs
  units = sq / q
  assert np.all(units == np.round(units))
  total = float(units.sum())
  assert total < EXACT_LIMIT, f"sum of squares is not exact in float32: {total} units of {q}"
  return F32(total * q)


def scale_of(values, p):
  """z of DS:870 for the damped values (all of them: a vector for a diagonal block, the matrix
  for a dense one)."""
  sumsq = exact_sumsq(values)
  with np.errstate(all="ignore"):
    return F32(F32(1 + p) / F32(F32(2) * np.sqrt(sumsq, dtype=F32)))


def chain_products(p):
  """Products of the binary-powering chain of one step, in order: (left, right, result) names;
  'mi' is the step's Mi, 't<k>' temporaries.  Returns (products, name of Mi^p)."""
  chain, nt = [], 0
  mat, power, i = "mi", None, int(p)
  while i > 0:
    if i & 1:
      if power is None:
        power = mat
      else:
        t = f"t{nt}"; nt += 1
        chain.append((mat, power, t)); power = t
    i >>= 1
    if i > 0:
      t = f"t{nt}"; nt += 1
      chain.append((mat, mat, t)); mat = t
  return chain, power


def _nanmax(x):
  """max |x| the way the kernel reduces it (unsigned maximum of the bit patterns): a NaN wins."""
  return F32(np.max(x)) if x.size else F32(0.0)


# ---------------------------------------------------------------------------
# Family 1: the scalar recursion of a diagonal block
# ---------------------------------------------------------------------------
def diag_root_emulate(d, p, ridge_epsilon, shift=0, num_iters=100, tol=1e-6):
  """The coupled Newton root of diag(d) in float32, element by element (DS:858-885 with
  relative_matrix_epsilon = False).  Returns (diagonal of the root, metrics dict with the PS_M_*
  names error / iters / ratio / retries / total_iters).  `shift` moves h0 of EVERY try."""
  d = np.asarray(d, F32)
  p = int(p)
  alpha = F32(-1.0 / p)
  oma = F32(1) - alpha
  ridge = F32(ridge_epsilon)      # * max(max_ev = 1, 1e-25)
  tol = F32(tol)
  chain, power_name = chain_products(p)
  tries, total = 0, 0
  failed = True
  with np.errstate(all="ignore"):
    while failed and tries < 6:
      rt = F32(ridge * F32(10.0 ** tries))
      damped = d + rt
      z = scale_of(damped, p)
      h0 = pth_root_candidate(z, p, shift)
      m = damped * z
      err = _nanmax(np.abs(m - F32(1)))
      h = np.full_like(d, h0)
      old_h = h
      it, ratio = 0, F32(1.0)
      while it < num_iters and err > tol and ratio < MAX_ERROR_RATIO:
        mi = oma + alpha * m                  # fl(oma * 1) = oma; two roundings as in DS:844
        buf = {"mi": mi}
        for a, b, c in chain:
          buf[c] = buf[a] * buf[b]
        new_m = buf[power_name] * m
        new_h = h * mi
        new_err = _nanmax(np.abs(new_m - F32(1)))
        ratio = F32(new_err / err)
        it, m, old_h, h, err = it + 1, new_m, h, new_h, new_err
      total += it
      result = h if ratio < MAX_ERROR_RATIO else old_h
      tries += 1
      failed = bool(err > F32(0.05))
  return result.astype(F32), dict(error=F32(err), iters=it, ratio=F32(ratio), retries=tries,
                                  total_iters=total)


# spectra of Family 1: d_i in {1, 2, 3, 4} times one power of two, ridge_epsilon = 2^-4
DIAG_RIDGE = 2.0 ** -4


def diag_spectrum(n, kind, salt=0):
  """float32 diagonal of length n.
  'full'   : {1, 2, 3, 4} * 2^-(salt % 4), position dependent: needs the full iteration count
  'equal'  : every value 3 * 2^-(salt % 4)
  'spread' : {1..4} * 2^-6 with every 8th element {1..4}: a spread of 4 * 2^6, more than 10 steps
  'retry'  : 'full' at scale 1 with one entry -1/8: try 1 (ridge 2^-4) sees -1/16 and diverges,
             try 2 (ridge 10/16) converges."""
  i = np.arange(n, dtype=np.int64)
  base = ((5 * i + salt) % 4 + 1).astype(np.float64)
  if kind == "full":
    d = base * 2.0 ** -(salt % 4)
  elif kind == "equal":
    d = np.full(n, 3.0 * 2.0 ** -(salt % 4))
  elif kind == "spread":
    d = np.where(i % 8 == 3, base, base * 2.0 ** -6)
    d[0] = 2.0 ** -6                           # the smallest value is always there
    if n > 3:
      d[3] = 4.0
  elif kind == "retry":
    d = base.copy()
    d[(salt * 7 + n // 2) % n] = -0.125
  else:
    raise ValueError(kind)
  return d.astype(F32)


# ---------------------------------------------------------------------------
# Family 2: dense integer blocks, step-limited
# ---------------------------------------------------------------------------
def dense_case(n, seed, symmetric=True):
  """int64 A = 64 I + E with E in {-1, 0, 1} (symmetric or not), random and position dependent."""
  rng = np.random.default_rng(seed)
  e = rng.integers(-1, 2, size=(n, n), dtype=np.int64)
  if symmetric:
    e = np.triu(e) + np.triu(e, 1).T
  return 64 * np.eye(n, dtype=np.int64) + e


def dense_init(a, p, shift=0):
  """float32 state after the initialisation of a try with ridge 0 (DS:866-875), exact on the
  host: dict z, h0, alpha, oma, M0, Mi0, H1 (= fl(h0 Mi0), the first H update)."""
  a32 = np.asarray(a, F32)
  n = a32.shape[0]
  assert np.array_equal(a32.astype(np.int64), np.asarray(a, np.int64))
  z = scale_of(a32, p)
  h0 = pth_root_candidate(z, p, shift)
  alpha = F32(-1.0 / p)
  oma = F32(1) - alpha
  eye = np.eye(n, dtype=F32)
  m0 = a32 * z
  mi0 = oma * eye + alpha * m0
  return dict(z=z, h0=h0, alpha=alpha, oma=oma, M0=m0, Mi0=mi0, H1=h0 * mi0, n=n, p=int(p))


def dense_steps_f32(init, k, matmul=None):
  """([H_1 .. H_k], [err_1 .. err_k]) of the step-limited run in float32 NumPy (full products,
  the reference's order); err_j = max |M_j - I| is what the loop control sees after step j.
  matmul(a, b, tag): the product; tag = (step, name) with name 'h', 'm' or the chain result --
  the hook the fault injections of the CPU test use."""
  if matmul is None:
    matmul = lambda a, b, tag: np.matmul(a, b)
  p, n = init["p"], init["n"]
  chain, power_name = chain_products(p)
  eye = np.eye(n, dtype=F32)
  m, mi, h = init["M0"], init["Mi0"], init["H1"]
  hs, errs = [], []
  for s in range(k):
    if s > 0:
      h = matmul(h, mi, (s, "h"))                           # H_{s+1} = H_s Mi_s
    buf = {"mi": mi}
    for a, b, c in chain:
      buf[c] = matmul(buf[a], buf[b], (s, c))
    m = matmul(buf[power_name], m, (s, "m"))                # M_{s+1}
    mi = init["oma"] * eye + init["alpha"] * m              # Mi_{s+1}
    hs.append(h)
    errs.append(F32(np.max(np.abs(m - eye))))
  return hs, errs


def _product64(a, b, kdepth, symmetric):
  (a64, ea), (b64, eb) = a, b
  c64 = a64 @ b64
  aa, ab = np.abs(a64), np.abs(b64)
  ec = (kdepth + 2) * U * ((aa + ea) @ (ab + eb))
  if ea.any():
    ec += ea @ ab + ea @ eb
  if eb.any():
    ec += aa @ eb
  if symmetric:
    ec = np.maximum(ec, ec.T)
    ec = ec + np.abs(c64 - c64.T) + 2 * U * (np.abs(c64) + ec)
  return c64, ec


def dense_bound(init, k, symmetric):
  """[(H64_j, E_j) for j = 1 .. k]: float64 evaluation of the same steps from the exact float32
  initial state and the derived elementwise bound on |H_j - H64_j| (module docstring).
  symmetric: the mirrored / averaged path (a superset of the bound of the full products)."""
  p, n = init["p"], init["n"]
  kdepth = npad_of(n)
  chain, power_name = chain_products(p)
  eye = np.eye(n)
  alpha, oma = float(init["alpha"]), float(init["oma"])
  zero = np.zeros((n, n))
  m = (init["M0"].astype(np.float64), zero)
  mi = (init["Mi0"].astype(np.float64), zero)
  h = (init["H1"].astype(np.float64), zero)
  out = [h]
  for s in range(k - 1):
    buf = {"mi": mi}
    for a, b, c in chain:
      buf[c] = _product64(buf[a], buf[b], kdepth, symmetric)
    m = _product64(buf[power_name], m, kdepth, symmetric)
    m64, em = m
    mi = (oma * eye + alpha * m64,
          abs(alpha) * em + 3 * U * (abs(oma) * eye + abs(alpha) * (np.abs(m64) + em)))
    h = _product64(h, mi, kdepth, symmetric)
    out.append(h)
  return out


def worst_ratio(got, ref64, bound):
  """max |got - ref| / bound (0 where got == ref; inf where the bound is 0 and they differ)."""
  err = np.abs(np.asarray(got, np.float64) - ref64)
  with np.errstate(all="ignore"):
    r = np.where(err == 0.0, 0.0, err / bound)
  r = np.where(np.isnan(r), np.inf, r)
  return float(r.max()) if r.size else 0.0


# injected faults (CPU test): each returns a matmul hook for dense_steps_f32
def fault_transpose32(tag, r0, c0):
  def mm(a, b, t):
    c = np.matmul(a, b)
    if t == tag:
      c = c.copy()
      c[r0:r0 + 32, c0:c0 + 32] = c[r0:r0 + 32, c0:c0 + 32].T.copy()
    return c
  return mm


def fault_drop_slab(tag, k0):
  def mm(a, b, t):
    c = np.matmul(a, b)
    if t == tag:
      c = c - np.matmul(a[:, k0:k0 + 16], b[k0:k0 + 16, :])
    return c
  return mm


def fault_swap(tag):
  def mm(a, b, t):
    return np.matmul(b, a) if t == tag else np.matmul(a, b)
  return mm


def fault_transposed_operand(tag):
  def mm(a, b, t):
    return np.matmul(a, b.T) if t == tag else np.matmul(a, b)
  return mm


# ---------------------------------------------------------------------------
# integer exactness of mat_power (ps_mat_power_f32)
# ---------------------------------------------------------------------------
# (n, p, density of the non-zeros): n across the 128-tile edges; the density keeps max |A|^p < 2^24
MAT_POWER_CASES = [(1, 1, 1.0), (1, 4, 1.0), (2, 3, 1.0), (7, 4, 1.0), (127, 4, 1.0), (128, 2, 1.0),
                   (128, 4, 1.0), (129, 1, 1.0), (129, 3, 1.0), (129, 4, 1.0), (255, 4, 1.0),
                   (256, 3, 1.0), (257, 2, 1.0), (257, 4, 0.9), (300, 3, 1.0), (384, 4, 0.5),
                   (385, 4, 0.5)]


def mat_power_int_case(n, p, density):
  """(A int64 with entries in {-1, 0, 1}, A^p int64).  Asserts max |A|^q < 2^24 for every q <= p:
  every product of the powering chain and every partial sum in it is then an exactly
  representable integer, whatever the multiplication and summation order."""
  rng = np.random.default_rng(7000 + 10 * n + p)
  a = rng.choice(np.array([-1, 1], np.int64), size=(n, n))
  a = np.where(rng.random((n, n)) < density, a, 0)
  assert 1 <= p <= 4
  absa = np.abs(a).astype(np.float64)
  power_abs, power = absa, a.astype(np.float64)
  for _ in range(p - 1):
    power_abs = power_abs @ absa
    power = power @ a.astype(np.float64)        # exact below 2^53
    assert power_abs.max() < EXACT_LIMIT, (n, p, power_abs.max())
  return a, power.astype(np.int64)
