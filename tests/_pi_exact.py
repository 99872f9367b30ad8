"""Helpers shared by test_pi_exact_references.py (CPU) and test_gpu_pi_exact.py (GPU): a float64
reference of the batched power iteration (precondition_amd/csrc/power_iter.hip.h, reference loop DS:625-652),
worst-case float32 error bounds that hold for ANY summation order, and matrix families on which a
wrong mat-vec, a wrong lane, a transposed tile or a leak from the padding cannot hide.

What the kernels compute per step, from the float32 iterate v^ (|v^| = 1):

    y = fl(A v^)     s = fl(v^ . y)     nrm = fl(sqrt(fl(sum y_i^2)))     v^' = fl(y / nrm)

and before the first step v^ = fl(v0 / fl(||v0||)).  The loop ends after the step in which
|s - s_prev| <= tol or with step num_iters; lambda is that step's s and the vector its v^'.
`reference64` runs the same loop in float64 on the float32 matrix.

Bounds (u = 2^-24; gamma_n = n u / (1 - n u); nothing below is fitted to a measurement)
--------------------------------------------------------------------------------------
Sums.  A float32 sum of n terms in any order (sequential, tree, per tile then across tiles, with or
without fused multiply-adds) puts at most n roundings on a term's way to the total (its product and
at most n - 1 additions; adding an exact zero does not round): sum_j t_j (1 + e_j), |e_j| <= gamma_n.

Norm.  ss = fl(sum x_i^2) = ||x||^2 (1 + e), |e| <= gamma_n (all terms are positive), so
sqrt(ss) = ||x|| (1 + e'), |e'| <= n u / 2 + O((n u)^2).  Correct rounding of sqrtf and of the
division is NOT assumed: each may be off by C_DIV = 4 u (2 ulp).  With (n u)^2 / 8 < 0.1 u for
n <= 1024:            |nrm / ||x|| - 1| <= THETA(n) = (n / 2 + 5) u,
and an element of the normalised vector is x_i / ||x|| (1 + kappa)(1 + d_i) with ONE common factor
|kappa| <= THETA(n) and an own |d_i| <= D = 4 u.

One dense step (num_iters = 1, v0 exact).  v^_j = v_j (1 + kappa0)(1 + d_j) with v the float64 unit
vector.  y_i = sum_j a_ij v^_j (1 + e_ij), |e_ij| <= gamma_n.  With y~ = y / (1 + kappa0):
    |y~_i - y64_i| <= EY_i = (n + C_Y) u (|A||v|)_i,   C_Y = 5   (gamma_n + D + 1 u second order)
    |s - s64|      <= (3 n + C_S) u |v|^T |A| |v|,     C_S = 21
s carries v^ twice (2 THETA + 2 D = (n + 18) u), the mat-vec and the dot product (2 gamma_n), 2 u of
second-order terms ((3 n u)^2 / 2 < 0.3 u) and 1 u for the rounding of s - s_prev in the stop rule.
The output V = fl(y / fl(||y||)) does not see the common factor of y (it cancels in y / ||y||):
    |y~/||y~|| - y64/||y64|||_i <= T_i = (EY_i + |V64_i| ||EY||) / (||y64|| - ||EY||)
    |V_i - V64_i| <= T_i + 2 (THETA(n) + D + u) (|V64_i| + T_i)
The last term is "the (n / 2 + c) u of each norm": the output norm and division need it once; it
is counted twice, for the input norm too, although that factor cancels to first order -- an
over-estimate of at most (n / 2 + 10) u |V_i|, small beside T_i for dense matrices.

Probe matrices (at most one non-zero per row and per column, entries +-2^k): a_ij v^_j is exact
and nothing is added to it but zeros, so y = A v^ EXACTLY in float32, in the mirrored (column-sum)
path as well.  A relative error of v^_j moves to y_i unchanged.  Let e_k bound the element-wise
(non-common) relative error of the iterate after k steps and kappa_k its common factor:
e_0 = D, e_k = e_{k-1} + D (one more division); kappa_k <= e_{k-1} + THETA(n) (the true norm of
the perturbed y, then its float32 evaluation; the previous common factor cancels).  So
    |v^(k)_i - v64(k)_i| <= R_k |v64(k)_i|,   R_k = THETA(n) + (2 k + 1) D + u
    |s_k - s64_k| <= (2 R_{k-1} + (n + 3) u) sum_i |v64(k-1)_i| |y64(k)_i|
(n u for the dot product, 2 u second order, 1 u for the subtraction of the stop rule).  These are the
"compounded" bounds of the k-step tests: linear in k because only the divisions accumulate.

Stop rule.  If the float64 |ds| of every step is further than E_k + E_{k-1} <= 2 E from tol, float32
and float64 take the same decision in every step (`stop_margin_ok`); the CPU test gates every
stop-rule case of the GPU file on it.

Magnitudes: entries are within [2^-3, 4] or O(1), at most 100 steps are taken and the probes stop
within 8, so no product, square or quotient leaves the normal float32 range.

Nothing here imports the package's host code except `run_pi`, which calls the C entry point.
"""
import functools

import numpy as np

U = 2.0 ** -24
F32 = np.float32
TILE = 128
SENTINEL = -7.25          # finite, unmistakable: no normalised vector holds it
SENTINEL_IT = -7
PS_EINVAL = -1
D = 4.0 * U               # one division (or sqrt): 2 ulp, correct rounding not assumed
C_Y, C_S = 5.0, 21.0

SIZES = (1, 2, 5, 127, 128, 129, 255, 257, 300, 384, 511, 512, 513, 640, 700, 1024)
SHIFT_ODD = 67


def theta(n):
  return (0.5 * n + 5.0) * U


def tiles_of(n):
  return (int(n) + TILE - 1) // TILE


def v0_f32(n):
  """DS:642-643 (uniform(size=n) is a prefix of uniform(size=m > n))."""
  return np.random.RandomState(1729).uniform(-1.0, 1.0, int(n)).astype(F32)


# ---------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------
class Ref:
  """steps[k]: dict(s, ds, y, absAv, v) of step k + 1 (v: the unit vector the step started from);
  iters, lam (s of the last step), vec (normalised y of the last step)."""

  def __init__(self, steps, iters, lam, vec):
    self.steps, self.iters, self.lam, self.vec = steps, iters, lam, vec


def reference64(a, n_eff, num_iters, tol):
  """DS:625-652 in float64 on the leading [n_eff, n_eff] part of the float32 matrix `a`, v0 masked."""
  a = np.asarray(a)
  assert a.dtype == F32 and a.ndim == 2 and a.shape[0] == a.shape[1]
  n_eff = int(n_eff)
  if n_eff == 0:   # v0 masked to zero: 0 / 0, NaN > tol is false, one step
    return Ref([], 1, np.nan, np.zeros(0))
  A = a[:n_eff, :n_eff].astype(np.float64)
  absA = np.abs(A)
  v = v0_f32(a.shape[0])[:n_eff].astype(np.float64)
  s, steps = 0.0, []
  for _ in range(int(num_iters)):
    vh = v / np.linalg.norm(v)
    y = A @ vh
    s_new = float(vh @ y)
    ds = abs(s_new - s)
    steps.append(dict(s=s_new, ds=ds, y=y, absAv=absA @ np.abs(vh), v=vh))
    s, v = s_new, y
    if not ds > tol:
      break
  return Ref(steps, len(steps), s, v / np.linalg.norm(v))


# ---------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------
def dense_bounds(ref):
  """(bound on s, componentwise bound on V) of a ONE-step run on any matrix."""
  st = ref.steps[0]
  n = st["y"].shape[0]
  es = (3.0 * n + C_S) * U * float(np.abs(st["v"]) @ st["absAv"])
  ey = (n + C_Y) * U * st["absAv"]
  ny, ne = np.linalg.norm(st["y"]), np.linalg.norm(ey)
  t = (ey + np.abs(ref.vec) * ne) / (ny - ne)
  return es, t + 2.0 * (theta(n) + D + U) * (np.abs(ref.vec) + t)


def probe_vec_rel(n, k):
  return theta(n) + (2 * k + 1) * D + U


def probe_s_bounds(ref):
  """Per-step bounds on s for a matrix whose float32 mat-vec is exact."""
  n = ref.steps[0]["y"].shape[0]
  return np.array([(2.0 * probe_vec_rel(n, k) + (n + 3.0) * U) * float(np.abs(st["v"]) @ np.abs(st["y"]))
                   for k, st in enumerate(ref.steps)])


def probe_bounds(ref):
  """(bound on s of the last step, componentwise bound on V) after ref.iters steps of a probe."""
  n = ref.steps[0]["y"].shape[0]
  return probe_s_bounds(ref)[-1], probe_vec_rel(n, ref.iters) * np.abs(ref.vec)


def stop_margin_ok(steps, tol, E):
  """True when every step's float64 |ds| lies outside [tol - 2 E, tol + 2 E] (E: one bound on s, or
  one per step -- a step then uses the larger of its own and its predecessor's)."""
  E = np.broadcast_to(np.asarray(E, np.float64), (len(steps),))
  for k, st in enumerate(steps):
    e = max(E[k], E[k - 1] if k else 0.0)
    if tol - 2.0 * e <= st["ds"] <= tol + 2.0 * e:
      return False
  return True


def first_mismatch(got, want, bound):
  """(row, tile, |error|, bound) of the first component outside its bound, or None."""
  bad = np.flatnonzero(~(np.abs(got.astype(np.float64) - want) <= bound))
  if bad.size == 0:
    return None
  r = int(bad[0])
  return r, r // TILE, float(abs(float(got[r]) - want[r])), float(np.broadcast_to(bound, want.shape)[r])


def ratio(got, want, bound):
  """max |error| / bound over the components with a non-zero bound."""
  err = np.abs(np.asarray(got, np.float64) - want)
  b = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
  nz = b > 0
  return float((err[nz] / b[nz]).max()) if nz.any() else 0.0


# ---------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------
def _rng(*key):
  return np.random.default_rng([int(k) for k in key])


def dense_sym(n, seed=0):
  g = _rng(11, seed, n).uniform(-1.0, 1.0, (n, n)).astype(F32)
  return np.ascontiguousarray(np.triu(g) + np.triu(g, 1).T)


def dense_gen(n, seed=0):
  return _rng(12, seed, n).uniform(-1.0, 1.0, (n, n)).astype(F32)


def _pow2(rng, m):
  return (rng.choice([-1.0, 1.0], m) * 2.0 ** rng.integers(-3, 1, m)).astype(F32)


def probe_involution(n, seed=0, dominant=False):
  """Symmetric: random transpositions (i j) with a_ij = a_ji = +-2^k and about n / 8 fixed points
  a_ii = +-2^k.  dominant: the fixed point with the largest |v0| gets the entry 4."""
  rng = _rng(13, seed, n)
  nfix = max(1, n // 8)
  nfix += (n - nfix) % 2
  perm = rng.permutation(n)
  a = np.zeros((n, n), F32)
  fix, rest = perm[:nfix], perm[nfix:]
  a[fix, fix] = _pow2(rng, nfix)
  i, j = rest[0::2], rest[1::2]
  w = _pow2(rng, i.size)
  a[i, j] = w
  a[j, i] = w
  if dominant:
    p = fix[np.argmax(np.abs(v0_f32(n)[fix]))]
    a[p, p] = 4.0
  return a


def probe_shift(n, d, seed=0, dominant=False):
  """a[i, (i + d) % n] = +-2^k: not symmetric, every row reaches into another tile.  dominant: the
  index p with the largest |v0| becomes a fixed point with the entry 4 (its row and the other entry
  of its column are cleared, which opens the cycle into a chain)."""
  rng = _rng(14, seed, n, d)
  a = np.zeros((n, n), F32)
  i = np.arange(n)
  a[i, (i + d) % n] = _pow2(rng, n)
  if dominant:
    p = int(np.argmax(np.abs(v0_f32(n))))
    a[p, :] = 0.0
    a[:, p] = 0.0
    a[p, p] = 4.0
  return a


def single_defect(n, i, j, seed=0):
  """dense_sym with ONE element made non-symmetric: a_ij = 64 max|A|, a_ji unchanged."""
  a = dense_sym(n, seed).copy()
  a[i, j] = F32(64.0) * np.abs(a).max()
  return a


def symmetric_reading(a):
  """What an execution that wrongly takes `a` for symmetric computes with: the upper triangle mirrored."""
  return np.ascontiguousarray(np.triu(a) + np.triu(a, 1).T)


@functools.lru_cache(maxsize=None)
def matrix(kind, n):
  """The named test matrices (read-only, shared between the tests)."""
  a = {"sym": dense_sym, "gen": dense_gen, "inv": probe_involution,
       "shift_odd": lambda m: probe_shift(m, SHIFT_ODD), "shift129": lambda m: probe_shift(m, 129)}[kind](n)
  a.setflags(write=False)
  return a


def is_probe(kind):
  return kind.startswith(("inv", "shift"))


@functools.lru_cache(maxsize=None)
def one_step_ref(kind, n, pad=None):
  return reference64(matrix(kind, n), n if pad is None else pad, 1, 0.0)


def one_step_bounds(kind, ref):
  return probe_bounds(ref) if is_probe(kind) else dense_bounds(ref)


# ---------------------------------------------------------------------------
# case lists of the GPU file (gated by the CPU file)
# ---------------------------------------------------------------------------
# a. two mixed-size batches, symmetric and general alternating; every size gets both kinds
DENSE_BATCHES = tuple(tuple((("sym", "gen")[(i + flip) % 2], n) for i, n in enumerate(SIZES))
                      for flip in (0, 1))
SHUFFLE = tuple(int(i) for i in np.random.RandomState(7).permutation(len(SIZES)))
# b. probes, one step
PROBE_BATCHES = (tuple(("inv", n) for n in SIZES), tuple(("shift_odd", n) for n in SIZES),
                 tuple(("shift129", n) for n in SIZES if n > 129))
# c. (n, i, j, where) of the single defect; positions exist only where the structure does
def defect_positions(n):
  pos = [(3, 70, "diagonal tile"), (1, n - 1, "ragged edge sub-block"), (n - 1, 0, "last row")]
  if n >= 2 * TILE - 64:   # a whole 64 x 64 sub-block of an off-diagonal tile
    pos.insert(1, (150, 10, "interior off-diagonal sub-block"))
  return pos
DEFECT_SIZES = (129, 300, 513)
DEFECT_CASES = tuple((n, i, j, w) for n in DEFECT_SIZES for i, j, w in defect_positions(n))
DEFECT_BEHIND_PADDING = (300, 200, 250, 10)   # n, padding_start, i, j
# d. (kind, n, padding_start): the issue's padding_start values at n = 300 and at the tile edges of
# other sizes, t = 7 (1024 cut to 770), the all-padding block
PAD_CASES = (("sym", 300, 1), ("gen", 300, 64), ("sym", 300, 128), ("gen", 300, 129),
             ("sym", 300, 299), ("gen", 300, 300), ("sym", 300, 0), ("gen", 129, 128),
             ("sym", 129, 129), ("gen", 513, 512), ("sym", 513, 513), ("gen", 700, 129),
             ("sym", 1024, 770), ("gen", 1024, 1023), ("sym", 640, 64), ("gen", 5, 4))
# e. (kind, n, padding_start) of the out_v batch, read with ldv = n_max + 5
OUT_V_CASES = (("gen", 5, 3), ("sym", 300, 300), ("gen", 129, 100), ("sym", 513, 513), ("sym", 300, 128))
# name -> (lda(n), offset of the view in its NaN-filled parent, floats)
LAYOUTS = {"lda_n_plus_3": (lambda n: n + 3, 0),
           "misaligned_base": (lambda n: (n + 3) // 4 * 4 + 4, 1)}


def vec_ok(offset, lda):
  """PiPlan::upload's rule, for a parent allocation that is 16-byte aligned."""
  return (4 * offset) % 16 == 0 and lda % 4 == 0


# f. (batch of (kind, n), tol): dominant fixed point, the loop stops by itself
# tol = 2^-7: below the first step's |s| of most seeds even at n = 1024 (2^-5 ends many runs at
# step 1), and more than 2 E (1e-3 at n = 1024) above zero
STOP_BATCHES = ((tuple(("inv", n) for n in SIZES), 2.0 ** -7),
                (tuple(("shift_odd", n) for n in SIZES), 2.0 ** -7),
                (tuple(("shift129", n) for n in SIZES if n > 129), 2.0 ** -7))
# a cyclic shift has n eigenvalues of one modulus: s keeps moving.  (kind, n), tol, num_iters
NEVER_BATCH = ((("shift_odd", 127), ("shift_odd", 129), ("shift129", 300), ("shift129", 513)), 2.0 ** -12, 7)
# g. n of the block that holds one NaN, and its position
NAN_CASES = ((129, 100, 128), (300, 131, 7))


@functools.lru_cache(maxsize=None)
def stop_case(kind, n, tol):
  """(matrix, float64 run with num_iters = 100) of the dominant-fixed-point probe `kind`: the first
  seed whose float64 run keeps clear of tol in every step (`stop_margin_ok`) and, for n >= 5, takes
  4 to 8 steps.  Chosen from the float64 reference alone.  The margin holds by this construction
  (no seed: an error, never a skip); what the CPU file then adds independently is that the float32
  oracle takes the float64 step counts on every case."""
  d = {"shift_odd": SHIFT_ODD, "shift129": 129}.get(kind)
  for seed in range(64):
    a = probe_involution(n, seed, True) if kind == "inv" else probe_shift(n, d, seed, True)
    ref = reference64(a, n, 100, tol)
    if stop_margin_ok(ref.steps, tol, probe_s_bounds(ref)) and (n < 5 or 4 <= ref.iters <= 8):
      a.setflags(write=False)
      return a, ref
  raise AssertionError(f"no seed gives a clear stop decision for {kind} n={n} tol={tol}")


def truncated(ref, m):
  """The run with num_iters = m <= ref.iters: the forced last step."""
  assert 1 <= m <= ref.iters
  if m == ref.iters:
    return ref
  y = ref.steps[m - 1]["y"]
  return Ref(ref.steps[:m], m, ref.steps[m - 1]["s"], y / np.linalg.norm(y))


def padded(kind, n, pad):
  """matrix(kind, n) with NaN in every row and column >= pad."""
  a = matrix(kind, n).copy()
  a[pad:, :] = np.nan
  a[:, pad:] = np.nan
  return a


# ---------------------------------------------------------------------------
# the call
# ---------------------------------------------------------------------------
def ld_of(t):
  """Leading dimension of a row-major 2-D view, as kernels._as_2d_ld derives it."""
  assert t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1)
  return int(t.stride(0)) if t.shape[0] > 1 else max(int(t.shape[1]), 1)


def run_pi(mats, pads=None, num_iters=100, tol=1e-6, symmetry="verify", options=None, ldv=None,
           expect_rc=0):
  """ps_power_iteration_batched_opt_f32 on device tensors / views.  Returns (lam [batch], iters
  [batch], V [batch, ldv]) as NumPy arrays; every output starts as a sentinel."""
  import ctypes as C
  import torch
  from precondition_amd import _lib
  L = _lib.lib()
  batch, dev = len(mats), mats[0].device
  i32 = lambda xs: np.ascontiguousarray(np.asarray(xs, dtype=np.int32))
  n = i32([m.shape[0] for m in mats])
  lda = i32([ld_of(m) for m in mats])
  pad = None if pads is None else i32(list(pads))
  if ldv is None:
    ldv = int(n.max())
  lam = torch.full((batch,), SENTINEL, dtype=torch.float32, device=dev)
  its = torch.full((batch,), SENTINEL_IT, dtype=torch.int32, device=dev)
  V = torch.full((batch, max(int(ldv), 1)), SENTINEL, dtype=torch.float32, device=dev)
  ws = torch.empty(max(int(L.ps_power_iteration_workspace_bytes(batch, n.ctypes.data)), 256),
                   dtype=torch.uint8, device=dev)
  ptrs = np.ascontiguousarray(np.asarray([m.data_ptr() for m in mats], dtype=np.uint64))
  popt, _keep = _lib.make_options(options)
  with torch.cuda.device(dev):
    rc = L.ps_power_iteration_batched_opt_f32(
        torch.cuda.current_stream().cuda_stream, ptrs.ctypes.data, n.ctypes.data, lda.ctypes.data,
        None if pad is None else pad.ctypes.data, batch, int(num_iters), float(tol), lam.data_ptr(),
        its.data_ptr(), V.data_ptr(), int(ldv), _lib.symmetry_code(symmetry), ws.data_ptr(),
        ws.numel(), C.byref(popt))
    torch.cuda.synchronize()
  assert rc == expect_rc, f"ps_power_iteration_batched_opt_f32 returned {rc}, expected {expect_rc}"
  return lam.cpu().numpy(), its.cpu().numpy(), V.cpu().numpy()
