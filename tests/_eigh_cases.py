"""Inputs, metrics and yardsticks of the eigensolver edge tests.  Pure NumPy: nothing here imports the
library, so the same list feeds the CPU self-check (test_eigh_cases_references.py) and the GPU tests
(test_gpu_eigh_solvers.py).

A family is a function (n, rng) -> float64 symmetric matrix; `case()` rounds it to float32, the matrix
every solver is handed.  The float64 eigendecomposition of that float32 matrix is the truth, LAPACK's
float32 ``ssyevd`` (oracle.lapack32.eigh32) on the same matrix is the yardstick, and a solver passes a
metric when it stays below ``bound(metric, yardstick_value, floor)`` = max(4 x yardstick, floor).  The
floors are the bounds the suite already asserts for the same solver and quantity
(test_eigh_batched_matches_lapack for n <= 128, test_eigh_tridiagonal_path_structured_inputs above).
"""
import zlib

import numpy as np

F32 = np.float32

SMALL_SIZES = (1, 2, 3, 17, 63, 64, 65, 95, 96, 97, 127, 128)   # eigh_small_kernel (n <= 128)
BIG_SIZES = (129, 192, 257)                                     # blocked Jacobi solvers
SMALL_ROOT_SIZES = (1, 2, 64, 65, 97, 128)
ROOT_PS = (1, 2, 4, 8)

#          eig_err, resid, orth
FLOORS_SMALL = {"eig_err": 2e-6, "resid": 2e-5, "orth": 2e-5}
FLOORS_BIG = {"eig_err": 3e-6, "resid": 3e-6, "orth": 5e-6}
YARDSTICK_FACTOR = 4.0


def floors_for(n):
  return FLOORS_SMALL if n <= 128 else FLOORS_BIG


def bound(metric, yardstick_value, floor):
  """The one bound rule: four times float32 LAPACK's own value on the same input, never below the
  floor the project already asserts for this solver and quantity."""
  del metric
  return max(YARDSTICK_FACTOR * float(yardstick_value), float(floor))


# ---------------------------------------------------------------------------------------------
# families
def _sym(g):
  return (g + g.T) / 2


def _wishart(n, k, rng):
  g = rng.standard_normal((n, k))
  return g @ g.T


def _f32_exact(a):
  """The float32 rounding of `a`, as float64: a power-of-two multiple of it rounds without error."""
  return _sym(a).astype(F32).astype(np.float64)


def _orth(n, rng):
  q, _ = np.linalg.qr(rng.standard_normal((n, n)))
  return q


def _reps(n):
  return np.repeat([1.0, 2.0, 3.0, 5.0], (n + 3) // 4)[:n]


def identity(n, rng):
  return np.eye(n)


def zero(n, rng):
  return np.zeros((n, n))


def diag_descending(n, rng):
  return np.diag(np.arange(n, 0, -1).astype(np.float64))


def diag_repeats(n, rng):
  return np.diag(_reps(n))


def rotated_repeats(n, rng):
  q = _orth(n, rng)
  return (q * _reps(n)) @ q.T


def two_i_plus_noise(n, rng):
  return 2 * np.eye(n) + 1e-6 * _sym(rng.standard_normal((n, n)))


def rank1(n, rng):
  x = rng.standard_normal((n, 1))
  return x @ x.T


def rank1_plus_i(n, rng):
  return rank1(n, rng) + np.eye(n)


def ones(n, rng):
  return np.ones((n, n))


def wilkinson(n, rng):
  return (np.diag(np.abs(np.arange(n) - n // 2).astype(np.float64)) + np.diag(np.ones(n - 1), 1) +
          np.diag(np.ones(n - 1), -1))


def psd_rank_deficient(n, rng):
  return _wishart(n, max(1, n // 4), rng)


def goe_indefinite(n, rng):
  return _sym(rng.standard_normal((n, n)))


def negative_definite(n, rng):
  return -_wishart(n, 2 * n, rng)


def exchange(n, rng):
  return np.eye(n)[::-1].copy()


def householder_uniform(n, rng):
  a = np.full((n, n), -2.0 / n)    # I - 2 u u^T with u = 1 / sqrt(n): constant diagonal 1 - 2 / n
  np.fill_diagonal(a, 1.0 - 2.0 / n)
  return a


def householder_random(n, rng):
  u = rng.standard_normal((n, 1))
  u /= np.linalg.norm(u)
  return np.eye(n) - 2 * (u @ u.T)


def bipartite_random(n, rng):
  h = n // 2
  b = rng.standard_normal((h, n - h))
  a = np.zeros((n, n))
  a[:h, h:] = b
  a[h:, :h] = b.T
  return a


def path_graph(n, rng):
  return np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1)


def symmetric_hadamard(n, rng):
  h = np.ones((1, 1))
  while h.shape[0] < n:
    h = np.block([[h, h], [h, -h]])
  return h


def wishart(n, rng):
  return _wishart(n, 3 * n, rng)


def wishart_x2p34(n, rng):
  return _f32_exact(wishart(n, rng)) * 2.0 ** 34


def wishart_x2m50(n, rng):
  return _f32_exact(wishart(n, rng)) * 2.0 ** -50


def goe_x2p34(n, rng):
  return _f32_exact(goe_indefinite(n, rng)) * 2.0 ** 34


def graded_1e8(n, rng):
  w = _wishart(n, 4 * n, rng) / (4 * n)
  d = np.logspace(0, -4, n)
  return d[:, None] * w * d[None, :]


def nan_entry(n, rng):
  a = _sym(rng.standard_normal((n, n)))
  i, j = n // 3, (2 * n) // 3
  a[i, j] = a[j, i] = np.nan
  return a


def inf_diagonal(n, rng):
  a = _wishart(n, 2 * n, rng)
  a[n // 2, n // 2] = np.inf
  return a


PLAIN = {"identity": identity, "zero": zero, "diag_descending": diag_descending, "diag_repeats": diag_repeats,
         "rotated_repeats": rotated_repeats, "two_I_plus_1e-6_noise": two_i_plus_noise, "rank1": rank1,
         "rank1_plus_I": rank1_plus_i, "ones": ones, "wilkinson": wilkinson,
         "psd_rank_deficient": psd_rank_deficient, "goe_indefinite": goe_indefinite,
         "negative_definite": negative_definite}
PM_MIXING = {"exchange": exchange, "householder_uniform": householder_uniform,
             "householder_random": householder_random, "bipartite_random": bipartite_random,
             "path_graph": path_graph, "symmetric_hadamard": symmetric_hadamard}
SCALE = {"wishart_x2^34": wishart_x2p34, "wishart_x2^-50": wishart_x2m50, "goe_x2^34": goe_x2p34}
GRADED = {"graded_1e8": graded_1e8}
NON_FINITE = {"nan_entry": nan_entry, "inf_diagonal": inf_diagonal}
UNSCALED = {"wishart_x2^34": (wishart, 34), "wishart_x2^-50": (wishart, -50), "goe_x2^34": (goe_indefinite, 34)}

FINITE = {**PLAIN, **PM_MIXING, **SCALE, **GRADED}
ALL = {**FINITE, **NON_FINITE}
POSITIVE_DEFINITE = ("identity", "diag_descending", "diag_repeats", "rotated_repeats", "two_I_plus_1e-6_noise",
                     "rank1_plus_I", "graded_1e8")

ROOT_FAMILIES_SMALL = ("psd_rank_deficient", "rank1", "zero", "identity", "graded_1e8", "wishart_x2^34",
                       "wishart_x2^-50")
ROOT_FAMILIES_ONE_SIDED = ("psd_rank_deficient", "rank1_plus_I", "graded_1e8", "two_I_plus_1e-6_noise",
                           "wishart_x2^34")


def defined(name, n):
  """The only family x size pairs that are left out: the ones that do not exist."""
  if name == "symmetric_hadamard":
    return n >= 2 and (n & (n - 1)) == 0   # Sylvester's construction; at n = 1 there is no -x
  if name == "bipartite_random":
    return n >= 2                          # both halves need a vertex
  return True


def names_for(n, families):
  return [k for k in families if defined(k, n)]


def _rng(name, n):
  return np.random.default_rng([zlib.crc32(name.encode()), n])


def case(name, n):
  """The float32 matrix of a family at size n (deterministic: the seed is the name and the size)."""
  a = ALL[name](n, _rng(name, n))
  with np.errstate(over="ignore", invalid="ignore"):
    return np.ascontiguousarray(a.astype(F32))


def unscaled_case(name, n):
  """(float32 matrix before the scaling, exponent) of a scale family: case(name, n) == matrix * 2^exponent."""
  fam, ex = UNSCALED[name]
  return _sym(fam(n, _rng(name, n))).astype(F32), ex


def singular_psd(n):
  """Exactly singular positive semi-definite float32 input: small-integer factors, so the Gram matrix is
  exact in float32 and its rank is exactly n // 2."""
  g = _rng("singular_psd", n).integers(-2, 3, size=(n, n // 2)).astype(np.float64)
  return np.ascontiguousarray((g @ g.T).astype(F32))


# ---------------------------------------------------------------------------------------------
# metrics
def truth(a32):
  """Ascending float64 eigenvalues of the float32 matrix."""
  return np.linalg.eigvalsh(a32.astype(np.float64))


def metrics(a32, e, v, w64=None):
  """eig_err, resid, orth (each / ||A||_2, or / 1 for the zero matrix), sorted, rel_eig_err: all in float64."""
  a = a32.astype(np.float64)
  e = np.asarray(e, np.float64)
  v = np.asarray(v, np.float64)
  w = truth(a32) if w64 is None else w64
  nrm = float(np.abs(w).max()) if w.size else 0.0
  if nrm == 0.0:
    nrm = 1.0
  a, e, w = a / nrm, e / nrm, w / nrm      # before any product: 2^34-scaled inputs square out of range otherwise
  n = a.shape[0]
  with np.errstate(all="ignore"):
    out = {"eig_err": float(np.abs(np.sort(e) - w).max()),
           "resid": float(np.abs(a @ v - v * e).max()),
           "orth": float(np.abs(v.T @ v - np.eye(n)).max()),
           "sorted": bool((np.diff(e) >= 0).all()),
           "rel_eig_err": float((np.abs(e - w) / np.abs(w)).max()) if (w > 0).all() else float("nan")}
  for k in ("eig_err", "resid", "orth"):
    if not np.isfinite(out[k]):
      out[k] = float("inf")
  return out


def yardstick(a32, w64=None):
  """The same metrics for float32 LAPACK (ssyevd) on the same input."""
  from oracle.lapack32 import eigh32
  e, v = eigh32(a32)
  return metrics(a32, e, v, w64)


def check(a32, e, v, floors, yard=None, w64=None):
  """(metrics, list of violated bounds) of one solver result under the bound rule."""
  w64 = truth(a32) if w64 is None else w64
  m = metrics(a32, e, v, w64)
  y = yardstick(a32, w64) if yard is None else yard
  bad = [(k, m[k], bound(k, y[k], floors[k])) for k in ("eig_err", "resid", "orth")
         if not m[k] <= bound(k, y[k], floors[k])]
  if not m["sorted"]:
    bad.append(("sorted", False, True))
  return m, bad


# ---------------------------------------------------------------------------------------------
# mutants: wrong answers a test built on the metrics has to notice
def mutant_swapped_values(a32, e, v):
  e = np.array(e, copy=True)
  i, j = 0, len(e) - 1
  e[i], e[j] = e[j], e[i]
  return e, v


def mutant_diagonal(a32, e, v):
  """What a one-sided Jacobi returns when it never rotates: V = I, lambda = diag(A), sorted."""
  d = np.diag(a32).astype(F32)
  order = np.argsort(d, kind="stable")
  return d[order], np.eye(len(d), dtype=F32)[:, order]


def mutant_scaled_vector(a32, e, v):
  v = np.array(v, copy=True)
  v[:, len(e) // 2] *= F32(1 + 1e-4)
  return e, v


MUTANTS = {"swapped_values": mutant_swapped_values, "diagonal": mutant_diagonal,
           "scaled_vector": mutant_scaled_vector}
