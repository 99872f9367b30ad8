"""Helpers shared by test_every_step_references.py (CPU) and test_gpu_every_step_exact.py (GPU).

The exact-arithmetic method: operands are small integers, so every product and every partial
sum of a contraction is an integer below 2^24 and therefore exactly representable in float32.
The float32 result then does not depend on summation order, tile shape, split count or MFMA
accumulation order, and the expected output is the int64 product -- compared with array_equal.

Precondition (asserted by `assert_exact`): |a|, |b| <= 8 gives |sum| <= 64 k < 2^24 for
k <= 262 144; the sharper max(|A| @ |B|) < 2^24 is what is checked.

Nothing here imports the library's host code: `splitk_for` / `split_plan` restate
csrc/misc.hip, `transform_ref64` restates include/ps_api.h's contract of
ps_transform_grads_f32 and DS:3496-3625 in NumPy float64.
"""
import math

import numpy as np

U = 2.0 ** -24          # unit roundoff of float32
EXACT_LIMIT = 1 << 24   # integers up to here are exact in float32
TILE = 128
KSPLIT_MAX = 64
TCHUNK = 4096
T_EPS = np.float32(1e-25)


# ---------------------------------------------------------------------------
# integer operands
# ---------------------------------------------------------------------------
def int_pattern(rows, cols, salt=0):
  """Non-symmetric, position-dependent integers in [-8, 8]: a transposed or shifted tile
  cannot reproduce them."""
  i = np.arange(rows, dtype=np.int64)[:, None]
  j = np.arange(cols, dtype=np.int64)[None, :]
  return (7 * i + 3 * j + salt) % 17 - 8


def int_random(rng, shape, lo=-8, hi=8):
  return rng.integers(lo, hi + 1, size=shape, dtype=np.int64)


def int_operand(rng, rows, cols, salt):
  """Pattern for even salts, random for odd ones: both kinds appear in every case list."""
  return int_pattern(rows, cols, salt) if salt % 2 == 0 else int_random(rng, (rows, cols))


def assert_exact(abs_bound):
  """abs_bound: max over the output of sum_k |a||b| (plus |old| terms).  Below 2^24 every
  partial sum in any order is an exactly representable integer."""
  assert float(abs_bound) < EXACT_LIMIT, f"integer case is not exact in float32: {abs_bound}"


def product_abs_bound(a, b):
  """max(|A| @ |B|) for int64 operands [m, k] and [k, n] (float64 holds these integers exactly)."""
  return float((np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)).max())


def int_matmul(a, b):
  """Exact product of integer matrices: float64 BLAS is exact below 2^53 and much faster than
  NumPy's int64 loop."""
  c = a.astype(np.float64) @ b.astype(np.float64)
  return c.astype(np.int64)


# ---------------------------------------------------------------------------
# split-K plan of the grouped float32 product (csrc/misc.hip: splitk_for, gplan_build)
# ---------------------------------------------------------------------------
def tiles_of(m, n):
  return ((m + TILE - 1) // TILE) * ((n + TILE - 1) // TILE)


def splitk_for(total_tiles, k):
  if total_tiles >= 512 or k < 512 or (total_tiles >= 256 and k < 2048):
    return 1
  s = (512 + total_tiles - 1) // total_tiles
  s = min(s, k // 256)
  return max(1, min(s, KSPLIT_MAX))


def split_plan(total_tiles, k):
  """(ksplit, kchunk, length of the last split) of one task in a call of `total_tiles` tiles."""
  s = splitk_for(total_tiles, k)
  if s <= 1:
    return 1, k, k
  kchunk = ((k + s - 1) // s + 127) // 128 * 128
  ksplit = (k + kchunk - 1) // kchunk
  if ksplit <= 1:
    return 1, k, k
  return ksplit, kchunk, k - (ksplit - 1) * kchunk


GEMM_LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]
GEMM_KS = [512, 640, 1000, 1153, 1800, 4096, 4100, 50000]
GEMM_MN = [(128, 128), (96, 33), (1, 200), (300, 1), (129, 257)]


def check_split_list(ks=None, mns=None):
  """The conditions the single-task case list of the grouped product must keep covering."""
  ks = GEMM_KS if ks is None else ks
  mns = GEMM_MN if mns is None else mns
  plans = [split_plan(tiles_of(m, n), k) for (m, n) in mns for k in ks]
  assert all(1 < p[0] <= KSPLIT_MAX for p in plans), "every listed case must take the split"
  rem = {p[0] % 4 for p in plans}
  assert rem == {0, 1, 2, 3}, f"split counts modulo 4 seen: {sorted(rem)}"
  assert any(p[2] < p[1] for p in plans), "no short last split"
  assert any(p[2] % 16 != 0 for p in plans), "no last split off the K-tile"
  return plans


# ---------------------------------------------------------------------------
# float64 restatement of the fused transform (ps_api.h contract; DS:3496-3625)
# ---------------------------------------------------------------------------
G_NONE, G_SGD, G_ADAGRAD, G_RMSPROP, G_RMSPROP_N, G_SQRT_N, G_ADAGRAD_N = range(7)
_DIAG = (G_ADAGRAD, G_RMSPROP, G_RMSPROP_N, G_ADAGRAD_N)
_NORMALIZED = (G_RMSPROP_N, G_ADAGRAD_N)

CFG_DEFAULT = dict(graft_type=G_SGD, nesterov=0, moving_average_for_momentum=0,
                   decoupled_learning_rate=0, decoupled_weight_decay=0, run_shampoo=1,
                   beta1=0.0, beta2_w1=1.0, beta2_w2=1.0, diagonal_epsilon=1e-10,
                   weight_decay=0.0, lr=0.05, clip_by_scaled_gradient_norm=0.0)


def make_cfg(**kw):
  cfg = dict(CFG_DEFAULT)
  cfg.update(kw)
  return cfg


def has_diag(graft):
  return int(graft) in _DIAG


def _f(cfg, name):
  """A float field of ps_transform_config is a float32: the contract's input is the rounded
  value, and the restatement starts from it."""
  return float(np.float32(cfg[name]))


def norm_depth(numel):
  """Summation depth D of one per-parameter norm of csrc/transform.hip: 16 adds per thread, 6
  wave levels and 3 block adds inside a 4096-element chunk, then ceil(nchunks / 256) adds per
  thread and 6 + 3 levels across the chunks.  All addends are non-negative, so the computed sum
  has a relative error of at most (D + 1) u (the squares add one rounding)."""
  nchunks = (int(numel) + TCHUNK - 1) // TCHUNK
  return 16 + 6 + 3 + (nchunks + 255) // 256 + 9


def transform_ref64(items, cfg, consume=None, block=1 << 22):
  """items: dicts of NumPy arrays {grad, pgrad | None, param | None, diag_in | None, mom_in,
  dmom_in}; cfg: fields of ps_transform_config.  Returns per item a dict
  name -> (value, magnitude) for upd, mom, dmom and (Adagrad / RMSProp grafting) diag, all
  float64 and flat.  `magnitude` is the same formula with every addend replaced by its absolute
  value: the scale a rounding error of the float32 evaluation is relative to.

  The arrays are walked in slices of `block` elements (the norms first, then the elementwise
  part), so a 38 M-element parameter needs a few hundred MB of float64 temporaries, not several
  GB.  With `consume(item, name, lo, hi, value, magnitude)` the slices are handed over instead
  of being collected, and the function returns None."""
  graft = int(cfg["graft_type"])
  lr, beta1 = _f(cfg, "lr"), _f(cfg, "beta1")
  w1, w2 = _f(cfg, "beta2_w1"), _f(cfg, "beta2_w2")
  deps, wd = _f(cfg, "diagonal_epsilon"), _f(cfg, "weight_decay")
  clip = _f(cfg, "clip_by_scaled_gradient_norm")
  eps = float(T_EPS)
  dec_lr, dec_wd = bool(cfg["decoupled_learning_rate"]), bool(cfg["decoupled_weight_decay"])
  pm = 1.0 if dec_lr else lr                       # DS:3549
  w = (1.0 - beta1) if cfg["moving_average_for_momentum"] else 1.0
  run = 1.0 if cfg["run_shampoo"] else 0.0
  mm = lr if dec_lr else 1.0                       # DS:3610
  wd_lr = 1.0 if dec_lr else lr
  out = []

  def flat(a):
    return None if a is None else np.asarray(a).ravel()

  for idx, it in enumerate(items):
    g_all, pg_all, prm_all = flat(it["grad"]), flat(it.get("pgrad")), flat(it.get("param"))
    diag_all, mom_all, dmom_all = flat(it.get("diag_in")), flat(it["mom_in"]), flat(it["dmom_in"])
    n = g_all.size
    ranges = [(lo, min(lo + block, n)) for lo in range(0, n, block)] or [(0, 0)]

    def f64(a, lo, hi):
      return a[lo:hi].astype(np.float64)

    def sumsq(fn):
      total = 0.0
      for lo, hi in ranges:
        x = fn(lo, hi)
        total += float(np.dot(x, x))
      return total

    with np.errstate(all="ignore"):
      gden = 1.0
      if graft in _NORMALIZED:
        gden = math.sqrt(sumsq(lambda lo, hi: f64(g_all, lo, hi))) + eps

      def graft_part(lo, hi):
        """Grafting update before clipping and lr (DS:3502-3528) -> (u, new_diag, its magnitude)."""
        g = f64(g_all, lo, hi)
        if graft in _DIAG:
          diag = f64(diag_all, lo, hi)
          scaled = g / gden if graft in _NORMALIZED else g
          if graft in (G_ADAGRAD, G_ADAGRAD_N):
            nd, nd_mag = diag + scaled * scaled, np.abs(diag) + scaled * scaled
          else:
            nd = w1 * diag + w2 * (scaled * scaled)
            nd_mag = np.abs(w1 * diag) + np.abs(w2 * (scaled * scaled))
          return scaled / (np.sqrt(nd) + deps), nd, nd_mag
        if graft == G_SQRT_N:
          return np.sign(g), None, None
        return g, None, None

      clip_div = 1.0
      if graft in (G_RMSPROP, G_RMSPROP_N) and clip > 0.0 and n:   # DS:3531-3535
        unorm = math.sqrt(sumsq(lambda lo, hi: graft_part(lo, hi)[0]))
        clip_div = max(1.0, (unorm / math.sqrt(float(n))) / clip)
      gnorm = math.sqrt(sumsq(lambda lo, hi: graft_part(lo, hi)[0] / clip_div * pm))
      if pg_all is None:                            # DS:3557-3561: precond_grad = grafting_update
        pnorm = gnorm
      else:
        pnorm = math.sqrt(sumsq(lambda lo, hi: f64(pg_all, lo, hi)))
      mult = gnorm / (pnorm + eps) if graft != G_NONE else 1.0   # DS:3566-3569

      pieces = {}
      for lo, hi in ranges:
        gu, nd, nd_mag = graft_part(lo, hi)
        gu = gu / clip_div * pm
        pg = gu if pg_all is None else f64(pg_all, lo, hi)
        su = pg * mult
        su_mag, gu_mag = np.abs(su), np.abs(gu)
        sw, gw = su, gu
        if wd != 0.0:
          prm = f64(prm_all, lo, hi)
          if not dec_wd:
            sw, gw = su + wd * prm, gu + wd * prm
            su_mag, gu_mag = su_mag + np.abs(wd * prm), gu_mag + np.abs(wd * prm)
        mom, dmom = f64(mom_all, lo, hi), f64(dmom_all, lo, hi)
        smom, smom_mag = mom * beta1 + w * sw, np.abs(mom * beta1) + abs(w) * su_mag   # DS:3581-3586
        gmom, gmom_mag = dmom * beta1 + w * gw, np.abs(dmom * beta1) + abs(w) * gu_mag
        mom_u, mom_u_mag = run * smom + (1.0 - run) * gmom, run * smom_mag + (1.0 - run) * gmom_mag
        wd_u, wd_u_mag = run * sw + (1.0 - run) * gw, run * su_mag + (1.0 - run) * gu_mag
        nest, nest_mag = mom_u, mom_u_mag
        if cfg["nesterov"]:                         # DS:3601-3602
          nest = w * wd_u + beta1 * mom_u
          nest_mag = abs(w) * wd_u_mag + abs(beta1) * mom_u_mag
        if wd != 0.0 and dec_wd:
          nest = nest + wd_lr * wd * prm
          nest_mag = nest_mag + np.abs(wd_lr * wd * prm)
        part = {"upd": (-1.0 * mm * nest, abs(mm) * nest_mag), "mom": (smom, smom_mag),
                "dmom": (gmom, gmom_mag)}
        if nd is not None:
          part["diag"] = (nd, nd_mag)
        for name, (val, mag) in part.items():
          if consume is not None:
            consume(idx, name, lo, hi, val, mag)
          else:
            pieces.setdefault(name, []).append((val, mag))
    if consume is None:
      out.append({name: (np.concatenate([p[0] for p in ps]), np.concatenate([p[1] for p in ps]))
                  for name, ps in pieces.items()})
  return None if consume is not None else out


def bound_ratio(got, ref, mag, factor):
  """max |got - ref| / (factor * u * magnitude) over the elements with a finite reference; 0
  where got == ref.  Elements whose reference is not finite are compared elsewhere."""
  got = np.asarray(got, np.float64).ravel()
  ref = np.asarray(ref, np.float64).ravel()
  mag = np.asarray(mag, np.float64).ravel()
  ok = np.isfinite(ref) & np.isfinite(mag)
  if not ok.any():
    return 0.0
  err = np.abs(got[ok] - ref[ok])
  bnd = factor * U * mag[ok]
  with np.errstate(all="ignore"):
    r = np.where(err == 0.0, 0.0, err / bnd)
  r = np.where(np.isnan(r), np.inf, r)
  return float(np.max(r))


# ---------------------------------------------------------------------------
# vectors with exactly known norms (norm probes of the fused transform)
# ---------------------------------------------------------------------------
def hot_chunks(numel):
  nch = (numel + TCHUNK - 1) // TCHUNK
  return sorted({c for c in (0, 255, 256, 257, 511, 512, nch - 1) if 0 <= c < nch})


def exact_norm_vector(numel, dense, with_twos=False):
  """int64 vector of `numel` entries from {0, +-1, +-2} whose sum of squares is a perfect square
  below 2^24.  dense: floor(sqrt(numel))^2 entries +-1 (every chunk contributes); otherwise only
  the chunks of hot_chunks() hold non-zeros, each a different count, so that a chunk that is
  lost, doubled or credited to a neighbouring parameter changes the norm.  with_twos: some
  groups of four +-1 in chunk 0 become one +-2 and three zeros (same sum of squares).
  Returns (vector, sqrt of the sum of squares)."""
  x = np.zeros(numel, np.int64)
  if numel == 0:
    return x, 0
  if dense:
    s = math.isqrt(numel)
    idx = np.arange(s * s)
    x[idx] = np.where((idx * 7 + idx // TCHUNK) % 3 == 0, -1, 1)   # the tail stays zero
  else:
    hot = hot_chunks(numel)
    caps = [min(TCHUNK, numel - c * TCHUNK) for c in hot]
    weights = np.arange(1, len(hot) + 1, dtype=np.float64)   # shares 1 : 2 : 3 ... of half the room
    s = max(1, math.isqrt(max(1, int(0.5 * sum(caps)))))
    total = s * s
    counts = [min(cap, int(total * wt / weights.sum())) for cap, wt in zip(caps, weights)]
    rest = total - sum(counts)
    for i in range(len(hot)):
      add = min(rest, caps[i] - counts[i])
      counts[i] += add
      rest -= add
    assert rest == 0, (numel, counts)
    for c, cnt in zip(hot, counts):
      idx = np.arange(cnt)
      x[c * TCHUNK + idx] = np.where((idx + c) % 2 == 0, 1, -1)
  if with_twos:
    nz = np.flatnonzero(x[:TCHUNK])
    for q in range(min(len(nz) // 4, 25)):
      grp = nz[4 * q:4 * q + 4]
      x[grp[0]] = 2 * x[grp[0]]
      x[grp[1:]] = 0
  ss = int(np.sum(x * x))
  root = math.isqrt(ss)
  assert root * root == ss and ss < EXACT_LIMIT, (numel, ss)
  return x, root


def ulp_distance(a, b):
  """Distance in units of the last place between two finite float32 arrays."""
  a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
  b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
  a = np.where(a < 0, -(a & 0x7fffffff), a)
  b = np.where(b < 0, -(b & 0x7fffffff), b)
  return np.abs(a - b)
