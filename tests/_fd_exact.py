"""Helpers shared by test_fd_exact_references.py (CPU) and test_gpu_fd_exact.py (GPU): the
exact-arithmetic method of tests/_exact.py carried over to the bf16 kernels of the
Frequent-Directions branch (csrc/gemm_bf16.hip, csrc/fd.hip).

A bf16 plane holds 8 significant bits, so a product of two plane entries is exact in float32,
and a float32 accumulation of such products is exact in ANY order when every partial sum is
representable.  The expected value is therefore defined from the PLANES (a NumPy restatement of
the conversion's definition in include/ps_api.h), not from the float32 operand:
  hi/lo pair on both sides   Ah Bh + Al Bh + Ah Bl           (no Al Bl)
  six-product form           p0q0 + p0q1 + p1q0 + p1q1 + p0q2 + p2q0
and compared with array_equal, whatever the tile shape, the split count or the summation order.

Precondition, asserted per case by `assert_planes_exact`: every kept plane product is a multiple
of one power of two q (q = the product of the lowest set bits of the two operands' planes), and
the maximum over the outputs of the summed absolute products is below 2^24 q.  This generalises
_exact.assert_exact (q = 1, one plane).

Nothing here imports the library's host code: the layouts restate include/ps_api.h, the plans
restate csrc/gemm_bf16.hip (hsplit_for, sym_plan, fd_half_blocks).
"""
import functools

import numpy as np

from tests._exact import EXACT_LIMIT, TILE, assert_exact, int_pattern, tiles_of

HBK = 32            # k per stage of the bf16 product: k % 32 == 0, split chunks are multiples of it
BF16_SENT = 0x5A5A  # sentinel bit pattern of the plane buffers (1.5e16: no test value has it)


# ---------------------------------------------------------------------------
# float32 -> bf16, round to nearest even, as bit operations on the uint32 view
# ---------------------------------------------------------------------------
def _u32(x):
  return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def bf16_bits(x):
  """uint16 bf16 bit patterns of RNE_bf16(x).  Finite values add 0x7fff plus the lowest kept bit
  and drop the low half (a finite value at or above 0x7f7f8000 thereby becomes infinity), +-inf
  pass, a NaN keeps its upper half with the quiet bit set (NaNs are compared by position)."""
  u = _u32(x)
  nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
  r = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
  q = (u >> np.uint32(16)) | np.uint32(0x0040)
  return np.where(nan, q, r).astype(np.uint16)


def bf16_to_f32(bits):
  return (np.asarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_rne(x):
  """RNE_bf16(x) as float32."""
  return bf16_to_f32(bf16_bits(x))


def bf16_split(x, planes):
  """[hi, lo, lo2][:planes] as float32 arrays: hi = RNE_bf16(x), lo = RNE_bf16(x - hi),
  lo2 = RNE_bf16((x - hi) - lo), the subtractions in float32 (ps_api.h: ps_convert_f32_to_bf16,
  ps_convert_f32_to_bf16x3_frag).

  Float32 subnormals are outside the contract, and so are values whose residual x - hi is
  subnormal: whether the conversion instruction and the subtraction flush them is the device's
  denormal mode, not the library's definition.  Callers keep |x| >= 2^-100 or x == 0 (the
  residuals are then multiples of 2^-123 and normal)."""
  x = np.ascontiguousarray(x, dtype=np.float32)
  out = []
  with np.errstate(all="ignore"):
    rest = x
    for _ in range(planes):
      p = bf16_rne(rest)
      out.append(p)
      rest = (rest - p).astype(np.float32)
  return out


def is_nan_bits(bits):
  return (np.asarray(bits, np.uint16) & np.uint16(0x7fff)) > np.uint16(0x7f80)


# ---------------------------------------------------------------------------
# destination layouts of the conversions (include/ps_api.h): element (r, c) -> offset
# ---------------------------------------------------------------------------
def _grid(rows, cols):
  return (np.arange(rows, dtype=np.int64)[:, None], np.arange(cols, dtype=np.int64)[None, :])


def idx_plain(rows, cols, ld):
  r, c = _grid(rows, cols)
  return r * ld + c


def idx_transposed(rows, cols, ld):
  r, c = _grid(rows, cols)
  return c * ld + r


def idx_tiled(rows, cols):
  """transpose = 2: tile (i, j) of 128 rows x 32 columns contiguous at (i * (cols / 32) + j) * 4096;
  the destination holds ceil(rows / 128) * 128 * cols elements, rows past `rows` zero."""
  assert cols % 32 == 0
  r, c = _grid(rows, cols)
  return ((r // 128) * (cols // 32) + c // 32) * 4096 + (r % 128) * 32 + c % 32


def tiled_numel(rows, cols):
  return (rows + 127) // 128 * 128 * cols


def idx_frag_left(rows, cols):
  """transpose = 3 (fragment-major left operand): element (r, k) at
  (((r / 64) * (cols / 16) + k / 16) * 2 + (r % 64) / 32) * 512 + (32 * ((k % 16) / 8) + r % 32) * 8 + k % 8."""
  assert rows % 64 == 0 and cols % 64 == 0
  r, k = _grid(rows, cols)
  return ((((r // 64) * (cols // 16) + k // 16) * 2 + (r % 64) // 32) * 512
          + (32 * ((k % 16) // 8) + r % 32) * 8 + k % 8)


def idx_frag_iter(n, b):
  """Fragment-major planes of one factor's iterate [n][b] (ps_fd_filter_step_f32 with ldt = 0):
  element (row r, column c) at ((r / 16) * (b / 32) + c / 32) * 512 + (32 * ((r % 16) / 8) + c % 32) * 8 + r % 8;
  factor j starts at j * n * b."""
  assert n % 64 == 0 and b % 32 == 0
  r, c = _grid(n, b)
  return ((r // 16) * (b // 32) + c // 32) * 512 + (32 * ((r % 16) // 8) + c % 32) * 8 + r % 8


def idx_iter_transposed(batch, n, b, ldt):
  """Transposed planes of the stacked iterates [batch][n][b]: element (j, r, c) at c * ldt + j * n + r."""
  j = np.arange(batch, dtype=np.int64)[:, None, None]
  r = np.arange(n, dtype=np.int64)[None, :, None]
  c = np.arange(b, dtype=np.int64)[None, None, :]
  return c * ldt + j * n + r


def idx_iter_frag(batch, n, b):
  j = np.arange(batch, dtype=np.int64)[:, None, None]
  return j * (n * b) + idx_frag_iter(n, b)[None]


# ---------------------------------------------------------------------------
# plans (csrc/gemm_bf16.hip)
# ---------------------------------------------------------------------------
def hsplit_for(total_tiles, k):
  """Split only when the call has fewer than 512 tiles and k >= 1024;
  s = min(ceil(512 / tiles), k / 512, 16)."""
  if total_tiles >= 512 or k < 1024:
    return 1
  s = (512 + total_tiles - 1) // total_tiles
  s = min(s, k // 512)
  return max(1, min(s, 16))


def hsplit_plan(total_tiles, k):
  """(ksplit, kchunk, length of the last piece); the chunk is rounded up to 32."""
  s = hsplit_for(total_tiles, k)
  if s <= 1:
    return 1, k, k
  kchunk = ((k + s - 1) // s + HBK - 1) // HBK * HBK
  ksplit = (k + kchunk - 1) // kchunk
  if ksplit <= 1:
    return 1, k, k
  return ksplit, kchunk, k - (ksplit - 1) * kchunk


SYM_SLOTS, SYM_TAIL_MAX, SYM_NKS = 512, 64, 32


def sym_plan(m, k):
  """Symmetric product: dict(tiles, tail, kc, nks, last): the last `tail` of the T (T + 1) / 2
  upper tiles are cut along k into nks pieces of kc (the last piece `last`)."""
  t = (m + TILE - 1) // TILE
  tiles = t * (t + 1) // 2
  tail, want = 0, 1
  if tiles < SYM_SLOTS:
    tail = tiles
    want = min(SYM_NKS, (SYM_SLOTS + tiles - 1) // tiles)
  elif tiles % SYM_SLOTS != 0 and tiles % SYM_SLOTS <= SYM_TAIL_MAX:
    tail = tiles % SYM_SLOTS
    want = SYM_NKS
  kc = max(4 * HBK, ((k + want - 1) // want + HBK - 1) // HBK * HBK)
  nks = (k + kc - 1) // kc
  if nks <= 1:
    tail, nks, kc = 0, 1, k
  return dict(tiles=tiles, tail=tail, kc=kc, nks=nks, last=k - (nks - 1) * kc)


def fd_half_blocks(batch, n):
  """The fused kernels run 32-row workgroups when batch * n / 64 < 129, 64-row ones otherwise."""
  return batch * (n // 64) < 129


# ---------------------------------------------------------------------------
# committed case lists
# ---------------------------------------------------------------------------
GEMM_MN = [(1, 1), (33, 200), (128, 128), (129, 257), (200, 96), (300, 1)]
GEMM_K_UNSPLIT = [32, 64, 96, 160]
GEMM_K_SPLIT = [1024, 1056, 1568, 8192]
SPLITS = [(2, 2), (2, 1), (1, 2), (1, 1)]          # (planes of A, planes of B): the four instances
GEMM_TILED = [(128, 96, 96), (200, 96, 96), (128, 96, 1056), (200, 33, 1568)]   # (m, n, k), a_tiled = 1
GEMM_MIXED = [(129, 257, 1568, (2, 2)), (33, 200, 96, (2, 1)), (128, 128, 1024, (1, 2)),
              (300, 1, 160, (2, 2)), (200, 96, 8192, (1, 1)), (1, 1, 32, (2, 2))]
SYM_CASES = [(128, 64), (200, 160), (257, 1056), (4096, 160)]   # (m, k)
SYM_PAIR = [(200, 160), (257, 1056)]
FUSED_SHAPES = [(1, 128, 32), (3, 256, 96), (2, 384, 64), (16, 640, 96)]   # (batch, n, b)
CY_STEPS = [2, 5]
FILTER_DYADIC = [(3, 200, 40), (3, 128, 96)]       # (batch, n, b)
FILTER_DYADIC_STEPS = [1, 2, 7]
FILTER_GENERAL = [(3, 200, 40), (3, 128, 96)]
FILTER_GENERAL_STEPS = [1, 2, 4, 9]
COV_SHAPES = [(1, 65), (2, 200), (3, 256)]
COV_DECAYS = [0.5, 1.0, 0.0]
CONVERT_PLAIN = [(1, 1), (63, 65), (64, 64), (65, 130), (200, 33)]
CONVERT_TILED = [(128, 32), (200, 96), (129, 64)]
CONVERT_FRAG = [(64, 64), (128, 192), (256, 128)]


def check_fd_lists(sym_cases=None, fused_shapes=None, k_split=None):
  """The conditions the committed case lists must keep covering (in the manner of
  _exact.check_split_list); other lists can be passed to see a condition fail."""
  SYM_CASES_ = SYM_CASES if sym_cases is None else sym_cases
  FUSED_SHAPES_ = FUSED_SHAPES if fused_shapes is None else fused_shapes
  GEMM_K_SPLIT_ = GEMM_K_SPLIT if k_split is None else k_split
  # every non-symmetric single call (one combination alone: tiles_of; all four: 4 x) below 512 tiles
  plans = {}
  for (m, n) in GEMM_MN:
    for mult in (1, 4):
      assert mult * tiles_of(m, n) < 512
      for k in GEMM_K_UNSPLIT:
        assert hsplit_plan(mult * tiles_of(m, n), k)[0] == 1, "listed as unsplit"
      for k in GEMM_K_SPLIT_:
        plans[(m, n, k, mult)] = hsplit_plan(mult * tiles_of(m, n), k)
  assert all(p[0] > 1 for p in plans.values()), "every listed split case must split"
  seen = {p[0] for p in plans.values()}
  assert {2, 3, 16} <= seen, f"split counts seen: {sorted(seen)}"
  assert any(p[2] < p[1] for p in plans.values()), "no short last split"
  for mult in (1, 4):
    assert plans[(129, 257, 1056, mult)] == (2, 544, 512)
    assert plans[(129, 257, 1568, mult)] == (3, 544, 480)
    assert plans[(129, 257, 8192, mult)][0] == 16
  nks = {(m, n, k): hsplit_plan(sum(tiles_of(a, b) for (a, b, _, _) in GEMM_MIXED), k)[0]
         for (m, n, k, _) in GEMM_MIXED}
  assert any(v > 1 for v in nks.values()) and any(v == 1 for v in nks.values()), "mixed call: both kinds"
  assert {k % 64 for k in GEMM_K_UNSPLIT} == {0, 32}, "odd and even numbers of K tiles"
  assert 32 in GEMM_K_UNSPLIT, "one K tile"
  # symmetric products
  sp = {c: sym_plan(*c) for c in SYM_CASES_}
  assert any(p["tail"] == 0 and p["nks"] == 1 for p in sp.values()), "no uncut symmetric product"
  assert any(p["tiles"] < SYM_SLOTS and p["tail"] == p["tiles"] and p["nks"] > 1 for p in sp.values()), \
      "no symmetric product cut as a whole"
  assert any(p["tiles"] >= SYM_SLOTS and 0 < p["tail"] <= SYM_TAIL_MAX and p["nks"] > 1
             for p in sp.values()), "no symmetric product cut in the tail round only"
  assert any(p["nks"] > 1 and p["last"] < p["kc"] for p in sp.values()), "no short last piece"
  assert sp[(128, 64)] == dict(tiles=1, tail=0, kc=64, nks=1, last=64)
  assert sp[(200, 160)] == dict(tiles=3, tail=3, kc=128, nks=2, last=32)
  assert sp[(257, 1056)] == dict(tiles=6, tail=6, kc=128, nks=9, last=32)
  assert sp[(4096, 160)] == dict(tiles=528, tail=16, kc=128, nks=2, last=32)
  assert all(c in SYM_CASES_ for c in SYM_PAIR) and len({m for m, _ in SYM_PAIR}) == len(SYM_PAIR)
  # fused kernels: both workgroup forms, every column count
  forms = {fd_half_blocks(bt, n) for (bt, n, _) in FUSED_SHAPES_}
  assert forms == {True, False}, "both workgroup forms of the fused kernels"
  assert {b for (_, _, b) in FUSED_SHAPES_} == {32, 64, 96}
  assert all(n % 128 == 0 and bt <= 16 for (bt, n, _) in FUSED_SHAPES_)
  return plans, sp


# ---------------------------------------------------------------------------
# operands: integers, position dependent (a shifted or transposed tile cannot reproduce them)
# ---------------------------------------------------------------------------
def _special_grid(rows, cols):
  """Columns are grouped in `stride`-wide slots (8 slots at most, spread over the whole k range, so
  every split piece holds some): special entries sit at fixed lanes of a slot."""
  i, j = _grid(rows, cols)
  stride = max(8, cols // 8)
  return i, j, j % stride, j // stride


def narrow(rows, cols, salt=0):
  """Entries in [-8, 8]: one plane, lo = 0."""
  return int_pattern(rows, cols, salt)


def wide(rows, cols, salt, lane, lo=257, hi=32767, every=3):
  """narrow() with sparse wide entries (|v| in [lo, hi]: two planes below 2^17, up to three below
  2^24) at column lane `lane` of a slot, on every third row (which rows: depends on the slot).  Wide
  entries of the two operands use different lanes (1 for the left, 5 for the right operand), so
  a wide entry meets narrow ones only: each cross term alone."""
  x = narrow(rows, cols, salt)
  i, j, ln, slot = _special_grid(rows, cols)
  v = lo + (i * 131 + j * 71 + salt * 17) % (hi - lo + 1)
  v = np.where((i + j) % 2 == 0, v, -v)
  return np.where((ln == lane) & ((i + slot) % every == 0), v, x)


def medium(rows, cols, salt, hi, base=None):
  """`base` (narrow by default) with medium entries of 9 bits up to `hi` (<= 12 bits) at lane 3 of
  every second slot, on every second row: medium entries of both operands share the lane, so they
  MEET (p1 q1 of the six-product form; a stray lo lo on the three-product form)."""
  x = narrow(rows, cols, salt) if base is None else base
  i, j, ln, slot = _special_grid(rows, cols)
  v = 257 + (i * 37 + j * 101 + salt * 29) % (hi - 257 + 1)
  v = np.where((i + 2 * j) % 3 == 0, -v, v)
  return np.where((ln == 3) & (slot % 2 == 0) & ((i + slot // 2) % 2 == 0), v, x)


def left_operand(rows, cols, salt, wlo=257, whi=32767, mhi=4095, every=3):
  return medium(rows, cols, salt, mhi, base=wide(rows, cols, salt, 1, wlo, whi, every))


def right_operand(rows, cols, salt, wlo=257, whi=32767, mhi=511, every=3):
  """Stored K-contiguous like the left one: [n][k]."""
  return medium(rows, cols, salt + 1, mhi, base=wide(rows, cols, salt + 1, 5, wlo, whi, every))


def sym_operand(rows, cols, salt):
  """Operand of c = a a^T: it meets itself, so its two-plane entries are 9 to 10 bits only."""
  return medium(rows, cols, salt, 1023)


def kept_products(sa, sb):
  """Plane pairs the kernels accumulate: all with i + j <= 1 for hi/lo pairs (and single planes),
  all with i + j <= 2 for the three-plane form."""
  top = 2 if max(sa, sb) == 3 else 1
  return [(i, j) for i in range(sa) for j in range(sb) if i + j <= top]


def _lowest_bit(planes):
  """Largest power of two that divides every non-zero entry of the planes."""
  q = None
  for p in planes:
    v = np.abs(np.asarray(p, np.float64).ravel())
    v = v[v != 0]
    if v.size == 0:
      continue
    m, e = np.frexp(v)
    mi = (m * float(1 << 53)).astype(np.int64)
    low = (mi & -mi).astype(np.float64) * np.exp2((e - 53).astype(np.float64))
    q = float(low.min()) if q is None else min(q, float(low.min()))
  return 1.0 if q is None else q


def assert_planes_exact(a_planes, b_planes, extra_abs=None):
  """The condition that makes a plane product exact in float32 in any summation order: with
  q = lowest bit of A's planes times lowest bit of B's planes every plane product is a multiple
  of q, and max(sum_i |A_i| @ sum_j |B_j|^T) -- an upper bound of the summed absolute kept
  products -- is below 2^24 q.  Returns (q, bound / q)."""
  for p in list(a_planes) + list(b_planes):
    assert np.isfinite(p).all()
  q = _lowest_bit(a_planes) * _lowest_bit(b_planes)
  sa = sum(np.abs(np.asarray(p, np.float64)) for p in a_planes)
  sb = sum(np.abs(np.asarray(p, np.float64)) for p in b_planes)
  bound = sa @ sb.T
  if extra_abs is not None:
    bound = bound + extra_abs
  ratio = float(bound.max()) / q
  assert ratio < EXACT_LIMIT, f"plane product is not exact in float32: {ratio} q, q = {q}"
  return q, ratio


def planes_product(a_planes, b_planes, kept):
  """sum over the kept pairs of A_i @ B_j^T in float64 (exact: integers far below 2^53)."""
  out = None
  for (i, j) in kept:
    t = np.asarray(a_planes[i], np.float64) @ np.asarray(b_planes[j], np.float64).T
    out = t if out is None else out + t
  return out


@functools.lru_cache(maxsize=8)
def product_case(m, n, k, salt, scale_a=1.0, scale_b=1.0):
  """Operands of one non-symmetric product: (a [m][k] float32, bt [n][k] float32, planes of a,
  planes of bt, {(sa, sb): expected float64}).  The exactness precondition is asserted here."""
  a = (left_operand(m, k, salt) * scale_a).astype(np.float32)
  bt = (right_operand(n, k, salt) * scale_b).astype(np.float32)
  ap, bp = bf16_split(a, 2), bf16_split(bt, 2)
  assert_planes_exact(ap, bp)
  exp = {(sa, sb): planes_product(ap[:sa], bp[:sb], kept_products(sa, sb)) for (sa, sb) in SPLITS}
  return a, bt, ap, bp, exp


def product_scales(m, n, k):
  """Some cases scale an operand by a power of two (the planes and q scale with it)."""
  return (0.25 if (m + k // 32) % 3 == 1 else 1.0, 32.0 if (n + k // 32) % 4 == 1 else 1.0)


@functools.lru_cache(maxsize=4)
def sym_case(m, k, salt):
  """(a float32, planes, {sa: expected}) of c = a a^T (the single-plane form only up to m = 1024:
  the big case is run as a hi/lo pair alone)."""
  a = sym_operand(m, k, salt).astype(np.float32)
  ap = bf16_split(a, 2)
  assert_planes_exact(ap, ap)
  exp = {sa: planes_product(ap[:sa], ap[:sa], kept_products(sa, sa)) for sa in ((2, 1) if m <= 1024 else (2,))}
  return a, ap, exp


# ---------------------------------------------------------------------------
# fused filter step and six-product C x
# ---------------------------------------------------------------------------
DYADIC = dict(ctr=0.5, e=0.25, sigma1=1.0)


def sigma_chain32(sigma1, step):
  """float32 evaluation of the kernels' sigma recurrence: (sigma_{step-1}, sigma_step)."""
  s1 = np.float32(sigma1)
  sigma = s1
  for _ in range(2, step):
    sigma = np.float32(1) / (np.float32(2) / s1 - sigma)
  return sigma, np.float32(1) / (np.float32(2) / s1 - sigma)


def dyadic_coefficients(step):
  """With ctr = 0.5, e = 0.25, sigma1 = 1 every sigma_k is 1: y' = (z - y / 2) c1 - c2 y_prev with
  (c1, c2) = (4, 0) at step 1 and (8, 1) afterwards."""
  return (4.0, 0.0) if step <= 1 else (8.0, 1.0)


def dyadic_step(z, y, y_prev, step):
  """Exact y' of the dyadic recurrence (float64 holds it exactly) and the precondition: z, y and
  y_prev are integers, every intermediate is a multiple of 1/2 below 2^23 and the result an
  integer below 2^24."""
  c1, c2 = dyadic_coefficients(step)
  z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
  yp = np.zeros_like(y) if y_prev is None else np.asarray(y_prev, np.float64)
  inner = np.abs(z) + 0.5 * np.abs(y)
  assert float(inner.max()) < EXACT_LIMIT / 2
  assert_exact((inner * c1 + c2 * np.abs(yp)).max())
  return (z - 0.5 * y) * c1 - c2 * yp


def fused_degrees(batch, step):
  """Per-factor degrees: factor 1 (when there is one) has finished (degree < step)."""
  deg = np.full(batch, 12.0, np.float32)
  if batch > 1:
    deg[1] = step - 1
  return deg


@functools.lru_cache(maxsize=4)
def cy_case(batch, n, b, step):
  """Fused step: dict(c [batch][n][n], y, y_prev [batch][n][b] float32, params [batch][4], exp
  [batch][n][b] float64).  z is defined from the hi/lo planes of C and y."""
  c = np.stack([left_operand(n, n, 3 + 2 * j, whi=8191, mhi=511) for j in range(batch)]).astype(np.float32)
  y = np.stack([right_operand(b, n, 11 + 2 * j, whi=8191, mhi=511).T for j in range(batch)]).astype(np.float32)
  y_prev = np.stack([int_pattern(n, b, 5 + j) * 4097 for j in range(batch)]).astype(np.float32)
  deg = fused_degrees(batch, step)
  params = np.stack([np.array([DYADIC["ctr"], DYADIC["e"], DYADIC["sigma1"], d], np.float32) for d in deg])
  exp = np.empty((batch, n, b), np.float64)
  for j in range(batch):
    cp, yp = bf16_split(c[j], 2), bf16_split(np.ascontiguousarray(y[j].T), 2)
    _, ratio = assert_planes_exact(cp, yp)
    z = planes_product(cp, yp, kept_products(2, 2))
    nxt = dyadic_step(z, y[j], y_prev[j], step)
    # the product's absolute sum, not only its value, must leave room for the recurrence
    assert_exact(8.0 * (ratio + 0.5 * float(np.abs(y[j]).max())) + float(np.abs(y_prev[j]).max()))
    exp[j] = nxt if step <= deg[j] else y[j]
  return dict(c=c, y=np.ascontiguousarray(y), y_prev=y_prev, params=params, exp=exp, deg=deg)


@functools.lru_cache(maxsize=4)
def cx6_case(batch, n, b):
  """Six-product C x: wide three-plane entries of C (18 bits: the remainder after the first plane
  has up to 10) meet narrow x, narrow C meets wide x, medium meets medium.  dict(c, x, exp)."""
  c = np.stack([left_operand(n, n, 7 + 2 * j, 131073, 262143, 1023, 4) for j in range(batch)]).astype(np.float32)
  x = np.stack([right_operand(b, n, 13 + 2 * j, 131073, 262143, 511, 4).T for j in range(batch)]).astype(np.float32)
  exp = np.empty((batch, n, b), np.float64)
  for j in range(batch):
    cp, xp = bf16_split(c[j], 3), bf16_split(np.ascontiguousarray(x[j].T), 3)
    assert np.any(cp[2] != 0) and np.any(xp[2] != 0), "no third plane in the case"
    assert_planes_exact(cp, xp)
    exp[j] = planes_product(cp, xp, kept_products(3, 3))
  return dict(c=c, x=np.ascontiguousarray(x), exp=exp)


def place_iter_frag(values):
  """Stacked iterates [batch][n][b] (bf16-representable float32) -> flat uint16 fragment-major planes."""
  batch, n, b = values.shape
  out = np.empty(batch * n * b, np.uint16)
  out[idx_iter_frag(batch, n, b).ravel()] = bf16_bits(values).ravel()
  return out


# ---------------------------------------------------------------------------
# ps_fd_filter_step_f32: dyadic cases and the float64 restatement
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def filter_dyadic_case(batch, n, b, step):
  z = np.stack([wide(n, b, 21 + j, 1, 257, 65535) for j in range(batch)]).astype(np.float32)
  y = np.stack([wide(n, b, 31 + j, 5, 257, 65535) for j in range(batch)]).astype(np.float32)
  y_prev = np.stack([int_pattern(n, b, 41 + j) * 4097 for j in range(batch)]).astype(np.float32)
  deg = fused_degrees(batch, step)
  params = np.stack([np.array([DYADIC["ctr"], DYADIC["e"], DYADIC["sigma1"], d], np.float32) for d in deg])
  exp = np.stack([dyadic_step(z[j], y[j], y_prev[j], step) if step <= deg[j] else y[j].astype(np.float64)
                  for j in range(batch)])
  return dict(z=z, y=y, y_prev=y_prev, params=params, exp=exp, deg=deg)


def filter_factor(step):
  """F of |got - ref| <= F u magnitude for one step of the recurrence, from the kernel's
  operation count (first order in u = 2^-24; every float32 operation is correctly rounded, a
  contraction into an FMA only removes a rounding).

  sigma recurrence: one round is d = 2 / sigma1 (u), s = d - sigma (u on s; the incoming errors
  enter as (d e_d + sigma e_sigma) / (d - sigma), and with sigma <= sigma1 <= 1, d >= 2 that is
  at most 2 e_d + e_sigma), sigma' = 1 / s (u): e' <= e + 4 u.  sigma_{step-1} takes step - 2
  rounds and sigma_step one more: e(sigma) <= 4 (step - 2) u, e(sn) <= 4 (step - 1) u.
  coefficients: c1 = 2 sn / e is one division, e(c1) <= e(sn) + u; c2 = sigma sn is one product,
  e(c2) <= e(sigma) + e(sn) + u.
  multiply-adds: t = ctr y (u), w = z - t (u), x = w c1 (u + e(c1)), p = c2 y_prev (u + e(c2)),
  x - p (u).  Relative to magnitude = (|z| + |ctr y|) |c1| + |c2 y_prev| the first term carries
  4 u + e(c1) = (4 step + 1) u and the second 2 u + e(c2) = (8 step - 9) u.
  F = 8 step + 8 covers both for every step >= 1 (step 1: c1 = sigma1 / e, 4 u in all) and
  leaves 9 u or more for the second-order terms."""
  return 8.0 * step + 8.0


def filter_step_ref64(z, y, y_prev, params, step):
  """float64 restatement of ps_fd_filter_step_f32 (include/ps_api.h) for stacked [batch][n][b]
  arrays and params [batch][4] = {ctr, e, sigma1, degree} (the float32 values are the inputs).
  step 1: y' = (z - ctr y) sigma1 / e; step k >= 2: y' = (z - ctr y) 2 sigma_k / e
  - sigma_{k-1} sigma_k y_prev, sigma_m = 1 / (2 / sigma1 - sigma_{m-1}); degree < step keeps y.
  Returns (value, magnitude): magnitude is the same formula with absolute values."""
  z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
  val, mag = np.empty_like(y), np.empty_like(y)
  for j in range(y.shape[0]):
    ctr, e, sigma1, deg = (float(v) for v in np.asarray(params[j], np.float32))
    if step > int(deg):
      val[j], mag[j] = y[j], np.abs(y[j])
      continue
    if step <= 1:
      c1, c2 = sigma1 / e, 0.0
    else:
      sigma = sigma1
      for _ in range(2, step):
        sigma = 1.0 / (2.0 / sigma1 - sigma)
      sn = 1.0 / (2.0 / sigma1 - sigma)
      c1, c2 = 2.0 * sn / e, sigma * sn
    yp = np.zeros_like(y[j]) if step <= 1 else np.asarray(y_prev[j], np.float64)
    val[j] = (z[j] - ctr * y[j]) * c1 - c2 * yp
    mag[j] = (np.abs(z[j]) + np.abs(ctr * y[j])) * abs(c1) + np.abs(c2 * yp)
  return val, mag


def filter_step_f32(z, y, y_prev, params, step):
  """The same formula evaluated in plain float32 NumPy, operation for operation."""
  f = np.float32
  z, y = np.asarray(z, f), np.asarray(y, f)
  out = np.empty_like(y)
  for j in range(y.shape[0]):
    ctr, e, sigma1, deg = (f(v) for v in np.asarray(params[j], f))
    if step > int(deg):
      out[j] = y[j]
      continue
    if step <= 1:
      out[j] = (z[j] - ctr * y[j]) * (sigma1 / e)
      continue
    sigma, sn = sigma_chain32(sigma1, step)
    c1, c2 = f(2) * sn / e, sigma * sn
    out[j] = (z[j] - ctr * y[j]) * c1 - c2 * np.asarray(y_prev[j], f)
  return out


def control_rows(batch):
  """params rows of the kind ps_fd_round_control_f32 writes (csrc/fd.hip), evaluated in float32:
  ctr = e = cut / 2, sigma1 = e / (top (1 + 1e-6) - ctr), an integer degree.  Mixed degrees."""
  f = np.float32
  tops = [f(10.0), f(3.7), f(118.5), f(1.0)]
  cuts = [f(1.3), f(0.9), f(0.017), f(0.31)]
  degs = [12, 1, 3, 6]
  rows = []
  for j in range(batch):
    top, cut = tops[j % 4], cuts[j % 4]
    e = ctr = f(0.5) * cut
    a0 = top * (f(1.0) + f(1e-6))
    rows.append([ctr, e, e / (a0 - ctr), f(degs[j % 4])])
  return np.asarray(rows, np.float32)


@functools.lru_cache(maxsize=8)
def filter_general_case(batch, n, b):
  rng = np.random.default_rng(7000 + 13 * n + b)
  z = rng.standard_normal((batch, n, b)).astype(np.float32) * np.float32(5.0)
  y = rng.standard_normal((batch, n, b)).astype(np.float32)
  y_prev = rng.standard_normal((batch, n, b)).astype(np.float32)
  return dict(z=z, y=y, y_prev=y_prev, params=control_rows(batch))


# ---------------------------------------------------------------------------
# ps_fd_cov_update_f32
# ---------------------------------------------------------------------------
def cov_case(batch, n, decay):
  """Integer c and non-symmetric integer Gram matrices; decay in {0, 0.5, 1} keeps
  0.5 ((decay c + g) + (decay c + g)^T) exact (multiples of 1/4 far below 2^22)."""
  c = np.stack([int_pattern(n, n, 50 + j) * 129 for j in range(batch)]).astype(np.float64)
  g = np.stack([int_pattern(n, n, 60 + j) * 77 + int_pattern(n, n, 3 * j).T for j in range(batch)]).astype(np.float64)
  assert decay in (0.0, 0.5, 1.0)
  u = decay * c + g
  assert_exact(4.0 * float((np.abs(decay * c) + np.abs(g)).max()) * 2.0)
  exp = 0.5 * (u + np.transpose(u, (0, 2, 1)))
  assert not np.array_equal(g, np.transpose(g, (0, 2, 1)))
  return c.astype(np.float32), g.astype(np.float32), exp


# ---------------------------------------------------------------------------
# inputs of the conversion tests
# ---------------------------------------------------------------------------
SPECIAL_BITS = np.array([
    0x3f808000, 0x3f818000,              # ties: to an even and to an odd mantissa
    0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001,   # one ulp each side of a tie
    0xbf808000, 0xbf818000,
    0x00000000, 0x80000000,              # +-0
    0x7f800000, 0xff800000,              # +-inf
    0x7fc00000, 0xffc00000, 0x7f800001,  # NaNs
    0x7f7f0000, 0xff7f0000,              # the largest finite bf16
    0x7f7f7fff, 0x7f7f8000, 0x7f7fffff, 0xff7f7fff, 0xff7f8000,   # around the overflow threshold
], dtype=np.uint32)
# ties: 65792 (first plane, to the even 65536) and 131329 (second plane: 131072, 256, 1); 65793 is
# NOT a tie (it is above the half and rounds up: 66048, -255, 0); 16777215 rounds up to 2^24
WIDE_INTS = np.array([257, 65793, -65793, 16777215, 511, 65535, -257, 131329, 65792], np.float32)


def special_values():
  return SPECIAL_BITS.view(np.float32).copy()


def convert_input(rows, cols, salt=0):
  """float32 [rows][cols]: normals scaled by powers of two in 2^-20 .. 2^20, every seventh entry a
  wide integer and every fifth a special value (cycled, so every shape above 1 x 1 sees them in
  interior and edge tiles).  No subnormals and |x| >= 2^-100 or 0 (see bf16_split)."""
  rng = np.random.default_rng(900 + 31 * rows + cols + salt)
  x = rng.standard_normal((rows, cols)).astype(np.float32)
  x = np.where(np.abs(x) < 1e-3, np.float32(1e-3), x).astype(np.float32)
  x = x * np.exp2(rng.integers(-20, 21, size=(rows, cols))).astype(np.float32)
  flat = x.ravel()
  idx = np.arange(flat.size)
  sp = special_values()
  flat[idx % 7 == 3] = WIDE_INTS[(idx[idx % 7 == 3] // 7) % WIDE_INTS.size]
  flat[idx % 5 == 0] = sp[(idx[idx % 5 == 0] // 5 + salt) % sp.size]
  x = flat.reshape(rows, cols)
  a = np.abs(x[np.isfinite(x)])
  assert np.all((a == 0) | (a >= 2.0 ** -100))
  return x
