"""Exact-arithmetic tests of the bf16 kernels of the Frequent-Directions branch
(csrc/gemm_bf16.hip, csrc/fd.hip): the conversions, the grouped bf16 product with its split-K and
symmetric plans, the fused filter step, the six-product C x and the elementwise glue.

Method (tests/_fd_exact.py): the expected value is defined from the bf16 PLANES of integer
operands -- a NumPy restatement of the conversion's definition in include/ps_api.h -- as the sum
of the plane products the contract keeps (hi/lo: Ah Bh + Al Bh + Ah Bl; three planes: the six
products with i + j <= 2).  Every such product is exact in float32 and, under the precondition
asserted per case, so is every partial sum in any order: the comparison is array_equal, whatever
the tile shape, split count or summation order.  The conversion kernels are compared bit for bit
with the restatement, the operands of the products are PLACED from the restatement with the
restated layouts, so a fault of the conversion cannot hide in both sides of a comparison.

Every output buffer is pre-filled with a sentinel (NaN for float32, the bit pattern 0x5A5A for
bf16 planes) and everything outside the declared region must still hold it afterwards.

Sensitivity, each mutant of the kernels run once against this file (109 tests, 8 s wall on an
MI355X, no test above 0.4 s) -- the tests that fail:
  Al Bh dropped in the <2, 2> product instance   test_gemm_bf16_exact (47 cases), tile-blocked, mixed, symmetric
  Al Bl added                                    test_gemm_bf16_exact (40 cases), tile-blocked, mixed, symmetric
  split-K reduce starts at piece 1               test_gemm_bf16_exact (the 24 split cases), tile-blocked, mixed
  sym_plan one piece fewer                       test_gemm_bf16_symmetric_exact[257 x 1056], the two-product call
  mirror store un-transposed                     test_gemm_bf16_symmetric_exact[4096 x 160]
  two planes swapped in fd_cx6_kernel            test_fd_cx6_exact (all four shapes)
  sigma1 for sigma in c2 of the filter step      test_fd_filter_step_general_parameters (steps 4 and 9)
  fd_cy_step_kernel before its finished-factor   test_fd_cy_step_exact (every batch > 1 case: the sentinel
  plane copy                                     stays in factor 1's range of nt_hi / nt_lo)
"""
import numpy as np
import pytest
import torch

from tests import _exact as E
from tests import _fd_exact as F

pytestmark = pytest.mark.gpu

GUARD = 64   # sentinel elements before and after a flat output (keeps 16-byte alignment)


def K():
  from precondition_amd import kernels
  return kernels


def _lib():
  from precondition_amd import _lib as L
  return L.lib()


def _check(rc, what):
  from precondition_amd import _lib as L
  L.check(rc, what)


def _stream():
  return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------
def _bf16_full(numel, dev):
  return torch.full((int(numel),), F.BF16_SENT, dtype=torch.int16, device=dev).view(torch.bfloat16)


def _bits_of(t):
  """uint16 bit patterns of a bfloat16 tensor (as stored, flattened)."""
  return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).ravel()


def _to_bf16_tensor(bits, dev):
  return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).to(dev).view(torch.bfloat16)


def _plane_view(plane, ld_pad, dev):
  """A bf16-representable float32 matrix as a device bfloat16 view with leading dimension
  cols + ld_pad inside a sentinel-filled holder."""
  r, c = plane.shape
  holder = _bf16_full(r * (c + ld_pad), dev).view(r, c + ld_pad)
  view = holder[:, :c]
  view.copy_(_to_bf16_tensor(F.bf16_bits(plane), dev).view(r, c))
  return view


def _guarded_f32(shape, dev):
  """(holder, contiguous view of `shape`) with GUARD NaNs before and after."""
  n = int(np.prod(shape))
  holder = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
  return holder, holder[GUARD:GUARD + n].view(*shape)


def _guarded_bf16(numel, dev):
  holder = _bf16_full(numel + 2 * GUARD, dev)
  return holder, holder[GUARD:GUARD + numel]


def _assert_guards_f32(holder, what):
  assert bool(torch.isnan(holder[:GUARD]).all()) and bool(torch.isnan(holder[-GUARD:]).all()), \
      f"{what}: written outside the output"


def _assert_guards_bf16(holder, what):
  bits = _bits_of(holder)
  assert np.all(bits[:GUARD] == F.BF16_SENT) and np.all(bits[-GUARD:] == F.BF16_SENT), \
      f"{what}: written outside the planes"


def _assert_equal(got, exp, what):
  got, exp = np.asarray(got), np.asarray(exp)
  assert got.shape == exp.shape, (what, got.shape, exp.shape)
  if not np.array_equal(got, exp):
    bad = np.argwhere(got != exp)
    first = tuple(bad[0])
    raise AssertionError(
        f"{what}: {len(bad)} of {got.size} elements differ; first at {first}: got {got[first]!r}, "
        f"expected {exp[first]!r}; index ranges "
        + ", ".join(f"{bad[:, d].min()}..{bad[:, d].max()}" for d in range(bad.shape[1])))


def _assert_bits(got, exp, what):
  """Bit for bit; NaNs compared by position."""
  got, exp = np.asarray(got, np.uint16).ravel(), np.asarray(exp, np.uint16).ravel()
  nan = F.is_nan_bits(exp)
  _assert_equal(F.is_nan_bits(got), nan, what + " (NaN positions)")
  _assert_equal(np.where(nan, 0, got), np.where(nan, 0, exp), what)


def _framed(m, n, dev):
  """(holder, view): an m x n float32 output as a strided view (ldc = n + 3) of a NaN-filled holder."""
  holder = torch.full((m + 2, n + 3), float("nan"), dtype=torch.float32, device=dev)
  return holder, holder[1:m + 1, 2:n + 2]


def _check_framed(holder, exp, what):
  """The framed region equals `exp` (float64, exactly representable in float32), the frame is NaN.
  Compared on the device; the host comparison only runs to describe a mismatch."""
  m, n = exp.shape
  e32 = exp.astype(np.float32)
  assert np.array_equal(e32.astype(np.float64), exp)
  inner = holder[1:m + 1, 2:n + 2]
  if not torch.equal(inner, torch.from_numpy(e32).to(holder.device)):
    _assert_equal(inner.cpu().numpy().astype(np.float64), exp, what)
  mask = torch.ones_like(holder, dtype=torch.bool)
  mask[1:m + 1, 2:n + 2] = False
  assert bool(torch.isnan(holder[mask]).all()), f"{what}: written outside the declared region"


# ---------------------------------------------------------------------------
# 1. conversions, bit for bit against the restatement
# ---------------------------------------------------------------------------
def _src_view(x, pad, dev):
  r, c = x.shape
  holder = torch.full((r, c + pad), float("nan"), dtype=torch.float32, device=dev)
  holder[:, :c].copy_(torch.from_numpy(x).to(dev))
  return holder


def _convert(src_holder, hi, lo, rows, cols, ldd, mode):
  _check(_lib().ps_convert_f32_to_bf16(_stream(), src_holder.data_ptr(), hi.data_ptr(),
                                       lo.data_ptr() if lo is not None else None, rows, cols,
                                       int(src_holder.stride(0)), ldd, mode), "ps_convert_f32_to_bf16")


def _expected_planes(x, idx, numel, planes, zero_upto=0):
  out = []
  for p in F.bf16_split(x, planes):
    e = np.full(numel + 2 * GUARD, F.BF16_SENT, np.uint16)
    e[GUARD:GUARD + zero_upto] = 0
    e[GUARD + idx.ravel()] = F.bf16_bits(p).ravel()
    out.append(e)
  return out


@pytest.mark.parametrize("shape", F.CONVERT_PLAIN)
@pytest.mark.parametrize("mode", [0, 1])
def test_convert_plain_and_transposed(device, shape, mode):
  r, c = shape
  x = F.convert_input(r, c, mode)
  for (spad, dpad, split) in [(0, 0, True), (3, 8, True), (5, 1, False)]:
    src = _src_view(x, spad, device)
    ldd = (r if mode else c) + dpad
    numel = (c if mode else r) * ldd
    idx = F.idx_transposed(r, c, ldd) if mode else F.idx_plain(r, c, ldd)
    hh, hi = _guarded_bf16(numel, device)
    lh, lo = _guarded_bf16(numel, device)
    _convert(src, hi, lo if split else None, r, c, ldd, mode)
    exp = _expected_planes(x, idx, numel, 2)
    what = f"mode {mode} {shape} lds +{spad} ldd +{dpad}"
    _assert_bits(_bits_of(hh), exp[0], what + " hi")
    _assert_bits(_bits_of(lh), exp[1] if split else np.full_like(exp[1], F.BF16_SENT), what + " lo")
  if r > 1:
    # the wrapper's planes are the same bits
    h, l = K().to_bf16(torch.from_numpy(x).to(device), split=True, transpose=bool(mode))
    p = F.bf16_split(x.T if mode else x, 2)
    _assert_bits(_bits_of(h), F.bf16_bits(p[0]), "to_bf16 hi")
    _assert_bits(_bits_of(l), F.bf16_bits(p[1]), "to_bf16 lo")


@pytest.mark.parametrize("shape", F.CONVERT_TILED)
def test_convert_tile_blocked(device, shape):
  r, c = shape
  x = F.convert_input(r, c, 2)
  numel = F.tiled_numel(r, c)
  for (spad, split) in [(0, True), (7, True), (1, False)]:
    src = _src_view(x, spad, device)
    hh, hi = _guarded_bf16(numel, device)
    lh, lo = _guarded_bf16(numel, device)
    _convert(src, hi, lo if split else None, r, c, c, 2)
    # the declared region is the whole padded destination: rows past `rows` read as zero
    exp = _expected_planes(x, F.idx_tiled(r, c), numel, 2, zero_upto=numel)
    _assert_bits(_bits_of(hh), exp[0], f"mode 2 {shape} lds +{spad} hi")
    _assert_bits(_bits_of(lh), exp[1] if split else np.full_like(exp[1], F.BF16_SENT), f"mode 2 {shape} lo")


@pytest.mark.parametrize("shape", F.CONVERT_FRAG)
def test_convert_fragment_major(device, shape):
  r, c = shape
  x = F.convert_input(r, c, 3)
  numel, idx = r * c, F.idx_frag_left(r, c)
  exp = _expected_planes(x, idx, numel, 3)
  for spad in (0, 9):
    src = _src_view(x, spad, device)
    hh, hi = _guarded_bf16(numel, device)
    lh, lo = _guarded_bf16(numel, device)
    _convert(src, hi, lo, r, c, c, 3)
    _assert_bits(_bits_of(hh), exp[0], f"mode 3 {shape} lds +{spad} hi")
    _assert_bits(_bits_of(lh), exp[1], f"mode 3 {shape} lds +{spad} lo")
    holders = [_guarded_bf16(numel, device) for _ in range(3)]
    _check(_lib().ps_convert_f32_to_bf16x3_frag(_stream(), src.data_ptr(), holders[0][1].data_ptr(),
                                                holders[1][1].data_ptr(), holders[2][1].data_ptr(), r, c,
                                                int(src.stride(0))), "ps_convert_f32_to_bf16x3_frag")
    got = [_bits_of(h[0]) for h in holders]
    for pl in range(3):
      _assert_bits(got[pl], exp[pl], f"x3_frag {shape} lds +{spad} plane {pl}")
    # x3_frag's hi and lo are mode 3's, bit for bit (NaN payloads included)
    _assert_equal(got[0], _bits_of(hh), "x3_frag p0 vs mode 3 hi")
    _assert_equal(got[1], _bits_of(lh), "x3_frag p1 vs mode 3 lo")
  hi_only_h, hi_only = _guarded_bf16(numel, device)
  _convert(_src_view(x, 0, device), hi_only, None, r, c, c, 3)
  _assert_bits(_bits_of(hi_only_h), exp[0], f"mode 3 {shape} hi alone")


# ---------------------------------------------------------------------------
# 2. ps_gemm_bf16_grouped, non-symmetric
# ---------------------------------------------------------------------------
def _operands(ap, bp, sa, sb, dev, pads=(8, 16)):
  a = tuple(_plane_view(ap[i], pads[0], dev) if i < sa else None for i in range(2))
  b = tuple(_plane_view(bp[i], pads[1], dev) if i < sb else None for i in range(2))
  return a, b


def _run_product(cases, dev):
  """cases: list of (ap, bp, (sa, sb), exp) -> runs them in ONE call, checks every output."""
  items, outs = [], []
  for (ap, bp, (sa, sb), exp) in cases:
    a, b = _operands(ap, bp, sa, sb, dev)
    holder, view = _framed(exp.shape[0], exp.shape[1], dev)
    items.append((a, b, view))
    outs.append((holder, exp))
  K().gemm_bf16_grouped(items)
  for t, (holder, exp) in enumerate(outs):
    _check_framed(holder, exp, f"task {t} of {len(outs)} {cases[t][2]} {exp.shape}")
  return [h[1:e.shape[0] + 1, 2:e.shape[1] + 2].clone() for (h, e) in outs]


@pytest.mark.parametrize("k", F.GEMM_K_UNSPLIT + F.GEMM_K_SPLIT)
@pytest.mark.parametrize("mn", F.GEMM_MN)
def test_gemm_bf16_exact(device, mn, k):
  m, n = mn
  a, bt, ap, bp, exp = F.product_case(m, n, k, 0, *F.product_scales(m, n, k))
  # all four (A split, B split) instances in one call, then each alone
  _run_product([(ap, bp, s, exp[s]) for s in F.SPLITS], device)
  for s in F.SPLITS:
    _run_product([(ap, bp, s, exp[s])], device)


@pytest.mark.parametrize("mnk", F.GEMM_TILED)
def test_gemm_bf16_tile_blocked_left_operand(device, mnk):
  m, n, k = mnk
  a, bt, ap, bp, exp = F.product_case(m, n, k, 2)
  numel, idx = F.tiled_numel(m, k), F.idx_tiled(m, k).ravel()
  planes = []
  for p in ap:
    bits = np.zeros(numel, np.uint16)          # rows past m are zero
    bits[idx] = F.bf16_bits(p).ravel()
    planes.append(_to_bf16_tensor(bits, device))
  for (sa, sb) in F.SPLITS:
    tiled = K().TiledBf16(planes[0], planes[1] if sa == 2 else None, m, k)
    _, b = _operands(ap, bp, sa, sb, device)
    holder, view = _framed(m, n, device)
    K().gemm_bf16_grouped([(tiled, b, view)])
    _check_framed(holder, exp[(sa, sb)], f"a_tiled {mnk} {(sa, sb)}")
    plain = _run_product([(ap, bp, (sa, sb), exp[(sa, sb)])], device)[0]
    assert torch.equal(view, plain), "tile-blocked and plain layouts differ"
  # the conversion writes the same planes
  conv = K().to_bf16(torch.from_numpy(a).to(device), split=True, tiled=True)
  _assert_equal(_bits_of(conv.hi), _bits_of(planes[0]), "to_bf16(tiled) hi")
  _assert_equal(_bits_of(conv.lo), _bits_of(planes[1]), "to_bf16(tiled) lo")


def test_gemm_bf16_mixed_split_and_unsplit(device):
  cases = []
  for (m, n, k, s) in F.GEMM_MIXED:
    _, _, ap, bp, exp = F.product_case(m, n, k, 4)
    cases.append((ap, bp, s, exp[s]))
  together = _run_product(cases, device)
  for case, got in zip(cases, together):
    alone = _run_product([case], device)[0]
    assert torch.equal(got, alone), f"task {case[2]} {case[3].shape} differs from its single-task result"


# ---------------------------------------------------------------------------
# 3. symmetric = 1
# ---------------------------------------------------------------------------
def _run_symmetric(cases, dev):
  """cases: list of (planes, sa, exp) -> one symmetric call; every result equals the reference
  and its own transpose."""
  items, outs = [], []
  for (ap, sa, exp) in cases:
    a = tuple(_plane_view(ap[i], 8, dev) if i < sa else None for i in range(2))
    holder, view = _framed(exp.shape[0], exp.shape[0], dev)
    items.append((a, a, view))
    outs.append((holder, view, exp))
  K().gemm_bf16_grouped(items, symmetric=True)
  for t, (holder, view, exp) in enumerate(outs):
    _check_framed(holder, exp, f"symmetric task {t} m = {exp.shape[0]} planes {cases[t][1]}")
    assert torch.equal(view, view.t()), "result is not bitwise symmetric"
  return [v.clone() for (_, v, _) in outs]


@pytest.mark.parametrize("mk", F.SYM_CASES)
def test_gemm_bf16_symmetric_exact(device, mk):
  m, k = mk
  _, ap, exp = F.sym_case(m, k, 1)
  for sa in ((2,) if m > 1024 else (2, 1)):
    _run_symmetric([(ap, sa, exp[sa])], device)


def test_gemm_bf16_symmetric_two_products_in_one_call(device):
  cases = []
  for (m, k) in F.SYM_PAIR:
    _, ap, exp = F.sym_case(m, k, 1)
    cases.append((ap, 2, exp[2]))
  together = _run_symmetric(cases, device)
  for case, got in zip(cases, together):
    assert torch.equal(got, _run_symmetric([case], device)[0])


# ---------------------------------------------------------------------------
# 4. ps_fd_cy_step_f32
# ---------------------------------------------------------------------------
def _dev(x, dev):
  return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


@pytest.mark.parametrize("step", F.CY_STEPS)
@pytest.mark.parametrize("shape", F.FUSED_SHAPES)
def test_fd_cy_step_exact(device, shape, step):
  bt, n, b = shape
  case = F.cy_case(bt, n, b, step)
  c16 = [K().to_bf16(_dev(case["c"][j], device), split=True, tiled="frag") for j in range(bt)]
  for j in range(bt):   # the covariance planes are the restated ones at the restated positions
    cp = F.bf16_split(case["c"][j], 2)
    idx = F.idx_frag_left(n, n).ravel()
    for got, p in ((c16[j].hi, cp[0]), (c16[j].lo, cp[1])):
      e = np.empty(n * n, np.uint16)
      e[idx] = F.bf16_bits(p).ravel()
      _assert_equal(_bits_of(got), e, f"covariance planes of factor {j}")
  yp = F.bf16_split(case["y"], 2)
  yt = tuple(_to_bf16_tensor(F.place_iter_frag(p), device) for p in yp)
  oh, y_next = _guarded_f32((bt, n, b), device)
  holders = [_guarded_bf16(bt * n * b, device) for _ in range(2)]
  K().fd_cy_step(c16, yt, _dev(case["y"], device), _dev(case["y_prev"], device), y_next,
                 (holders[0][1], holders[1][1]), _dev(case["params"], device), step)
  _assert_equal(y_next.cpu().numpy().astype(np.float64), case["exp"], f"y_next {shape} step {step}")
  _assert_guards_f32(oh, "fd_cy_step")
  if bt > 1:
    assert step > case["deg"][1] and torch.equal(y_next[1], _dev(case["y"][1], device)), "finished factor keeps y"
  # the written planes: the restated split of the expected y_next at the restated positions
  np_planes = F.bf16_split(case["exp"].astype(np.float32), 2)
  for (holder, _), p, name in zip(holders, np_planes, ("nt_hi", "nt_lo")):
    _assert_guards_bf16(holder, name)
    _assert_equal(_bits_of(holder)[GUARD:-GUARD], F.place_iter_frag(p), f"{name} {shape} step {step}")
  # without output planes the iterate is the same
  oh2, y2 = _guarded_f32((bt, n, b), device)
  K().fd_cy_step(c16, yt, _dev(case["y"], device), _dev(case["y_prev"], device), y2, None,
                 _dev(case["params"], device), step)
  assert torch.equal(y2, y_next)
  _assert_guards_f32(oh2, "fd_cy_step without planes")


# ---------------------------------------------------------------------------
# 5. ps_fd_cx6_f32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", F.FUSED_SHAPES)
def test_fd_cx6_exact(device, shape):
  bt, n, b = shape
  case = F.cx6_case(bt, n, b)
  c16 = [K().to_bf16(_dev(case["c"][j], device), split=True, tiled="frag3") for j in range(bt)]
  oh, z = _guarded_f32((bt, n, b), device)
  holders = [_guarded_bf16(bt * n * b, device) for _ in range(3)]
  K().fd_cx6(c16, _dev(case["x"], device), z, scratch=[h[1] for h in holders])
  _assert_equal(z.cpu().numpy().astype(np.float64), case["exp"], f"z {shape}")
  _assert_guards_f32(oh, "fd_cx6")
  for (holder, _), p, name in zip(holders, F.bf16_split(case["x"], 3), ("xt0", "xt1", "xt2")):
    _assert_guards_bf16(holder, name)
    _assert_equal(_bits_of(holder)[GUARD:-GUARD], F.place_iter_frag(p), f"{name} {shape}")


# ---------------------------------------------------------------------------
# 6. ps_fd_filter_step_f32
# ---------------------------------------------------------------------------
def _filter_step(case, step, dev, planes, ldt):
  """planes: 0 none, 1 hi only, 2 hi and lo.  Returns (y_next host array, hi bits, lo bits)."""
  bt, n, b = case["y"].shape
  numel = bt * n * b
  oh, y_next = _guarded_f32((bt, n, b), dev)
  hh, hi = _guarded_bf16(numel, dev)
  lh, lo = _guarded_bf16(numel, dev)
  z, y, yp, prm = (_dev(case[name], dev) for name in ("z", "y", "y_prev", "params"))
  _check(_lib().ps_fd_filter_step_f32(
      _stream(), z.data_ptr(), y.data_ptr(), yp.data_ptr() if step > 1 else None, y_next.data_ptr(),
      hi.data_ptr() if planes >= 1 else None, lo.data_ptr() if planes >= 2 else None, prm.data_ptr(),
      step, bt, n, b, ldt), "ps_fd_filter_step_f32")
  _assert_guards_f32(oh, "fd_filter_step")
  return y_next.cpu().numpy(), _bits_of(hh), _bits_of(lh)


def _expected_iter_planes(values, idx, numel):
  out = []
  for p in F.bf16_split(values.astype(np.float32), 2):
    e = np.full(numel + 2 * GUARD, F.BF16_SENT, np.uint16)
    e[GUARD + idx.ravel()] = F.bf16_bits(p).ravel()
    out.append(e)
  return out


@pytest.mark.parametrize("step", F.FILTER_DYADIC_STEPS)
@pytest.mark.parametrize("shape", F.FILTER_DYADIC)
def test_fd_filter_step_dyadic_exact(device, shape, step):
  bt, n, b = shape
  case = F.filter_dyadic_case(bt, n, b, step)
  numel = bt * n * b
  untouched = np.full(numel + 2 * GUARD, F.BF16_SENT, np.uint16)
  layouts = [(bt * n, F.idx_iter_transposed(bt, n, b, bt * n))]
  if n % 64 == 0 and b % 32 == 0:
    layouts.append((0, F.idx_iter_frag(bt, n, b)))
  for (ldt, idx) in layouts:
    exp_planes = _expected_iter_planes(case["exp"], idx, numel)
    for planes in (2, 1, 0):
      got, hi, lo = _filter_step(case, step, device, planes, ldt)
      what = f"{shape} step {step} ldt {ldt} planes {planes}"
      _assert_equal(got.astype(np.float64), case["exp"], "y_next " + what)
      _assert_equal(hi, exp_planes[0] if planes >= 1 else untouched, "yt_hi " + what)
      _assert_equal(lo, exp_planes[1] if planes >= 2 else untouched, "yt_lo " + what)
  if step > 1 and bt > 1:
    assert np.array_equal(case["exp"][1], case["y"][1])   # the finished factor kept y
  # the wrapper returns the same planes
  z, y, yp, prm = (_dev(case[name], device) for name in ("z", "y", "y_prev", "params"))
  oh, out = _guarded_f32((bt, n, b), device)
  hi, lo = K().fd_filter_step(z, y, yp if step > 1 else None, out, prm, step)
  _assert_equal(out.cpu().numpy().astype(np.float64), case["exp"], "wrapper y_next")
  _assert_guards_f32(oh, "fd_filter_step wrapper")
  exp_planes = _expected_iter_planes(case["exp"], F.idx_iter_transposed(bt, n, b, bt * n), numel)
  _assert_equal(_bits_of(hi), exp_planes[0][GUARD:-GUARD], "wrapper yt_hi")
  _assert_equal(_bits_of(lo), exp_planes[1][GUARD:-GUARD], "wrapper yt_lo")


@pytest.mark.parametrize("step", F.FILTER_GENERAL_STEPS)
@pytest.mark.parametrize("shape", F.FILTER_GENERAL)
def test_fd_filter_step_general_parameters(device, shape, step):
  """|got - ref| <= F u magnitude against the float64 restatement, F = _fd_exact.filter_factor(step)
  (derived there from the kernel's operation count); the planes are the restated split of the
  iterate the kernel itself wrote."""
  bt, n, b = shape
  case = F.filter_general_case(bt, n, b)
  ref, mag = F.filter_step_ref64(case["z"], case["y"], case["y_prev"], case["params"], step)
  got, hi, lo = _filter_step(case, step, device, 2, bt * n)
  ratio = E.bound_ratio(got, ref, mag, F.filter_factor(step))
  print(f"filter step {shape} step {step}: max error / bound = {ratio:.4f}")
  assert ratio <= 1.0, (shape, step, ratio)
  for j in range(bt):
    if step > case["params"][j, 3]:
      _assert_equal(got[j], case["y"][j], f"finished factor {j} keeps y")
  exp_planes = _expected_iter_planes(got, F.idx_iter_transposed(bt, n, b, bt * n), bt * n * b)
  _assert_equal(hi, exp_planes[0], "yt_hi")
  _assert_equal(lo, exp_planes[1], "yt_lo")


# ---------------------------------------------------------------------------
# 7. ps_fd_cov_update_f32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("decay", F.COV_DECAYS)
@pytest.mark.parametrize("shape", F.COV_SHAPES)
def test_fd_cov_update_exact(device, shape, decay):
  bt, n = shape
  c, g, exp = F.cov_case(bt, n, decay)
  holder, cd = _guarded_f32((bt, n, n), device)
  cd.copy_(_dev(c, device))
  grams = [_dev(g[j], device) for j in range(bt)]
  out = K().fd_cov_update(cd, grams, decay)
  assert out.data_ptr() == cd.data_ptr()
  _assert_equal(cd.cpu().numpy().astype(np.float64), exp, f"cov update {shape} decay {decay}")
  assert torch.equal(cd, cd.transpose(1, 2)), "result is not bitwise symmetric"
  _assert_guards_f32(holder, "fd_cov_update")
  for j in range(bt):
    assert torch.equal(grams[j], _dev(g[j], device)), "a Gram matrix was written"
