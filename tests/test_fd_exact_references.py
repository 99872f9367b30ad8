"""CPU checks of tests/_fd_exact.py, the helper of test_gpu_fd_exact.py: the bf16 restatement
against torch's CPU conversion, the layout maps, the plan restatements and the coverage
conditions of the committed case lists, and the exactness precondition of EVERY GPU case (so
the case lists stay honest without a GPU)."""
import numpy as np
import pytest
import torch

from tests import _exact as E
from tests import _fd_exact as F


def _torch_bits(x):
  t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16)
  return t.view(torch.int16).numpy().view(np.uint16)


def _assert_bits(got, exp):
  nan = F.is_nan_bits(exp)
  assert np.array_equal(F.is_nan_bits(got), nan)
  assert np.array_equal(np.where(nan, 0, got), np.where(nan, 0, exp))


def test_bf16_rne_special_values():
  x = F.special_values()
  got = F.bf16_bits(x)
  _assert_bits(got, _torch_bits(x))
  by = dict(zip(F.SPECIAL_BITS.tolist(), got.tolist()))
  assert by[0x3f808000] == 0x3f80 and by[0x3f818000] == 0x3f82      # ties to even
  assert by[0x3f807fff] == 0x3f80 and by[0x3f808001] == 0x3f81
  assert by[0x3f817fff] == 0x3f81 and by[0x3f818001] == 0x3f82
  assert by[0x00000000] == 0x0000 and by[0x80000000] == 0x8000
  assert by[0x7f800000] == 0x7f80 and by[0xff800000] == 0xff80
  assert by[0x7f7f0000] == 0x7f7f and by[0x7f7f7fff] == 0x7f7f
  assert by[0x7f7f8000] == 0x7f80 and by[0x7f7fffff] == 0x7f80 and by[0xff7f8000] == 0xff80
  assert F.is_nan_bits(got[[12, 13, 14]]).all()


def test_bf16_rne_matches_torch_on_test_inputs():
  rng = np.random.default_rng(5)
  x = rng.standard_normal(1 << 16).astype(np.float32) * np.exp2(rng.integers(-60, 60, 1 << 16)).astype(np.float32)
  _assert_bits(F.bf16_bits(x), _torch_bits(x))
  for shape in F.CONVERT_PLAIN + F.CONVERT_TILED + F.CONVERT_FRAG:
    x = F.convert_input(*shape)
    _assert_bits(F.bf16_bits(x), _torch_bits(x))
    with np.errstate(all="ignore"):
      hi = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
      lo = torch.from_numpy((x - hi).astype(np.float32)).to(torch.bfloat16)
    planes = F.bf16_split(x, 2)
    _assert_bits(F.bf16_bits(planes[1]), lo.view(torch.int16).numpy().view(np.uint16))
  # every integer up to 2^16 exactly, as a spot check of the whole low range
  ints = np.arange(-65536, 65537, dtype=np.float32)
  _assert_bits(F.bf16_bits(ints), _torch_bits(ints))


def test_bf16_split_reconstructs_wide_integers():
  two = np.arange(-65535, 65536, dtype=np.int64)
  hi, lo = F.bf16_split(two.astype(np.float32), 2)
  assert np.array_equal(hi.astype(np.int64) + lo.astype(np.int64), two)
  rng = np.random.default_rng(6)
  three = np.concatenate([rng.integers(-(1 << 24) + 1, 1 << 24, 200000), [65793, 65792, 131329, (1 << 24) - 1]])
  p = F.bf16_split(three.astype(np.float32), 3)
  assert np.array_equal(sum(q.astype(np.int64) for q in p), three)
  assert [int(q[-4]) for q in p] == [66048, -255, 0]         # 65793 = 0x10101: above the half, rounds up
  assert [int(q[-3]) for q in p] == [65536, 256, 0]          # 65792: a tie, to the even mantissa
  assert [int(q[-2]) for q in p] == [131072, 256, 1]         # 131329: a tie in the SECOND plane, three planes
  h, l = F.bf16_split(np.array([257], np.float32), 2)
  assert (int(h[0]), int(l[0])) == (256, 1)
  # every plane is a bf16 value
  for q in p:
    assert np.array_equal(F.bf16_rne(q), q)
  # the builders' wide entries need the planes they are meant to need
  w = F.wide(64, 64, 3, 1)
  assert np.any(F.bf16_split(w.astype(np.float32), 2)[1] != 0)
  w3 = F.wide(64, 64, 3, 1, 131073, 262143)
  assert np.any(F.bf16_split(w3.astype(np.float32), 3)[2] != 0)
  m = F.medium(64, 64, 3, 4095)
  big = np.abs(m) > 8
  assert big.any() and np.all(np.abs(m[big]) >= 257) and np.all(np.abs(m[big]) <= 4095)


def _is_permutation(idx, size):
  flat = np.sort(np.asarray(idx).ravel())
  return flat.size == size and np.array_equal(flat, np.arange(size))


def test_index_maps():
  for (r, c) in F.CONVERT_PLAIN:
    assert _is_permutation(F.idx_plain(r, c, c), r * c)
    assert _is_permutation(F.idx_transposed(r, c, r), r * c)
    ld = c + 5
    ip = F.idx_plain(r, c, ld)
    assert len(np.unique(ip)) == r * c and ip.max() == (r - 1) * ld + c - 1
    assert np.array_equal(F.idx_transposed(r, c, r + 3), F.idx_plain(c, r, r + 3).T)
  for (r, c) in F.CONVERT_TILED + [(256, 64)]:
    it = F.idx_tiled(r, c).ravel()
    total = F.tiled_numel(r, c)
    assert len(np.unique(it)) == r * c and it.min() >= 0 and it.max() < total
    if r % 128 == 0:
      assert _is_permutation(it, total)
    else:
      # an injection whose complement is exactly the zero padding: the rows past `rows`
      full = F.idx_tiled((r + 127) // 128 * 128, c)
      assert _is_permutation(full, total)
      assert np.array_equal(full[:r], F.idx_tiled(r, c))
      assert np.array_equal(np.sort(np.setdiff1d(np.arange(total), it)), np.sort(full[r:].ravel()))
  for (r, c) in F.CONVERT_FRAG:
    assert _is_permutation(F.idx_frag_left(r, c), r * c)
  for (bt, n, b) in F.FUSED_SHAPES + [(3, 128, 96)]:
    assert _is_permutation(F.idx_frag_iter(n, b), n * b)
    assert _is_permutation(F.idx_iter_frag(bt, n, b), bt * n * b)
  for (bt, n, b) in F.FILTER_DYADIC:
    assert _is_permutation(F.idx_iter_transposed(bt, n, b, bt * n), bt * n * b)
  # one 16-byte fragment of the left operand is 8 consecutive k of one row; of the iterate, 8
  # consecutive rows (k) of one column
  il = F.idx_frag_left(64, 64)
  assert np.array_equal(il[5, 8:16], il[5, 8] + np.arange(8)) and il[0, 0] == 0 and il[32, 0] == 512
  ii = F.idx_frag_iter(64, 32)
  assert np.array_equal(ii[8:16, 7], ii[8, 7] + np.arange(8)) and ii[16, 0] == 512


def test_plans_and_case_lists():
  plans, sp = F.check_fd_lists()
  assert F.hsplit_for(512, 8192) == 1 and F.hsplit_for(511, 1023) == 1
  assert F.hsplit_for(1, 8192) == 16 and F.hsplit_for(256, 8192) == 2 and F.hsplit_for(100, 1536) == 3
  assert F.hsplit_plan(6, 1024) == (2, 512, 512)
  assert F.fd_half_blocks(16, 512) and not F.fd_half_blocks(16, 640) and F.fd_half_blocks(2, 4096)
  assert not F.fd_half_blocks(3, 4096)
  with pytest.raises(AssertionError):     # without the 4096 case no product is cut in the tail round only
    F.check_fd_lists(sym_cases=[c for c in F.SYM_CASES if c != (4096, 160)])
  with pytest.raises(AssertionError):     # without the last shape only the 32-row form runs
    F.check_fd_lists(fused_shapes=F.FUSED_SHAPES[:-1])
  with pytest.raises(AssertionError):     # without k = 1568 no split count 3
    F.check_fd_lists(k_split=[k for k in F.GEMM_K_SPLIT if k != 1568])


def test_exactness_of_the_product_cases():
  for (m, n) in F.GEMM_MN:
    for k in F.GEMM_K_UNSPLIT + F.GEMM_K_SPLIT:
      sa, sb = F.product_scales(m, n, k)
      a, bt, ap, bp, exp = F.product_case(m, n, k, 0, sa, sb)     # asserts the precondition
      assert np.array_equal(ap[0] + ap[1], a) and np.array_equal(bp[0] + bp[1], bt)
      if m * n >= 128 * 96 and k >= 160:
        # the cross terms and the dropped lo lo term are all present: each would change the result
        lolo = F.planes_product(ap, bp, [(1, 1)])
        assert np.any(lolo != 0) and np.any(F.planes_product(ap, bp, [(1, 0)]) != 0)
        assert np.any(F.planes_product(ap, bp, [(0, 1)]) != 0)
        assert not np.array_equal(exp[(2, 2)], exp[(2, 1)]) and not np.array_equal(exp[(2, 2)], exp[(1, 2)])
  scaled = [F.product_scales(m, n, k) for (m, n) in F.GEMM_MN for k in F.GEMM_K_UNSPLIT + F.GEMM_K_SPLIT]
  assert any(s[0] != 1.0 for s in scaled) and any(s[1] != 1.0 for s in scaled) and (1.0, 1.0) in scaled
  for (m, n, k) in F.GEMM_TILED:
    F.product_case(m, n, k, 2)
  for (m, n, k, _) in F.GEMM_MIXED:
    F.product_case(m, n, k, 4)


def test_exactness_of_the_symmetric_cases():
  for (m, k) in F.SYM_CASES:
    a, ap, exp = F.sym_case(m, k, 1)
    assert all(np.array_equal(e, e.T) for e in exp.values())
    if m <= 257:
      assert not np.array_equal(exp[2], exp[1])
      assert np.any(F.planes_product(ap, ap, [(1, 1)]) != 0)


def test_exactness_of_the_fused_cases():
  for (bt, n, b) in F.FUSED_SHAPES:
    for step in F.CY_STEPS:
      case = F.cy_case(bt, n, b, step)
      assert np.array_equal(case["exp"], np.round(case["exp"]))
      if bt > 1:
        assert np.array_equal(case["exp"][1], case["y"][1])
      assert not np.array_equal(case["c"][0], case["c"][0].T)
    F.cx6_case(bt, n, b)
  for (bt, n, b) in F.FILTER_DYADIC:
    for step in F.FILTER_DYADIC_STEPS:
      F.filter_dyadic_case(bt, n, b, step)
  for (bt, n) in F.COV_SHAPES:
    for decay in F.COV_DECAYS:
      F.cov_case(bt, n, decay)


def test_sigma_recurrence_is_one_for_sigma1_one():
  for step in range(1, 40):
    sigma, sn = F.sigma_chain32(1.0, step)
    assert sigma == np.float32(1) and sn == np.float32(1)
  assert F.dyadic_coefficients(1) == (4.0, 0.0) and F.dyadic_coefficients(7) == (8.0, 1.0)
  # the restatement agrees with the dyadic closed form, exactly
  case = F.filter_dyadic_case(3, 200, 40, 7)
  val, _ = F.filter_step_ref64(case["z"], case["y"], case["y_prev"], case["params"], 7)
  assert np.array_equal(val, case["exp"])


def test_filter_restatement_against_float32():
  for (bt, n, b) in F.FILTER_GENERAL:
    case = F.filter_general_case(bt, n, b)
    degs = case["params"][:, 3]
    assert len(set(degs.tolist())) == bt
    for step in F.FILTER_GENERAL_STEPS + [30]:
      ref, mag = F.filter_step_ref64(case["z"], case["y"], case["y_prev"], case["params"], step)
      got = F.filter_step_f32(case["z"], case["y"], case["y_prev"], case["params"], step)
      ratio = E.bound_ratio(got, ref, mag, F.filter_factor(step))
      assert ratio <= 1.0, (n, b, step, ratio)
      for j in range(bt):
        if step > degs[j]:
          assert np.array_equal(got[j], case["y"][j])
  assert any(step > d for step in F.FILTER_GENERAL_STEPS for d in F.control_rows(3)[:, 3])
