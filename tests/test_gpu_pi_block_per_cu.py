"""The one-workgroup resident power iteration (pi_block_kernel, power_iter.hip.h): blocks of up to
4 x 4 tiles (n <= 512) are iterated by ONE workgroup each, off-diagonal tiles in registers and
diagonal tiles as packed upper triangles in LDS.  Its arithmetic is the streaming kernels' term for
term, so eigenvalues, step counts, roots and metrics must equal the streaming execution's bit for
bit -- for odd sizes, padded blocks, a block that is not symmetric (its tiles are read from memory),
more blocks than CUs and calls that mix small blocks with team blocks (n > 512)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STREAMING = {"power_iteration": "streaming"}


def K():
  from precondition_amd import kernels
  return kernels


def L():
  from precondition_amd import _lib
  return _lib.lib()


def health():
  e, c, r = C.c_uint(), C.c_int(), C.c_int()
  assert L().ps_power_iteration_health(C.addressof(e), C.addressof(c), C.addressof(r)) == 0
  return e.value, c.value, r.value


@pytest.fixture
def resident():
  L().ps_power_iteration_reset_health()
  assert health() == (0, 0, 1)
  yield
  assert health()[0] == 0


def spd(n, seed, device, dominant=False):
  gen = torch.Generator(device=device).manual_seed(seed)
  g = torch.randn((n, 2 * n), generator=gen, device=device)
  a = g @ g.T
  if dominant:   # a dominant eigenvalue: the loop stops early (DS:639)
    a = a + 50.0 * torch.ones((n, n), device=device)
  return (0.5 * (a + a.T)).contiguous()


def both(mats, **kw):
  lam, its = K().power_iteration_batched(mats, **kw)
  lam_s, its_s = K().power_iteration_batched(mats, options=STREAMING, **kw)
  torch.cuda.synchronize()
  lam, its, lam_s, its_s = (x.cpu().numpy() for x in (lam, its, lam_s, its_s))
  assert np.array_equal(lam, lam_s, equal_nan=True), np.flatnonzero(lam != lam_s)
  assert np.array_equal(its, its_s)
  return lam, its


def test_sizes_and_padding_bit_identical_to_streaming(device, resident):
  sizes = [1, 100, 128, 129, 300, 384, 511, 512]
  mats = [spd(n, 10 + i, device, dominant=(i % 3 == 0)) for i, n in enumerate(sizes)]
  lam, its = both(mats)
  assert np.isfinite(lam).all() and its.max() == 100 and its.min() < 100
  # padding_start below n: only the leading part of the block is iterated
  pads = [1, 64, 128, 100, 257, 384, 300, 0]
  lam_p, _ = both(mats, padding_starts=pads)
  assert np.isnan(lam_p[-1]) and np.isfinite(lam_p[:-1]).all()
  for i in (2, 5):   # padding_start = n or a whole-tile boundary of a smaller block
    ref, _ = K().power_iteration_batched([mats[i][:pads[i], :pads[i]].contiguous()])
    assert np.isclose(lam_p[i], ref.item(), rtol=1e-5)


def test_one_non_symmetric_block_among_symmetric_ones(device, resident):
  gen = torch.Generator(device=device).manual_seed(3)
  mats = [spd(n, 20 + i, device) for i, n in enumerate([512, 300, 512, 129])]
  mats[2] = (mats[2] + 0.01 * torch.randn((512, 512), generator=gen, device=device)).contiguous()
  mats[3] = (mats[3] + 0.01 * torch.randn((129, 129), generator=gen, device=device)).contiguous()
  both(mats)
  both(mats, padding_starts=[512, 300, 500, 129])


def test_more_blocks_than_cus(device, resident):
  mats = torch.stack([spd(512, 1000 + i, device, dominant=(i % 7 == 0)) for i in range(300)])
  lam, its = both(list(mats.unbind(0)))
  assert its.min() < 100 and its.max() == 100


def test_mixed_small_and_team_blocks(device, resident):
  sizes = [512, 1024, 300, 1024, 512, 640, 128, 2048]
  mats = [spd(n, 40 + i, device) for i, n in enumerate(sizes)]
  both(mats)
  both(mats, padding_starts=[512, 1000, 300, 512, 0, 640, 100, 2048])


def test_inverse_pth_root_bit_identical_to_streaming(device, resident):
  sizes = [512, 300, 512, 1024, 129, 512]
  mats = [spd(n, 70 + i, device) for i, n in enumerate(sizes)]
  ps = [4, 2, 4, 4, 8, 4]
  roots, met = K().matrix_inverse_pth_root_batched(mats, ps)
  roots_s, met_s = K().matrix_inverse_pth_root_batched(mats, ps, options=STREAMING)
  torch.cuda.synchronize()
  assert torch.equal(met.cpu(), met_s.cpu())
  for r, r_s in zip(roots, roots_s):
    assert torch.equal(r, r_s)
  assert torch.isfinite(met[:, :5]).all()
