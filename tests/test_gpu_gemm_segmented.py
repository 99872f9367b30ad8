"""ps_gemm_grouped_seg_typed: grouped products whose rows are segmented (the three contractions of
a rank-3 block addressed in place, DS:1689-1708), called directly on a parent buffer [A, B, C].

Without split-K (every k < 512) a segmented product sums each element's products in the k order of
ps_gemm_grouped_typed, so it must equal that entry on a contiguous copy of the same operands BIT
FOR BIT.  The split-K case is held to the float64 bound of a float32 sum of k + 2 terms.  Every
case checks that nothing outside the addressed block was written."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PS_EUNSUPPORTED = -3
SENTINEL = -12345.5


def _mods():
  from precondition_amd import _lib, kernels
  return _lib, kernels, _lib.lib()


def _call(tbl, a_dt=0, b_dt=0):
  """One grouped call on a descriptor table of either dtype; returns the library's code."""
  L, K, lib = _mods()
  seg = tbl.dtype == K._GSEGDESC_DT
  descs = C.cast(tbl.ctypes.data, C.POINTER(L.GemmSegDesc if seg else L.GemmDesc))
  nbytes = (lib.ps_gemm_grouped_seg_workspace_bytes if seg else lib.ps_gemm_grouped_workspace_bytes)(
      descs, len(tbl))
  ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda:0")
  fn = lib.ps_gemm_grouped_seg_typed if seg else lib.ps_gemm_grouped_typed
  rc = fn(torch.cuda.current_stream().cuda_stream, descs, len(tbl), a_dt, b_dt, ws.data_ptr(), ws.numel())
  torch.cuda.synchronize()
  return rc


def _row(tbl, i, a, b, c, m, n, k, lda, ldb, ldc, transa=1, transb=0, m_seg=0, a_ss=0, c_ss=0):
  r = tbl[i]
  r["a"], r["b"], r["c"] = a, b, c
  r["m"], r["n"], r["k"], r["lda"], r["ldb"], r["ldc"] = m, n, k, lda, ldb, ldc
  r["transa"], r["transb"] = transa, transb
  if "m_seg" in tbl.dtype.names:
    r["m_seg"], r["a_seg_stride"], r["c_seg_stride"] = m_seg, a_ss, c_ss


def _addr(t, *index):
  """Address of element t[index] of a contiguous tensor."""
  off = sum(int(i) * int(s) for i, s in zip(index, t.stride()))
  return t.data_ptr() + off * t.element_size()


class _Stage1:
  """X1[(b c), a'] = G[a, (b c)]^T P for a block [a_n, nseg, m_seg] at (a0, b0, c0) of a parent
  [A, B, C]: operand A in place (nseg segments of m_seg rows, C apart), X1 dense inside a guarded buffer."""

  def __init__(self, rng, a_n, nseg, m_seg, c_full, c0, dtype=torch.float32):
    self.a_n, self.nseg, self.m_seg = a_n, nseg, m_seg
    self.lo = (1, 1, c0)
    shape = (a_n + 2, nseg + 2, c_full)
    assert c0 + m_seg <= c_full
    host = rng.standard_normal(shape).astype(np.float32)
    self.parent = torch.tensor(host, device="cuda:0").to(dtype)
    self.parent_before = self.parent.clone()
    self.P = torch.tensor(rng.standard_normal((a_n, a_n)).astype(np.float32), device="cuda:0")
    self.m = nseg * m_seg
    self.guard = 7
    self.out = torch.full((self.m * a_n + 2 * self.guard,), SENTINEL, device="cuda:0")
    self.out_ref = torch.full((self.m, a_n), SENTINEL, device="cuda:0")
    a0, b0, _ = self.lo
    self.block = self.parent[a0:a0 + a_n, b0:b0 + nseg, c0:c0 + m_seg]
    self.copy = self.block.reshape(a_n, self.m).contiguous()

  def seg_row(self, tbl, i):
    A, B, Cf = self.parent.shape
    _row(tbl, i, _addr(self.parent, *self.lo), self.P.data_ptr(), _addr(self.out, self.guard),
         self.m, self.a_n, self.a_n, B * Cf, self.a_n, self.a_n,
         m_seg=self.m_seg, a_ss=Cf, c_ss=self.m_seg * self.a_n)

  def plain_row(self, tbl, i):
    _row(tbl, i, self.copy.data_ptr(), self.P.data_ptr(), self.out_ref.data_ptr(),
         self.m, self.a_n, self.a_n, self.m, self.a_n, self.a_n)

  def check(self):
    g = self.guard
    assert torch.equal(self.parent, self.parent_before)
    assert bool((self.out[:g] == SENTINEL).all()) and bool((self.out[-g:] == SENTINEL).all())
    got = self.out[g:-g].reshape(self.m, self.a_n)
    assert not bool((self.out_ref == SENTINEL).any())
    assert torch.equal(got, self.out_ref), (self.a_n, self.nseg, self.m_seg)


@pytest.mark.parametrize("a_n", [5, 64, 130])
@pytest.mark.parametrize("aligned", [False, True], ids=["C_odd", "C_mult4"])
def test_stage1_segmented_operand_bit_identical_to_the_contiguous_copy(device, a_n, aligned):
  """m_seg in {3, 64, 128, 200} x nseg in {1, 2, 5}, one grouped call: a block at a non-zero offset
  of a parent whose last axis is odd (unaligned segments: the guarded loads) or a multiple of 4 with
  the block starting on a 16-byte boundary (the vector loads)."""
  L, K, lib = _mods()
  rng = np.random.default_rng(100 + a_n + int(aligned))
  cases = []
  for m_seg in (3, 64, 128, 200):
    for nseg in (1, 2, 5):
      if aligned:
        c_full, c0 = (m_seg + 3) // 4 * 4 + 8, 4
        # (a_n + 2, nseg + 2, c_full) row-major: the block's first element is 16-byte aligned when
        # its element offset is a multiple of 4
        assert ((1 * (nseg + 2) + 1) * c_full + c0) % 4 == 0
      else:
        c_full, c0 = (m_seg + 5) | 1, 3
      cases.append(_Stage1(rng, a_n, nseg, m_seg, c_full, c0))
  seg = np.zeros(len(cases), K._GSEGDESC_DT)
  plain = np.zeros(len(cases), K._GDESC_DT)
  for i, cs in enumerate(cases):
    cs.seg_row(seg, i)
    cs.plain_row(plain, i)
  assert _call(plain) == 0
  assert _call(seg) == 0
  for cs in cases:
    cs.check()


class _Stage3:
  """Y[(a' b'), c'] = X2[c, (a' b')]^T P written into a block [a_n, b_n, c_n] at (a0, b0, c0) of a
  parent [A, B, C]: a_n segments of b_n rows, B*C apart, ldc = C."""

  def __init__(self, rng, a_n, b_n, c_n, shape, lo):
    self.dims, self.lo = (a_n, b_n, c_n), lo
    self.x2 = torch.tensor(rng.standard_normal((c_n, a_n * b_n)).astype(np.float32), device="cuda:0")
    self.P = torch.tensor(rng.standard_normal((c_n, c_n)).astype(np.float32), device="cuda:0")
    self.parent = torch.full(shape, SENTINEL, device="cuda:0")
    self.out_ref = torch.full((a_n * b_n, c_n), SENTINEL, device="cuda:0")

  def seg_row(self, tbl, i):
    a_n, b_n, c_n = self.dims
    _, B, Cf = self.parent.shape
    _row(tbl, i, self.x2.data_ptr(), self.P.data_ptr(), _addr(self.parent, *self.lo),
         a_n * b_n, c_n, c_n, a_n * b_n, c_n, Cf, m_seg=b_n, a_ss=b_n, c_ss=B * Cf)

  def plain_row(self, tbl, i):
    a_n, b_n, c_n = self.dims
    _row(tbl, i, self.x2.data_ptr(), self.P.data_ptr(), self.out_ref.data_ptr(),
         a_n * b_n, c_n, c_n, a_n * b_n, c_n, c_n)

  def check(self):
    a_n, b_n, c_n = self.dims
    a0, b0, c0 = self.lo
    blk = self.parent[a0:a0 + a_n, b0:b0 + b_n, c0:c0 + c_n]
    assert torch.equal(blk.reshape(a_n * b_n, c_n), self.out_ref), self.dims
    outside = torch.ones(self.parent.shape, dtype=torch.bool, device="cuda:0")
    outside[a0:a0 + a_n, b0:b0 + b_n, c0:c0 + c_n] = False
    assert bool((self.parent[outside] == SENTINEL).all())


def test_stage3_segmented_output_ragged_block_inside_the_parent(device):
  """b_n < B: the result's rows (a', b') are segments.  Ragged extents, an unaligned (b_n odd) and an
  aligned segment of X2, more than one tile row per segment, a single-row segment."""
  L, K, lib = _mods()
  rng = np.random.default_rng(7)
  cases = [_Stage3(rng, 5, 37, 50, (7, 64, 77), (1, 20, 13)),
           _Stage3(rng, 3, 36, 64, (4, 40, 64), (1, 4, 0)),
           _Stage3(rng, 2, 150, 130, (3, 151, 133), (0, 1, 2)),
           _Stage3(rng, 6, 1, 9, (8, 3, 12), (2, 1, 3))]
  seg = np.zeros(len(cases), K._GSEGDESC_DT)
  plain = np.zeros(len(cases), K._GDESC_DT)
  for i, cs in enumerate(cases):
    cs.seg_row(seg, i)
    cs.plain_row(plain, i)
  assert _call(plain) == 0
  assert _call(seg) == 0
  for cs in cases:
    cs.check()


def test_one_call_mixes_segmented_and_unsegmented_descriptors(device):
  """Rows of the rank-2 stages (m_seg = 0, both orientations of A) ride in the call of the rank-3
  stages: every row equals its ps_gemm_grouped_typed twin."""
  L, K, lib = _mods()
  rng = np.random.default_rng(11)
  s1 = _Stage1(rng, 64, 2, 64, 71, 3)
  s3 = _Stage3(rng, 5, 37, 50, (7, 64, 77), (1, 20, 13))
  mk = lambda *s: torch.tensor(rng.standard_normal(s).astype(np.float32), device="cuda:0")
  # X = g^T P (transa = 1) and X^T = P g (transa = 0) on a [70, 150] block with ld 160
  g, p = mk(70, 160), mk(70, 70)
  outs = [torch.full((150, 70), SENTINEL, device="cuda:0") for _ in range(2)]
  outs_t = [torch.full((70, 150), SENTINEL, device="cuda:0") for _ in range(2)]
  tbls = []
  for j, dt in enumerate((K._GSEGDESC_DT, K._GDESC_DT)):
    t = np.zeros(4, dt)
    (s1.seg_row if j == 0 else s1.plain_row)(t, 0)
    (s3.seg_row if j == 0 else s3.plain_row)(t, 1)
    _row(t, 2, g.data_ptr(), p.data_ptr(), outs[j].data_ptr(), 150, 70, 70, 160, 70, 70)
    _row(t, 3, p.data_ptr(), g.data_ptr(), outs_t[j].data_ptr(), 70, 150, 70, 70, 160, 150, transa=0)
    tbls.append(t)
  assert _call(tbls[1]) == 0
  assert _call(tbls[0]) == 0
  s1.check()
  s3.check()
  assert torch.equal(outs[0], outs[1]) and torch.equal(outs_t[0], outs_t[1])
  assert not bool((outs[0] == SENTINEL).any()) and not bool((outs_t[0] == SENTINEL).any())


@pytest.mark.parametrize("c0", [3, 4], ids=["odd_offset", "aligned"])
def test_bf16_operand_a_segmented_bit_identical_to_the_contiguous_copy(device, c0):
  """bf16 gradients are operand A of stage 1: read where they lie, 2-byte elements, incl. a block that
  starts at an odd element offset (no 8-byte loads)."""
  L, K, lib = _mods()
  rng = np.random.default_rng(13 + c0)
  cases = [_Stage1(rng, a_n, nseg, m_seg, 212 if c0 == 4 else 211, c0, dtype=torch.bfloat16)
           for a_n, nseg, m_seg in ((64, 2, 64), (5, 5, 3), (130, 2, 200), (64, 1, 128))]
  if c0 == 3:
    assert any((_addr(cs.parent, *cs.lo) // 2) % 2 == 1 for cs in cases)
  seg = np.zeros(len(cases), K._GSEGDESC_DT)
  plain = np.zeros(len(cases), K._GDESC_DT)
  for i, cs in enumerate(cases):
    cs.seg_row(seg, i)
    cs.plain_row(plain, i)
  assert _call(plain, a_dt=1) == 0
  assert _call(seg, a_dt=1) == 0
  for cs in cases:
    cs.check()


def test_split_k_segmented_against_float64(device):
  """Parent [512, 2, 600], block [512, 2, 512]: k = 512 and 32 tiles, so the call splits k; the reduce
  pass writes the segmented result.  |got - ref| <= (k + 2) 2^-24 (|A|^T |B|) elementwise: a float32
  sum of k products accumulated in any order, plus the partial sums' final additions."""
  L, K, lib = _mods()
  rng = np.random.default_rng(17)
  k = 512
  host = rng.standard_normal((k, 2, 600)).astype(np.float32)
  parent = torch.tensor(host, device="cuda:0")
  ph = rng.standard_normal((k, k)).astype(np.float32)
  P = torch.tensor(ph, device="cuda:0")
  c0 = 40
  # result written segmented too: [2, 512 rows] inside a [2, 520, 512 + 8] buffer, row offset 3, column offset 4
  out = torch.full((2, 520, 520), SENTINEL, device="cuda:0")
  seg = np.zeros(1, K._GSEGDESC_DT)
  _row(seg, 0, _addr(parent, 0, 0, c0), P.data_ptr(), _addr(out, 0, 3, 4), 1024, k, k, 2 * 600, k, 520,
       m_seg=512, a_ss=600, c_ss=520 * 520)
  assert _call(seg) == 0
  assert torch.equal(parent, torch.tensor(host, device="cuda:0"))
  blk = host[:, :, c0:c0 + 512].astype(np.float64)                 # [k, 2, 512]
  ref = np.einsum("kbc,kn->bcn", blk, ph.astype(np.float64))
  bound = (k + 2) * 2.0 ** -24 * np.einsum("kbc,kn->bcn", np.abs(blk), np.abs(ph).astype(np.float64))
  got = out[:, 3:515, 4:516].cpu().numpy().astype(np.float64)
  err = np.abs(got - ref)
  print("split-K: max err / bound =", float((err / bound).max()))
  assert np.all(err <= bound)
  outside = torch.ones(out.shape, dtype=torch.bool, device="cuda:0")
  outside[:, 3:515, 4:516] = False
  assert bool((out[outside] == SENTINEL).all())


def test_unsupported_combinations_are_refused_and_write_nothing(device):
  L, K, lib = _mods()
  rng = np.random.default_rng(19)
  s1 = _Stage1(rng, 64, 2, 64, 72, 4)
  t = np.zeros(1, K._GSEGDESC_DT)
  s1.seg_row(t, 0)
  bad = []
  bad.append((t.copy(), 0, 1))            # bf16 B
  bad.append((t.copy(), 1, 1))            # both bf16
  u = t.copy(); u["transb"] = 1
  bad.append((u, 1, 0))                   # bf16 A with transb = 1
  u = t.copy(); u["transa"] = 0; u["lda"] = 4096
  bad.append((u, 0, 0))                   # segmented rows of a k-contiguous A
  u = t.copy(); u["m_seg"] = 0; u["transa"] = 0; u["lda"] = 4096
  bad.append((u, 1, 0))                   # bf16 A with transa = 0
  u = t.copy(); u["m"] = 40000; u["m_seg"] = 1
  bad.append((u, 0, 0))                   # 40000 tile rows: beyond the 16-bit tile coordinates
  for tbl, a_dt, b_dt in bad:
    assert _call(tbl, a_dt, b_dt) == PS_EUNSUPPORTED
    assert bool((s1.out == SENTINEL).all())
    assert torch.equal(s1.parent, s1.parent_before)
