"""Quantizer (GPU): the paths no other test reaches -- the 64 x 256 tile kernels (scalar and float4 branches, encode
and decode), strided views (ld != cols, ldq != cols: only the C ABI can express them) and one descriptor list with a
tensor of every path.  Inputs from the rounding-boundary generator; codes, bucket sizes, diagonals and to_float are
the oracle's (oracle/quantization_oracle.py) bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import quantization_oracle as qorc
from tests.quant_inputs import rounding_boundary_input

pytestmark = pytest.mark.gpu

_TQ = {8: torch.int8, 16: torch.int16}
_NP = {8: np.int8, 16: np.int16}
_CODE_SENTINEL = {8: -77, 16: -12345}
_FLOAT_SENTINEL = -7.5


def K():
  from precondition_amd import kernels
  return kernels


def _u32(a):
  return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


@pytest.mark.parametrize("shape,bits,extract", [((1100, 7), 8, False), ((1100, 13), 16, False),
                                                ((1027, 1027), 16, True)])
def test_tile_scalar_path_quantize_and_dequantize(shape, bits, extract, device):
  """More than 1024 rows and a column count that is no multiple of 4: quant_colmax_kernel / quant_encode_kernel and
  the tile decode, one column per lane.  (1027, 1027): the diagonal crosses a ragged last row chunk (rows 1024 ...
  1026) and a ragged last column strip (columns 1024 ... 1026)."""
  x = rounding_boundary_input(shape, bits, extract)
  oq, od, ob = qorc.quantize(x, _NP[bits], extract)
  q, d, b = K().quantize_grouped([torch.tensor(x, device=device)], _TQ[bits], extract)[0]
  assert np.array_equal(q.cpu().numpy(), oq)
  assert np.array_equal(_u32(b.cpu().numpy()), _u32(ob))
  if extract:
    assert np.array_equal(_u32(d.cpu().numpy()), _u32(od))
  f = K().dequantize_grouped([(q, d, b)])[0]
  assert np.array_equal(_u32(f.cpu().numpy()), _u32(qorc.to_float(oq, od, ob, _NP[bits], extract)))


class _Case:
  """One tensor of a descriptor list: input in a [rows, ld] buffer, codes in a [rows, ldq] buffer (ld = ldq), the
  padding columns of the code buffer and of the dequantize output filled with sentinels."""

  def __init__(self, shape, ld, bits, extract, device):
    self.shape, self.ld, self.bits, self.extract = shape, ld, bits, extract
    rows, cols = shape
    self.x = rounding_boundary_input(shape, bits, extract)
    self.oq, self.od, self.ob = qorc.quantize(self.x, _NP[bits], extract)
    self.of = qorc.to_float(self.oq, self.od, self.ob, _NP[bits], extract)
    self.fin = torch.full((rows, ld), _FLOAT_SENTINEL, dtype=torch.float32, device=device)
    self.fin[:, :cols] = torch.tensor(self.x, device=device)
    self.codes = torch.full((rows, ld), _CODE_SENTINEL[bits], dtype=_TQ[bits], device=device)
    self.fout = torch.full((rows, ld), _FLOAT_SENTINEL, dtype=torch.float32, device=device)
    self.bucket = torch.zeros(cols, dtype=torch.float32, device=device)
    self.diag = torch.zeros(rows if extract else 0, dtype=torch.float32, device=device)

  def check_quantized(self):
    cols = self.shape[1]
    codes = self.codes.cpu().numpy()
    assert np.array_equal(codes[:, :cols], self.oq), self.shape
    assert (codes[:, cols:] == _CODE_SENTINEL[self.bits]).all(), self.shape        # padding untouched
    assert np.array_equal(_u32(self.bucket.cpu().numpy()), _u32(self.ob)), self.shape
    if self.extract:
      assert np.array_equal(_u32(self.diag.cpu().numpy()), _u32(self.od)), self.shape

  def check_dequantized(self):
    cols = self.shape[1]
    f = self.fout.cpu().numpy()
    assert np.array_equal(_u32(f[:, :cols]), _u32(self.of)), self.shape
    assert (f[:, cols:] == np.float32(_FLOAT_SENTINEL)).all(), self.shape          # padding untouched


def _abi_roundtrip(cases, device):
  """ps_quantize_f32, then ps_dequantize_f32, of the whole list in one call each, as quantize_grouped issues them."""
  k = K()
  n = len(cases)
  L = k.lib()
  with torch.cuda.device(device):
    for fvalue, call, query, what in (("fin", L.ps_quantize_f32, L.ps_quantize_workspace_bytes, "ps_quantize_f32"),
                                      ("fout", L.ps_dequantize_f32, L.ps_dequantize_workspace_bytes,
                                       "ps_dequantize_f32")):
      tbl, descs = k._quant_desc_table(n)
      tbl["fvalue"] = [getattr(c, fvalue).data_ptr() for c in cases]
      tbl["codes"] = [c.codes.data_ptr() for c in cases]
      tbl["bucket_size"] = [c.bucket.data_ptr() for c in cases]
      tbl["diagonal"] = [c.diag.data_ptr() if c.extract else 0 for c in cases]
      tbl["rows"] = [c.shape[0] for c in cases]
      tbl["cols"] = [c.shape[1] for c in cases]
      tbl["ld"] = tbl["ldq"] = [c.ld for c in cases]
      tbl["bits"] = [c.bits for c in cases]
      tbl["extract_diagonal"] = [int(c.extract) for c in cases]
      ws = k._workspace(query(descs, n), device)
      k.check(call(k._stream(), descs, n, ws.data_ptr(), ws.numel()), what)
      torch.cuda.synchronize()
      for c in cases:
        c.check_quantized()            # (dequantize leaves codes, bucket sizes and diagonal alone)
        if fvalue == "fout":
          c.check_dequantized()


@pytest.mark.parametrize("shape,ld,bits,extract", [
    ((1100, 260), 264, 8, False), ((1100, 260), 264, 16, False), ((1028, 1028), 1032, 16, True),
    ((70, 260), 264, 16, False)])
def test_strided_views_through_the_c_abi(shape, ld, bits, extract, device):
  """ld = ldq > cols (include/ps_api.h).  (1100, 260): the tile float4 encode and decode, two column strips, the
  second four columns wide; (1028, 1028): the same with a diagonal; (70, 260): the small path encodes a strided
  tensor, the tile float4 branch decodes it."""
  _abi_roundtrip([_Case(shape, ld, bits, extract, device)], device)


def test_one_call_with_a_tensor_of_every_path(device):
  """int8, no diagonal: strip, tall strip (team of 3), small, small in several column ranges, flat, tile scalar and
  tile float4 in ONE descriptor list -- the offsets between the chunk lists of the per-chunk table.  Quantized, then
  dequantized as the same list in one call."""
  shapes = [((512, 320), 320), ((3072, 768), 768), ((200, 3), 3), ((1, 5000), 5000), ((4100, 64), 64),
            ((1100, 7), 7), ((1100, 260), 264)]
  _abi_roundtrip([_Case(s, ld, 8, False, device) for s, ld in shapes], device)
