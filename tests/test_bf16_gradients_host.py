"""Host side of the native bfloat16-gradient path (no GPU): argument checks of the typed entry
points, the tree plan's gradient pointer columns for 2- and 4-byte gradients, and the CPU stand-in
backend, which declares no bf16 capability and must keep being handed float32 copies."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cpu_backend

PS_EINVAL = -1
SHAPES = [(768, 3072), (197, 64), (768,), (3072,), (64,), (5000, 8)]   # the last one is skipped
BLOCK = 1024


def _lib():
  from precondition_amd import _lib as L
  return L, L.lib()


def test_typed_entries_refuse_unknown_dtype_codes_and_null_descriptors():
  L, lib = _lib()
  ws = C.create_string_buffer(4096)
  sd, gd, td = (L.StatsDesc * 1)(), (L.GemmDesc * 1)(), (L.TransformDesc * 1)()
  cfg = L.TransformConfig()
  assert lib.ps_version() >= 307
  assert lib.ps_stats_update_grouped_typed(None, sd, 1, 7, 1.0, 1.0, ws, 4096) == PS_EINVAL
  assert lib.ps_gemm_grouped_typed(None, gd, 1, 7, 0, ws, 4096) == PS_EINVAL
  assert lib.ps_gemm_grouped_typed(None, gd, 1, 0, 7, ws, 4096) == PS_EINVAL
  assert lib.ps_transform_grads_typed(None, td, 1, C.byref(cfg), 7, 0, ws, 4096) == PS_EINVAL
  assert lib.ps_transform_grads_typed(None, td, 1, C.byref(cfg), 0, 7, ws, 4096) == PS_EINVAL
  for code in (0, 1):
    assert lib.ps_stats_update_grouped_typed(None, None, 1, code, 1.0, 1.0, ws, 4096) == PS_EINVAL
    assert lib.ps_gemm_grouped_typed(None, None, 1, code, 0, ws, 4096) == PS_EINVAL
    assert lib.ps_transform_grads_typed(None, None, 1, C.byref(cfg), code, code, ws, 4096) == PS_EINVAL


def _plan():
  from precondition_amd.blocking import Preconditioner
  from precondition_amd.plan import TreePlan
  skipped = [any(d > 4096 for d in s) for s in SHAPES]
  pcs = [None if sk else Preconditioner(torch.empty(s, device="meta"), BLOCK, 4096, False)
         for s, sk in zip(SHAPES, skipped)]
  pl = TreePlan.build(SHAPES, pcs, skipped)
  assert pl is not None
  return pl, pcs, skipped


@pytest.mark.parametrize("itemsize", [2, 4])
def test_gradient_pointer_columns_scale_with_the_item_size(itemsize):
  pl, pcs, skipped = _plan()
  base = np.array([0x7F0000000000 + 0x10000000 * i + 6 for i in range(len(SHAPES))], np.uint64)
  cols = pl.grad_columns(base, itemsize)
  st, aa, sa = [], [], []
  vec_rows = []
  for i, (shape, pc, sk) in enumerate(zip(SHAPES, pcs, skipped)):
    if sk:
      continue
    meta = torch.empty(pc._transformed_shape, device="meta")
    for blk in pc._partitioner.partition(meta):
      addr = int(base[i]) + int(blk.storage_offset()) * itemsize
      if blk.dim() == 1:
        st.append(addr)
        vec_rows.append(len(aa))
        aa.append(addr)
      else:
        st += [addr, addr]       # both axes read the same block
        aa.append(addr)
        sa.append(addr)
  assert cols["st_g"].tolist() == st
  assert cols["a_a"].tolist() == aa               # reference orientation, one-row rows included
  assert cols["sa_b"].tolist() == sa              # symmetric orientation
  assert pl.a_vec_rows.tolist() == vec_rows
  assert len(vec_rows) > 0 and len(sa) > 3        # the tree has 1-D blocks and a parameter that blocks


def test_float32_offset_columns_do_not_depend_on_the_item_size():
  """a_coff, b_xoff, b_coff, sa_xoff address float32 buffers: bytes of float32 whatever the gradient;
  for a 1-D block a_coff (the result) is 4 x the element offset that a_goff holds."""
  pl, pcs, skipped = _plan()
  vr = pl.a_vec_rows
  assert np.array_equal(pl.a_coff[vr], pl.a_goff[vr] * np.uint64(4))
  assert np.array_equal(pl.b_coff, pl.sa_goff * np.uint64(4))   # stage B writes the block of the result
  mat = np.setdiff1d(np.arange(len(pl.a_tbl)), vr)
  assert np.array_equal(pl.a_coff[mat], pl.sa_xoff) and np.array_equal(pl.b_xoff, pl.sa_xoff)
  assert np.all(pl.sa_xoff % np.uint64(4) == 0)
  c2, c4 = pl.grad_columns(np.zeros(len(SHAPES), np.uint64), 2), pl.grad_columns(np.zeros(len(SHAPES), np.uint64), 4)
  for k in c2:
    assert np.array_equal(c2[k] * np.uint64(2), c4[k])


def test_symmetric_layout_rule():
  pl, _, _ = _plan()
  assert pl.symmetric_layout(True, torch.float32)
  assert not pl.symmetric_layout(False, torch.float32)
  assert not pl.symmetric_layout(True, torch.bfloat16)    # the tree has one-row products


def test_cpu_stand_in_backend_still_gets_promoted_copies():
  import precondition_amd as pa
  assert not hasattr(cpu_backend, "NATIVE_BF16_GRADIENTS")
  shapes = [(40, 24), (24,)]
  rng = np.random.default_rng(3)
  params = [torch.from_numpy(np.asarray(rng.standard_normal(s) * 0.1, np.float32)).to(torch.bfloat16)
            for s in shapes]

  def run(widen):
    opt = pa.distributed_shampoo(0.1, 16, preconditioning_compute_steps=2, start_preconditioning_step=1,
                                 graft_type=pa.GraftingType.RMSPROP_NORMALIZED, weight_decay=1e-3,
                                 _backend_for_testing=cpu_backend)
    prm = [p.float() for p in params] if widen else params
    st, ups = opt.init(prm), []
    for t in range(4):
      r = np.random.default_rng(50 + t)
      g = [torch.from_numpy(np.asarray(r.standard_normal(s) * 0.1, np.float32)).to(torch.bfloat16)
           for s in shapes]
      u, st = opt.update([x.float() for x in g] if widen else g, st, prm)
      ups.append(u)
    return ups

  for a, b in zip(run(True), run(False)):
    for x, y in zip(a, b):
      assert y.dtype == torch.bfloat16
      assert torch.equal(x.to(torch.bfloat16), y)
