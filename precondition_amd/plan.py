"""Per-tree plan of the every-step calls of update() (DS:3627-3659).

Everything about a parameter tree that depends on its SHAPES only — which blocks a parameter
is cut into, where a block starts inside the (merged, contiguous) gradient, the dimensions and
leading dimensions of every Gram update and of every product of the preconditioner
application — is resolved once, into NumPy descriptor-table templates.  A step then only
fills the pointer columns (`base pointer of the parameter's gradient + byte offset of the
block`, statistics / preconditioner / output pointers) with a few vector operations and hands
the tables to the C-ABI: no block views, no per-block Python objects.  The reference gets the
same effect from tracing its Python-unrolled loops (DS:1582-1590, 1689-1708) once under jit.

Covers blocks of merged rank 1, 2 and 3 with every axis preconditioned and no compression (the
dense mode of a transformer tree; conv kernels and stacked expert / per-head weights, which
merge_small_dims leaves at rank 3); anything else makes `TreePlan.build` return None and the
optimizer keeps its general per-block path.

A rank-3 block [a, b, c] of a parameter [A, B, C] is applied as the reference applies it, three
contractions of the leading axis with the new axis last (DS:1689-1708), each one row of a grouped
launch that addresses the block where it lies (ps_gemm_seg_desc, include/ps_api.h):
    X1[(b c), a']  = G [a, (b c)]^T  P_a    A = the gradient block in place: b segments of c rows
    X2[(c a'), b'] = X1[b, (c a')]^T P_b    scratch to scratch
    Y [(a' b'), c'] = X2[c, (a' b')]^T P_c   into the result in place: a segments of b rows
Stage 1 rides in the launch of the rank-2 stage A, stage 2 in that of stage B, stage 3 is a third
launch; trees without rank-3 blocks get the tables and the two launches they always had.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import kernels
from ._lib import GemmDesc, GemmSegDesc, StatsDesc, check, lib


# storage type codes of the ps_*_typed entry points (include/ps_api.h PS_DTYPE_*)
DTYPE_CODE = {torch.float32: 0, torch.bfloat16: 1}


def _as_seg(tbl: np.ndarray) -> np.ndarray:
  """A ps_gemm_desc table as unsegmented ps_gemm_seg_desc rows (m_seg = 0)."""
  t = np.zeros(len(tbl), kernels._GSEGDESC_DT)
  for name in kernels._GDESC_DT.names:
    t[name] = tbl[name]
  return t


def _with_rank3(tbl: np.ndarray, r_tbl: np.ndarray) -> np.ndarray:
  """A stage's rows followed by the rank-3 rows that share its launch; `tbl` itself when there are none."""
  return np.concatenate([_as_seg(tbl), r_tbl]) if len(r_tbl) else tbl


def gemm_workspace_bytes(tbl: np.ndarray) -> int:
  L = lib()
  if tbl.dtype == kernels._GSEGDESC_DT:
    return L.ps_gemm_grouped_seg_workspace_bytes(C.cast(tbl.ctypes.data, C.POINTER(GemmSegDesc)), len(tbl))
  return L.ps_gemm_grouped_workspace_bytes(C.cast(tbl.ctypes.data, C.POINTER(GemmDesc)), len(tbl))


def gemm_launch(stream, tbl: np.ndarray, a_dt: int, b_dt: int, ws_ptr: int, ws_bytes: int):
  """One grouped launch of a stage table: the segmented entry for tables that carry rank-3 rows."""
  L = lib()
  if tbl.dtype == kernels._GSEGDESC_DT:
    rc = L.ps_gemm_grouped_seg_typed(stream, C.cast(tbl.ctypes.data, C.POINTER(GemmSegDesc)), len(tbl),
                                     a_dt, b_dt, ws_ptr, ws_bytes)
    check(rc, "ps_gemm_grouped_seg_typed")
  else:
    rc = L.ps_gemm_grouped_typed(stream, C.cast(tbl.ctypes.data, C.POINTER(GemmDesc)), len(tbl),
                                 a_dt, b_dt, ws_ptr, ws_bytes)
    check(rc, "ps_gemm_grouped_typed")


def _tiles_fit(m: int, m_seg: int, n: int) -> bool:
  """The tile coordinates of a (segmented) product fit the library's 16-bit fields (ps_api.h)."""
  m_seg = m_seg or m
  return (m // m_seg) * ((m_seg + 127) // 128) <= 0x7fff and (n + 127) // 128 <= 0x7fff


def uniform_dtype(tensors):
  """The common dtype of `tensors` when it is one the typed kernels read (float32 / bfloat16), else None."""
  if not tensors:
    return None
  dt = tensors[0].dtype
  if dt not in DTYPE_CODE or any(t.dtype != dt for t in tensors):
    return None
  return dt


class TreePlan:

  def __init__(self):
    self.n_params = 0
    self.skipped: List[bool] = []
    self.numel: List[int] = []
    self.tshapes: List[tuple] = []
    self.n_stats_of: List[int] = []       # statistics per parameter
    self.stat_dims = np.zeros(0, np.int64)  # d of every statistic, plan order
    # statistics table
    self.stats_tbl = None
    self.st_param = None
    self.st_goff = None
    # application tables
    self.a_tbl = self.b_tbl = None
    self.a_param = self.a_goff = self.a_stat = self.a_coff = self.a_c_is_res = None
    self.b_param = self.b_stat = self.b_xoff = self.b_coff = None
    self.x_elems = 0
    # rank-3 blocks: one row per block in each of three stage tables (ps_gemm_seg_desc)
    self.r1_tbl = self.r2_tbl = self.r3_tbl = np.zeros(0, kernels._GSEGDESC_DT)
    self.r_param = self.r_stat = np.zeros(0, np.int64)
    self.r_goff = self.r_roff = self.r_coff = np.zeros(0, np.uint64)
    self.r_elems = 0        # floats of EACH of the two ping-pong regions X1, X2

  @property
  def scratch_elems(self) -> int:
    """Floats of the application's scratch: X of the rank-2 blocks, then X1 and X2 of the rank-3 blocks."""
    return max(self.x1_start + 2 * self.r_elems, 1)

  @property
  def x1_start(self) -> int:
    """First float of X1 inside the scratch (16-byte aligned); X2 follows r_elems floats later."""
    return (self.x_elems + 3) // 4 * 4 if self.r_elems else self.x_elems

  @staticmethod
  def build(shapes: Sequence[tuple], pcs, skipped: Sequence[bool]) -> Optional["TreePlan"]:
    """pcs[i]: blocking.Preconditioner of parameter i (None when skipped)."""
    pl = TreePlan()
    pl.n_params = len(shapes)
    pl.skipped = list(skipped)
    st_rows, a_rows, b_rows, sa_rows, sb_rows, r_rows = [], [], [], [], [], []
    stat_base = 0
    x_off = 0
    r_off = 0
    for i, (shape, pc) in enumerate(zip(shapes, pcs)):
      ne = 1
      for d in shape:
        ne *= int(d)
      pl.numel.append(ne)
      if pl.skipped[i]:
        pl.tshapes.append(tuple(shape))
        pl.n_stats_of.append(0)
        continue
      tshape = pc._transformed_shape
      nd = len(tshape)
      if nd not in (1, 2, 3) or not all(pc.should_precondition_dims()) or pc._compression_rank:
        return None
      if ne == 0:
        return None
      pl.tshapes.append(tshape)
      meta = torch.empty(tshape, dtype=torch.float32, device="meta")
      row_ld = int(tshape[1]) if nd == 2 else 1
      k = 0
      if nd == 3:
        B_, C_ = int(tshape[1]), int(tshape[2])
        for blk in pc._partitioner.partition(meta):
          off = int(blk.storage_offset())
          a, b, c = (int(x) for x in blk.shape)
          if tuple(blk.stride()) != (B_ * C_, C_, 1):
            return None
          # gram_desc's 3-D cases on the parameter's strides: (layout, d, k, ld, nseg, seg_stride)
          st_rows.append((i, off, 0, a, c, B_ * C_, b, C_))     # axis 0: k = (j, c), segments over j
          st_rows.append((i, off, 0, b, c, C_, a, B_ * C_))     # axis 1: k = (a, c), segments over a
          st_rows.append((i, off, 1, c, b, C_, a, B_ * C_))     # axis 2: k = (a, j), segments over a
          # rows (b, c) of the gradient block / rows (a', b') of the result are one run when the block
          # spans the axis (or has one segment): plain rows then
          seg1 = 0 if (c == C_ or b == 1) else c
          seg3 = 0 if (b == B_ or a == 1 or b == 1) else b   # (b == 1: plain rows B*C apart)
          if not (_tiles_fit(b * c, seg1, a) and _tiles_fit(c * a, 0, b) and _tiles_fit(a * b, seg3, c)):
            return None
          r_rows.append((i, off, stat_base + k, a, b, c, B_, C_, seg1, seg3, r_off))
          r_off += (a * b * c + 3) // 4 * 4   # every block's scratch 16-byte aligned
          k += 3
        pl.n_stats_of.append(k)
        stat_base += k
        continue
      for blk in pc._partitioner.partition(meta):
        # offset of the block inside its parameter in ELEMENTS: the gradient columns scale it by the
        # gradient's item size (grad_columns), the float32 result / intermediate columns by 4
        off = int(blk.storage_offset())
        if nd == 1:
          d = int(blk.shape[0])
          # gram_desc: [d] -> layout 1, k = 1, ld = d
          st_rows.append((i, off, 1, d, 1, d, 1, 0))
          # g^T P as a one-row product: a = [d, 1] (transa), c = [1, d] inside the result
          a_rows.append((i, off, stat_base + k, d * 0 + 1, d, d, 1, d, d, True, off * 4))
          k += 1
        else:
          m, n = int(blk.shape[0]), int(blk.shape[1])
          if blk.stride(1) != 1 or blk.stride(0) != row_ld:
            return None
          st_rows.append((i, off, 0, m, n, row_ld, 1, 0))   # axis 0: layout 0, d = m, k = n
          st_rows.append((i, off, 1, n, m, row_ld, 1, 0))   # axis 1: layout 1, d = n, k = m
          # stage A: X [n, m] = g^T P_L (transa);  stage B: Y [m, n] = X^T P_R into the result
          a_rows.append((i, off, stat_base + k, n, m, m, row_ld, m, m, False, x_off * 4))
          b_rows.append((i, stat_base + k + 1, x_off * 4, off * 4, m, n, n, m, n, row_ld))
          # symmetric preconditioners (apply_preconditioners): X^T [m, n] = P_L g, Y = X^T P_R
          # (param, goff, stat, m, n, k, lda, ldb, ldc, xoff) / (param, stat, xoff, coff, m, n, k, lda, ldb, ldc)
          sa_rows.append((i, off, stat_base + k, m, n, m, m, row_ld, n, x_off * 4))
          sb_rows.append((i, stat_base + k + 1, x_off * 4, off * 4, m, n, n, n, n, row_ld))
          x_off += m * n
          k += 2
      pl.n_stats_of.append(k)
      stat_base += k
    pl.x_elems = x_off
    pl.r_elems = r_off
    # ---- statistics template -------------------------------------------------
    S = len(st_rows)
    tbl = np.zeros(S, kernels._SDESC_DT)
    if S:
      arr = np.array(st_rows, np.int64)
      pl.st_param, pl.st_goff = arr[:, 0].copy(), arr[:, 1].astype(np.uint64)
      tbl["layout"], tbl["d"], tbl["k"], tbl["ld"] = arr[:, 2], arr[:, 3], arr[:, 4], arr[:, 5]
      tbl["nseg"], tbl["seg_stride"] = arr[:, 6], arr[:, 7]
      tbl["lds"] = arr[:, 3]
      pl.stat_dims = arr[:, 3].copy()
    pl.stats_tbl = tbl
    # ---- application templates -------------------------------------------------
    def gemm_tbl(rows):
      t = np.zeros(len(rows), kernels._GDESC_DT)
      return t
    if r_rows:
      # (param, goff, stat, a, b, c, B, C, seg1, seg3, roff): three products per block, transa = 1
      r = np.array(r_rows, np.int64)
      a, b, c, B_, C_ = r[:, 3], r[:, 4], r[:, 5], r[:, 6], r[:, 7]
      pl.r_param, pl.r_stat = r[:, 0].copy(), r[:, 2].copy()
      pl.r_goff = r[:, 1].astype(np.uint64)
      pl.r_coff = pl.r_goff * np.uint64(4)
      pl.r_roff = r[:, 10].astype(np.uint64) * np.uint64(4)
      def seg_tbl(m, n, k, lda, ldc, m_seg=0, a_seg=0, c_seg=0):
        t = np.zeros(len(r_rows), kernels._GSEGDESC_DT)
        t["m"], t["n"], t["k"], t["lda"], t["ldb"], t["ldc"] = m, n, k, lda, n, ldc
        t["transa"], t["transb"] = 1, 0
        t["m_seg"], t["a_seg_stride"], t["c_seg_stride"] = m_seg, a_seg, c_seg
        return t
      seg1, seg3 = r[:, 8], r[:, 9]
      # stage 1 reads b segments of c rows, C apart, and writes X1 [(b c), a] densely
      pl.r1_tbl = seg_tbl(b * c, a, a, B_ * C_, a, seg1, np.where(seg1 > 0, C_, 0),
                          np.where(seg1 > 0, c * a, 0))
      pl.r2_tbl = seg_tbl(c * a, b, b, c * a, b)
      # stage 3 reads X2 [c, (a b)] densely and writes a segments of b rows, B*C apart
      pl.r3_tbl = seg_tbl(a * b, c, c, a * b, np.where(b == 1, B_ * C_, C_), seg3, np.where(seg3 > 0, b, 0),
                          np.where(seg3 > 0, B_ * C_, 0))
    pl.a_tbl = gemm_tbl(a_rows)
    if a_rows:
      # (param, goff, stat, m, n, k, lda, ldb, ldc, c_is_res, coff)
      pl.a_param = np.array([r[0] for r in a_rows], np.int64)
      pl.a_goff = np.array([r[1] for r in a_rows], np.uint64)
      pl.a_stat = np.array([r[2] for r in a_rows], np.int64)
      pl.a_c_is_res = np.array([r[9] for r in a_rows], bool)
      pl.a_coff = np.array([r[10] for r in a_rows], np.uint64)
      t = pl.a_tbl
      t["m"] = [r[3] for r in a_rows]
      t["n"] = [r[4] for r in a_rows]
      t["k"] = [r[5] for r in a_rows]
      t["lda"] = [r[6] for r in a_rows]
      t["ldb"] = [r[7] for r in a_rows]
      t["ldc"] = [r[8] for r in a_rows]
      t["transa"], t["transb"] = 1, 0
    pl.b_tbl = gemm_tbl(b_rows)
    if b_rows:
      # (param, stat, xoff, coff, m, n, k, lda, ldb, ldc)
      pl.b_param = np.array([r[0] for r in b_rows], np.int64)
      pl.b_stat = np.array([r[1] for r in b_rows], np.int64)
      pl.b_xoff = np.array([r[2] for r in b_rows], np.uint64)
      pl.b_coff = np.array([r[3] for r in b_rows], np.uint64)
      t = pl.b_tbl
      t["m"] = [r[4] for r in b_rows]
      t["n"] = [r[5] for r in b_rows]
      t["k"] = [r[6] for r in b_rows]
      t["lda"] = [r[7] for r in b_rows]
      t["ldb"] = [r[8] for r in b_rows]
      t["ldc"] = [r[9] for r in b_rows]
      t["transa"], t["transb"] = 1, 0
    # ---- the same application for bitwise symmetric preconditioners: P_L g instead of g^T P_L.
    # Element (i, j) of P_L g sums P[i][k] g[k][j] over k, element (j, i) of g^T P_L sums
    # g[k][j] P[k][i]: the same products in the same order when P[i][k] == P[k][i] bit for bit, so
    # X^T comes out bit-identical -- but the left operand is now k-contiguous (16-byte LDS
    # fragment reads instead of four 4-byte ones) and the stage-B product reads X^T the same way:
    # 0.72-0.77 -> 0.80-0.83 of the fp32 MFMA peak on uniform batches of ViT-B's block shapes
    # (round 4 measurement).  One-row products stay in the streaming mat-vec form.
    pl.sa_tbl = gemm_tbl(sa_rows)
    pl.sb_tbl = gemm_tbl(sb_rows)
    if sa_rows:
      pl.sa_param = np.array([r[0] for r in sa_rows], np.int64)
      pl.sa_goff = np.array([r[1] for r in sa_rows], np.uint64)
      pl.sa_stat = np.array([r[2] for r in sa_rows], np.int64)
      pl.sa_xoff = np.array([r[9] for r in sa_rows], np.uint64)
      t = pl.sa_tbl
      for col, idx in (("m", 3), ("n", 4), ("k", 5), ("lda", 6), ("ldb", 7), ("ldc", 8)):
        t[col] = [r[idx] for r in sa_rows]
      t["transa"], t["transb"] = 0, 0
      t = pl.sb_tbl
      for col, idx in (("m", 4), ("n", 5), ("k", 6), ("lda", 7), ("ldb", 8), ("ldc", 9)):
        t[col] = [r[idx] for r in sb_rows]
      t["transa"], t["transb"] = 0, 0
      # one-row products of the 1-D blocks: the rows of a_tbl whose result goes straight to the output
      pl.a_vec_rows = np.nonzero(pl.a_c_is_res)[0] if a_rows else np.zeros(0, np.int64)
    return pl

  # ---------------------------------------------------------------------------
  @staticmethod
  def _ptrs(tensors) -> np.ndarray:
    return np.fromiter((t.data_ptr() for t in tensors), np.uint64, len(tensors))

  def check_dense(self, tensors, what: str, gradients: bool = False):
    """Contiguous float32 tensors on one device (the plan addresses them by pointer).  gradients:
    a list that is uniformly float32 OR uniformly bfloat16 (read natively by the typed kernels)."""
    dev = tensors[0].device
    dt = tensors[0].dtype if gradients and tensors[0].dtype in DTYPE_CODE else torch.float32
    for t in tensors:
      if t.dtype != dt or not t.is_cuda or t.device != dev or not t.is_contiguous():
        kernels._require_gpu(t, what)
        raise ValueError(f"{what}: the tree plan needs contiguous float32 tensors (gradients: all "
                         "float32 or all bfloat16) on one device")
    return dev

  def grad_columns(self, gp: np.ndarray, itemsize: int) -> dict:
    """The pointer columns that address GRADIENT blocks, from the base address of every parameter's
    gradient (gp, uint64) and the gradient's item size: base + element offset * itemsize.
      st_g: `g` of the statistics table;  a_a: `a` of stage A in the reference orientation (the
      one-row products of 1-D blocks included);  sa_b: `b` of stage A in the symmetric orientation;
      r_a: `a` of stage 1 of the rank-3 blocks.
    Every other offset column (a_coff, b_xoff, b_coff, sa_xoff) addresses float32 buffers."""
    sz = np.uint64(itemsize)
    none = np.zeros(0, np.uint64)
    return dict(
        st_g=gp[self.st_param] + self.st_goff * sz if len(self.stats_tbl) else none,
        a_a=gp[self.a_param] + self.a_goff * sz if len(self.a_tbl) else none,
        sa_b=gp[self.sa_param] + self.sa_goff * sz if len(getattr(self, "sa_tbl", ())) else none,
        r_a=gp[self.r_param] + self.r_goff * sz if len(self.r1_tbl) else none)

  def symmetric_layout(self, symmetric_precs: bool, grad_dtype) -> bool:
    """Does stage A run in the symmetric orientation X^T = P_L g?  One grouped call carries one
    storage type per operand, and the one-row products of 1-D blocks keep the gradient as operand A:
    a bfloat16 tree that has such blocks runs the reference orientation (bit-identical results, see
    build), so that the call -- and with it the library's split-K choice -- stays the float32 one."""
    if not (symmetric_precs and len(getattr(self, "sa_tbl", ())) > 0):
      return False
    # (rank-3 blocks always run the reference orientation: their stage 1 keeps the gradient as A too)
    return grad_dtype == torch.float32 or (len(self.a_vec_rows) == 0 and len(self.r1_tbl) == 0)

  def stats_update(self, grads_flat, stats_in, stats_out, w1: float, w2: float):
    """gram_weighted_update of every (block, axis) of the tree (DS:1582-1590) in one launch.
    stats_in / stats_out: flat lists in plan order (contiguous [d, d] tensors)."""
    S = len(self.stats_tbl)
    if S == 0:
      return
    dev = self.check_dense(grads_flat, "gram_weighted_update", gradients=True)
    gdt = grads_flat[0].dtype
    if self.check_dense(list(stats_in) + list(stats_out), "gram_weighted_update") != dev:
      raise ValueError("gram_weighted_update: gradients and statistics live on different devices")
    tbl = self.stats_tbl.copy()
    gp = self._ptrs(grads_flat)
    tbl["g"] = self.grad_columns(gp, grads_flat[0].element_size())["st_g"]
    tbl["stat_in"] = self._ptrs(stats_in)
    tbl["stat_out"] = self._ptrs(stats_out)
    with torch.cuda.device(dev):
      descs = C.cast(tbl.ctypes.data, C.POINTER(StatsDesc))
      L = lib()
      ws = kernels._workspace(L.ps_stats_update_grouped_workspace_bytes(descs, S), dev)
      rc = L.ps_stats_update_grouped_typed(kernels._stream(), descs, S, DTYPE_CODE[gdt], float(w1),
                                           float(w2), ws.data_ptr(), ws.numel())
    check(rc, "ps_stats_update_grouped_typed")

  def apply_preconditioners(self, grads_flat, precs_flat, results, symmetric_precs=False):
    """Preconditioner.preconditioned_grad (DS:1645-1708) for every planned parameter:
    two grouped launches, and a third when the tree has rank-3 blocks.  precs_flat: preconditioners in plan order; results[i]: contiguous
    output of parameter i (None for skipped parameters).  symmetric_precs: the preconditioners
    are bitwise symmetric (roots of the symmetric Newton / eigh paths, identities): the products
    are issued as X^T = P_L g, Y = X^T P_R (bit-identical, faster operand layout; see build)."""
    if len(self.a_tbl) == 0 and len(self.r1_tbl) == 0:
      return
    dev = self.check_dense(grads_flat, "preconditioned_grad", gradients=True)
    gdt = grads_flat[0].dtype
    gcols = self.grad_columns(self._ptrs(grads_flat), grads_flat[0].element_size())
    self.check_dense([p for p in precs_flat] + [r for r in results if r is not None],
                     "preconditioned_grad")
    x = torch.empty(self.scratch_elems, dtype=torch.float32, device=dev)
    xp = np.uint64(x.data_ptr())
    pp = self._ptrs(precs_flat)
    rp = np.fromiter((0 if r is None else r.data_ptr() for r in results), np.uint64,
                     len(results))
    ta = self.a_tbl.copy()
    if len(ta):
      ta["a"] = gcols["a_a"]
      ta["b"] = pp[self.a_stat]
      ta["c"] = np.where(self.a_c_is_res, rp[self.a_param], xp) + self.a_coff
    sym = self.symmetric_layout(symmetric_precs, gdt)
    # storage of stage A's operands: the gradient is A in the reference orientation, B in the symmetric one
    a_dt, b_dt = (0, DTYPE_CODE[gdt]) if sym else (DTYPE_CODE[gdt], 0)
    if sym:
      vec = ta[self.a_vec_rows]
      sa = self.sa_tbl.copy()
      sa["a"] = pp[self.sa_stat]
      sa["b"] = gcols["sa_b"]
      sa["c"] = xp + self.sa_xoff
      ta = np.concatenate([sa, vec]) if len(vec) else sa
    tb = (self.sb_tbl if sym else self.b_tbl).copy()
    if len(tb):
      tb["a"] = xp + self.b_xoff
      tb["b"] = pp[self.b_stat]
      tb["c"] = rp[self.b_param] + self.b_coff
    r1, r2, r3 = self.rank3_stages(pp, rp, xp)
    if len(r1):
      r1["a"] = gcols["r_a"]
    with torch.cuda.device(dev):
      # stage A (+ rank-3 stage 1) reads the gradients; the later stages float32 intermediates
      for tbl, (sa_dt, sb_dt) in ((_with_rank3(ta, r1), (a_dt, b_dt)), (_with_rank3(tb, r2), (0, 0)),
                                  (r3, (0, 0))):
        if len(tbl) == 0:
          continue
        ws = kernels._workspace(gemm_workspace_bytes(tbl), dev)
        gemm_launch(kernels._stream(), tbl, sa_dt, sb_dt, ws.data_ptr(), ws.numel())
    del x  # the caching allocator keeps it alive until the stream has consumed it

  def rank3_stages(self, pp: np.ndarray, rp: np.ndarray, xp):
    """The three stage tables of the rank-3 blocks with every pointer column filled but stage 1's
    gradient column `a`.  pp / rp: preconditioner and result pointers, xp: the scratch."""
    r1, r2, r3 = self.r1_tbl.copy(), self.r2_tbl.copy(), self.r3_tbl.copy()
    if len(r1):
      x1 = xp + np.uint64(4 * self.x1_start) + self.r_roff
      x2 = x1 + np.uint64(4 * self.r_elems)
      r1["b"], r1["c"] = pp[self.r_stat], x1
      r2["a"], r2["b"], r2["c"] = x1, pp[self.r_stat + 1], x2
      r3["a"], r3["b"], r3["c"] = x2, pp[self.r_stat + 2], rp[self.r_param] + self.r_coff
    return r1, r2, r3


class DonatedStep:
  """The every-step calls of update() on a DONATED state (distributed_shampoo(donate_state=True)):
  the counterpart of the reference's jit-compiled update_fn (DS:3627-3659), which does no per-step
  host work beyond the dispatch.

  The state tensors (statistics, diagonal statistics, both momenta -- float32, or int8 codes and their
  bucket sizes through ps_transform_grads_q8) are updated IN PLACE, the
  preconditioned gradients, the intermediates of the application (X of the two-sided products,
  X1 / X2 of the rank-3 blocks) and the updates live in buffers this object owns, so every pointer
  column of the descriptor tables (Gram update, application stages A, B and -- rank-3 blocks -- C,
  _transform_grad) is filled ONCE per binding; a step patches only the gradient (and, with weight
  decay, parameter) columns when those pointers moved, and issues the same launches as the
  functional path.  No torch.empty, no per-tensor Python
  objects, no pytree rebuilt: the caller gets the same state objects back.

  Bound to one list of ParameterStats objects (identity is checked each step: a state the caller
  rebuilt, or the one a recompute step returned, is simply bound again)."""

  def __init__(self, plan: TreePlan, has_diag: bool, use_params: bool):
    self.plan = plan
    self.has_diag = has_diag
    self.use_params = use_params
    self.objs = None
    self.gp = None
    self.pp_params = None

  def bound_to(self, stats_flat) -> bool:
    objs = self.objs
    return (objs is not None and len(objs) == len(stats_flat) and
            all(a is b for a, b in zip(objs, stats_flat)))

  def bind(self, stats_flat, grads_flat, params_flat, symmetric_precs: bool):
    pl = self.plan
    dev = pl.check_dense(grads_flat, "update (donated state)", gradients=True)
    self.gdtype = grads_flat[0].dtype
    stats = [s for st in stats_flat for s in st.statistics]
    precs = [p for st in stats_flat for p in st.preconditioners]
    moms = [st.momentum.quantized for st in stats_flat]
    dmoms = [st.diagonal_momentum.quantized for st in stats_flat]
    diags = [st.diagonal_statistics.quantized for st in stats_flat] if self.has_diag else []
    if len(stats) != len(pl.stat_dims) or len(precs) != len(pl.stat_dims):
      return False
    # int8 momenta (best_effort_memory_usage_reduction): codes + bucket sizes, updated where they lie
    quant = [m.dtype == torch.int8 for m in moms]
    if any((d.dtype == torch.int8) != q for d, q in zip(dmoms, quant)):
      return False
    qidx = [i for i, q in enumerate(quant) if q]
    mbuckets = [stats_flat[i].momentum.bucket_size for i in qidx]
    dbuckets = [stats_flat[i].diagonal_momentum.bucket_size for i in qidx]
    for i, mb, db in zip(qidx, mbuckets, dbuckets):
      cols = kernels._as_rows_cols(moms[i].shape)[1]
      if (not moms[i].is_cuda or not moms[i].is_contiguous() or not dmoms[i].is_contiguous() or
          moms[i].numel() != pl.numel[i] or dmoms[i].numel() != pl.numel[i] or
          (pl.numel[i] and (mb.numel() != cols or db.numel() != cols))):
        return False
    pl.check_dense(stats + precs + [m for m, q in zip(moms, quant) if not q] +
                   [m for m, q in zip(dmoms, quant) if not q] + mbuckets + dbuckets + diags,
                   "update (donated state)")
    n = pl.n_params
    self.dev = dev
    # buffers owned by the step (valid until the next update call)
    if getattr(self, "upd", None) is None or self.upd[0].dtype != self.gdtype:
      self.upd = [torch.empty_like(g) for g in grads_flat]       # the gradient's dtype
    if getattr(self, "pg", None) is None:
      # float32 whatever the gradient's dtype (empty_like(g) would make them bfloat16)
      self.pg = [None if sk else torch.empty(g.shape, dtype=torch.float32, device=dev)
                 for g, sk in zip(grads_flat, pl.skipped)]
      self.x = torch.empty(pl.scratch_elems, dtype=torch.float32, device=dev)
    sp, prp = pl._ptrs(stats), pl._ptrs(precs)
    rp = np.fromiter((0 if r is None else r.data_ptr() for r in self.pg), np.uint64, n)
    xp = np.uint64(self.x.data_ptr())
    # ---- Gram update, in place ----
    st = pl.stats_tbl.copy()
    st["stat_in"] = sp
    st["stat_out"] = sp
    self.st_tbl = st
    # ---- application ----
    ta = pl.a_tbl.copy()
    ta["b"] = prp[pl.a_stat] if len(ta) else prp[:0]
    ta["c"] = (np.where(pl.a_c_is_res, rp[pl.a_param], xp) + pl.a_coff) if len(ta) else prp[:0]
    self.sym = pl.symmetric_layout(symmetric_precs, self.gdtype)
    gcode = DTYPE_CODE[self.gdtype]
    self.a_dtypes = (0, gcode) if self.sym else (gcode, 0)
    if self.sym:
      vec = ta[pl.a_vec_rows]
      sa = pl.sa_tbl.copy()
      sa["a"] = prp[pl.sa_stat]
      sa["c"] = xp + pl.sa_xoff
      self.n_sa = len(sa)
      self.ta = np.concatenate([sa, vec]) if len(vec) else sa
      tb = pl.sb_tbl.copy()
    else:
      self.ta = ta
      tb = pl.b_tbl.copy()
    if len(tb):
      tb["a"] = xp + pl.b_xoff
      tb["b"] = prp[pl.b_stat]
      tb["c"] = rp[pl.b_param] + pl.b_coff
    # rank-3 blocks: stage 1 behind the rows of stage A, stage 2 behind stage B, stage 3 on its own
    r1, r2, self.tc = pl.rank3_stages(prp, rp, xp)
    self.n_a = len(self.ta)
    self.ta = _with_rank3(self.ta, r1)
    self.tb = _with_rank3(tb, r2)
    # ---- _transform_grad, in place ----
    self.q8 = bool(qidx)
    self.tdesc = kernels.TransformQ8Desc if self.q8 else kernels.TransformDesc
    tt = np.zeros(n, kernels._TQDESC_DT if self.q8 else kernels._TDESC_DT)
    tt["pgrad"] = rp
    mp, dp = pl._ptrs(moms), pl._ptrs(dmoms)
    if self.q8:
      isq = np.array(quant)
      zero = np.uint64(0)
      tt["cols"] = [kernels._as_rows_cols(m.shape)[1] if q else 0 for m, q in zip(moms, quant)]
      for name, codes, buckets in (("mom", mp, mbuckets), ("dmom", dp, dbuckets)):
        bp = np.zeros(n, np.uint64)
        bp[qidx] = pl._ptrs(buckets)
        tt[name + "_codes_in"] = tt[name + "_codes_out"] = np.where(isq, codes, zero)
        tt[name + "_bucket_in"] = tt[name + "_bucket_out"] = bp
      mp, dp = np.where(isq, zero, mp), np.where(isq, zero, dp)
    tt["mom_in"] = mp; tt["mom_out"] = mp
    tt["dmom_in"] = dp; tt["dmom_out"] = dp
    if self.has_diag:
      gp_ = pl._ptrs(diags)
      tt["diag_in"] = gp_; tt["diag_out"] = gp_
    tt["upd_out"] = pl._ptrs(self.upd)
    tt["numel"] = pl.numel
    self.tt = tt
    L = lib()
    with torch.cuda.device(dev):
      def ws_for(nbytes):
        return torch.empty((max(int(nbytes), 256),), dtype=torch.uint8, device=dev)
      self.ws_stats = ws_for(L.ps_stats_update_grouped_workspace_bytes(
          C.cast(self.st_tbl.ctypes.data, C.POINTER(StatsDesc)), len(self.st_tbl))) if len(self.st_tbl) else None
      self.ws_a, self.ws_b, self.ws_c = (ws_for(gemm_workspace_bytes(t)) if len(t) else None
                                         for t in (self.ta, self.tb, self.tc))
      tt_probe = self.tt.copy()
      tt_probe["grad"] = tt_probe["upd_out"]   # sizes only
      ws_bytes = L.ps_transform_grads_q8_workspace_bytes if self.q8 else L.ps_transform_grads_workspace_bytes
      self.ws_t = ws_for(ws_bytes(C.cast(tt_probe.ctypes.data, C.POINTER(self.tdesc)), n))
    self.objs = list(stats_flat)
    self.gp = None
    self.pp_params = None
    return True

  def qualifies(self, grads_flat, params_flat) -> bool:
    """Checked on EVERY step, before the pointer comparison: the raw-pointer tables read a gradient as a
    contiguous tensor of the bound shape and dtype (float32 or bfloat16, one for the whole tree).  A
    tensor with the same data_ptr and shape but other strides (a `.t()` view of a square weight, an
    expanded tensor) or another dtype must not reach them; such a step takes the functional path (which
    copies / converts), it does not raise.  Parameters (read with weight decay only) are uniformly
    float32 or uniformly bfloat16, independently of the gradients."""
    for g, u in zip(grads_flat, self.upd):
      if (g.dtype != self.gdtype or not g.is_contiguous() or g.device != self.dev or
          g.shape != u.shape):
        return False
    if self.use_params:
      pdt = uniform_dtype(params_flat)
      if pdt is None:
        return False
      for p_, u in zip(params_flat, self.upd):
        if not p_.is_contiguous() or p_.device != self.dev or p_.shape != u.shape:
          return False
    return True

  def _patch_grads(self, grads_flat):
    pl = self.plan
    gp = pl._ptrs(grads_flat)
    if self.gp is not None and np.array_equal(gp, self.gp):
      return
    self.gp = gp
    cols = pl.grad_columns(gp, self.upd[0].element_size())
    if len(self.st_tbl):
      self.st_tbl["g"] = cols["st_g"]
    if self.sym:
      self.ta["b"][:self.n_sa] = cols["sa_b"]
      if self.n_a > self.n_sa:         # (float32 gradients only: symmetric_layout)
        self.ta["a"][self.n_sa:self.n_a] = cols["a_a"][pl.a_vec_rows]
    elif self.n_a:
      self.ta["a"][:self.n_a] = cols["a_a"]
    if len(self.ta) > self.n_a:
      self.ta["a"][self.n_a:] = cols["r_a"]
    self.tt["grad"] = gp

  def step(self, grads_flat, params_flat, cfg, do_stats: bool, w1: float, w2: float):
    """Enqueues the step; returns the update tensors (owned by this object)."""
    self._patch_grads(grads_flat)    # (the caller checked qualifies() for this step)
    gcode, pcode = DTYPE_CODE[self.gdtype], 0
    if self.use_params:
      pcode = DTYPE_CODE[params_flat[0].dtype]
      pp = self.plan._ptrs(params_flat)
      if self.pp_params is None or not np.array_equal(pp, self.pp_params):
        self.pp_params = pp
        self.tt["param"] = pp
    L = lib()
    stream = kernels._stream()
    with torch.cuda.device(self.dev):
      if do_stats and len(self.st_tbl):
        rc = L.ps_stats_update_grouped_typed(stream, C.cast(self.st_tbl.ctypes.data, C.POINTER(StatsDesc)),
                                             len(self.st_tbl), gcode, float(w1), float(w2),
                                             self.ws_stats.data_ptr(), self.ws_stats.numel())
        check(rc, "ps_stats_update_grouped_typed")
      for tbl, ws, (a_dt, b_dt) in ((self.ta, self.ws_a, self.a_dtypes), (self.tb, self.ws_b, (0, 0)),
                                    (self.tc, self.ws_c, (0, 0))):
        if len(tbl):
          gemm_launch(stream, tbl, a_dt, b_dt, ws.data_ptr(), ws.numel())
      c = kernels.TransformConfig()
      for k, v in cfg.items():
        setattr(c, k, v)
      transform = L.ps_transform_grads_q8 if self.q8 else L.ps_transform_grads_typed
      rc = transform(stream, C.cast(self.tt.ctypes.data, C.POINTER(self.tdesc)),
                     self.plan.n_params, C.byref(c), gcode, pcode,
                     self.ws_t.data_ptr(), self.ws_t.numel())
      check(rc, "ps_transform_grads_q8" if self.q8 else "ps_transform_grads_typed")
    return self.upd
