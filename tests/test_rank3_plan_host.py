"""Host side of the tree plan for merged rank-3 parameters (no GPU): TreePlan.build accepts them, and
its descriptor tables -- statistics rows and the three application stage tables -- address exactly
the elements the reference's per-block contractions read and write (DS:1582-1590, 1689-1708).

The tables are checked by a NumPy interpreter that applies element offsets, m_seg, the segment
strides, lda and ldc as include/ps_api.h defines them, over flat float64 buffers holding small
integers: every sum is exact, so the comparison with np.tensordot is equality."""
import hashlib

import numpy as np
import pytest
import torch

from precondition_amd.blocking import Preconditioner
from precondition_amd.plan import TreePlan

BLOCK = 64
RANK3_SHAPES = [(6, 70, 150), (130, 3, 64), (64, 64, 64)]
MIXED_TREE = [(96,), (64, 48), (6, 70, 150), ()]


def _build(shapes, block=BLOCK, best_effort=False):
  skipped = [len(s) < 1 for s in shapes]
  pcs = [None if sk else Preconditioner(torch.empty(s, device="meta"), block, 4096, best_effort)
         for s, sk in zip(shapes, skipped)]
  return TreePlan.build(shapes, pcs, skipped), pcs, skipped


@pytest.mark.parametrize("shapes", [[s] for s in RANK3_SHAPES] + [MIXED_TREE, RANK3_SHAPES],
                         ids=lambda s: "+".join("x".join(map(str, t)) or "scalar" for t in s))
def test_build_accepts_rank3_parameters(shapes):
  pl, pcs, skipped = _build(shapes)
  assert pl is not None
  n3 = sum(len(list(pc._partitioner.partition(torch.empty(pc._transformed_shape, device="meta"))))
           for pc in pcs if pc is not None and len(pc._transformed_shape) == 3)
  assert n3 > 0 and len(pl.r1_tbl) == len(pl.r2_tbl) == len(pl.r3_tbl) == n3
  assert len(pl.stats_tbl) == len(pl.stat_dims) == sum(pl.n_stats_of)


def test_rank4_and_partially_preconditioned_parameters_still_have_no_plan():
  assert _build([(96,), (5, 6, 70, 150)])[0] is None
  from precondition_amd.blocking import PreconditionerType
  shapes = [(6, 70, 150)]
  pc = Preconditioner(torch.empty(shapes[0], device="meta"), BLOCK, 4096, False,
                      preconditioner_type=PreconditionerType.INPUT)
  assert TreePlan.build(shapes, [pc], [False]) is None


# ---- the interpreter ---------------------------------------------------------------------------
def _gemm_rows(tbl, bufs):
  """C = op(A) op(B) for every row of a ps_gemm_desc / ps_gemm_seg_desc table.  The pointer columns
  hold (buffer id << 40) + element offset; bufs[id] is a flat float64 array."""
  seg = "m_seg" in tbl.dtype.names
  for row in tbl:
    (ia, oa), (ib, ob), (ic, oc) = (divmod(int(row[c]), 1 << 40) for c in "abc")
    A, B, Cm = bufs[ia], bufs[ib], bufs[ic]
    m, n, k = int(row["m"]), int(row["n"]), int(row["k"])
    lda, ldb, ldc = int(row["lda"]), int(row["ldb"]), int(row["ldc"])
    m_seg = int(row["m_seg"]) if seg else 0
    if m_seg == 0 or m_seg == m:
      m_seg, a_ss, c_ss = m, 0, 0
    else:
      a_ss, c_ss = int(row["a_seg_stride"]), int(row["c_seg_stride"])
      assert row["transa"] == 1 and m % m_seg == 0
    r = np.arange(m)
    kk = np.arange(k)
    if row["transa"]:
      ai = oa + (r // m_seg)[:, None] * a_ss + kk[None, :] * lda + (r % m_seg)[:, None]
    else:
      ai = oa + r[:, None] * lda + kk[None, :]
    cols = np.arange(n)
    bi = ob + (cols[None, :] * ldb + kk[:, None] if row["transb"] else kk[:, None] * ldb + cols[None, :])
    ci = oc + (r // m_seg)[:, None] * c_ss + (r % m_seg)[:, None] * ldc + cols[None, :]
    assert len(np.unique(ci)) == ci.size          # no element written twice
    Cm[ci] = A[ai] @ B[bi]


def _stats_rows(tbl, bufs):
  """stat_out = sum over segments of X_s X_s^T for every ps_stats_desc row (w1 = 0, w2 = 1)."""
  out = []
  for row in tbl:
    ig, og = divmod(int(row["g"]), 1 << 40)
    g = bufs[ig]
    d, k, nseg, ld, ss = (int(row[c]) for c in ("d", "k", "nseg", "ld", "seg_stride"))
    i, kk = np.arange(d)[:, None], np.arange(k)[None, :]
    acc = np.zeros((d, d))
    for s in range(nseg):
      x = g[og + s * ss + (i * ld + kk if row["layout"] == 0 else kk * ld + i)]
      acc += x @ x.T
    out.append(acc)
  return out


def _tag(buf_id, elem_off=0):
  return np.uint64((buf_id << 40) + elem_off)


def _blocks(pc, t):
  return list(pc._partitioner.partition(t))


@pytest.mark.parametrize("shapes", [[s] for s in RANK3_SHAPES] + [MIXED_TREE, [(9, 256, 256)]],
                         ids=lambda s: "+".join("x".join(map(str, t)) or "scalar" for t in s))
def test_stage_tables_compute_the_chain_of_tensordots_exactly(shapes):
  block = 128 if shapes == [(9, 256, 256)] else BLOCK
  pl, pcs, skipped = _build(shapes, block)
  assert pl is not None
  rng = np.random.default_rng(3)
  n = len(shapes)
  grads = [rng.integers(-3, 4, size=s).astype(np.float64) for s in shapes]
  precs = [rng.integers(-2, 3, size=(int(d), int(d))).astype(np.float64) for d in pl.stat_dims]
  # buffers: gradient i -> id 1 + i, result i -> 1 + n + i, preconditioner j -> 1 + 2n + j, scratch -> 0
  scratch = np.full(pl.scratch_elems, np.nan)
  results = [np.full(g.size, np.nan) for g in grads]
  bufs = {0: scratch}
  for i in range(n):
    bufs[1 + i] = grads[i].reshape(-1)
    bufs[1 + n + i] = results[i]
  for j, p in enumerate(precs):
    bufs[1 + 2 * n + j] = p.reshape(-1)
  gp = np.array([_tag(1 + i) for i in range(n)], np.uint64)
  rp = np.array([_tag(1 + n + i) for i in range(n)], np.uint64)
  pp = np.array([_tag(1 + 2 * n + j) for j in range(len(precs))], np.uint64)
  cols = pl.grad_columns(gp, 1)            # offsets in elements
  # float32 offset columns are bytes: the interpreter's buffers count elements
  def el(col):
    assert np.all(col % np.uint64(4) == 0)
    return col // np.uint64(4)
  xp = _tag(0)
  ta, tb = pl.a_tbl.copy(), pl.b_tbl.copy()
  if len(ta):
    ta["a"], ta["b"] = cols["a_a"], pp[pl.a_stat]
    ta["c"] = np.where(pl.a_c_is_res, rp[pl.a_param], xp) + el(pl.a_coff)
  if len(tb):
    tb["a"], tb["b"], tb["c"] = xp + el(pl.b_xoff), pp[pl.b_stat], rp[pl.b_param] + el(pl.b_coff)
  # rank3_stages adds byte offsets to the scratch pointer: give it a zero base and add the tag after
  r1, r2, r3 = pl.rank3_stages(pp, rp, np.uint64(0))
  r1["a"] = cols["r_a"]
  r1["c"] = xp + el(r1["c"])
  r2["a"], r2["c"] = xp + el(r2["a"]), xp + el(r2["c"])
  r3["a"] = xp + el(r3["a"])
  r3["c"] = rp[pl.r_param] + el(pl.r_coff)
  for tbl in (ta, r1, tb, r2, r3):
    _gemm_rows(tbl, bufs)
  k = 0
  for i, (shape, pc, sk) in enumerate(zip(shapes, pcs, skipped)):
    if sk:
      assert np.all(np.isnan(results[i]))
      continue
    tshape = pc._transformed_shape
    want = np.empty(tshape)
    for gb, wb in zip(_blocks(pc, torch.from_numpy(grads[i].reshape(tshape))),
                      _blocks(pc, torch.from_numpy(want))):
      x = gb.numpy()
      for _ in range(len(tshape)):
        x = np.tensordot(x, precs[k], axes=[[0], [0]])
        k += 1
      wb.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    assert np.array_equal(results[i].reshape(tshape), want), shape
  assert k == len(precs)


@pytest.mark.parametrize("shapes", [[s] for s in RANK3_SHAPES] + [MIXED_TREE],
                         ids=lambda s: "+".join("x".join(map(str, t)) or "scalar" for t in s))
def test_statistics_rows_compute_the_gram_of_every_axis_exactly(shapes):
  pl, pcs, skipped = _build(shapes)
  rng = np.random.default_rng(4)
  grads = [rng.integers(-3, 4, size=s).astype(np.float64) for s in shapes]
  bufs = {1 + i: g.reshape(-1) for i, g in enumerate(grads)}
  tbl = pl.stats_tbl.copy()
  tbl["g"] = pl.grad_columns(np.array([_tag(1 + i) for i in range(len(shapes))], np.uint64), 1)["st_g"]
  got = _stats_rows(tbl, bufs)
  k = 0
  for i, (pc, sk) in enumerate(zip(pcs, skipped)):
    if sk:
      continue
    tshape = pc._transformed_shape
    for gb in _blocks(pc, torch.from_numpy(grads[i].reshape(tshape))):
      x = gb.numpy()
      for axis in range(x.ndim):
        rest = [a for a in range(x.ndim) if a != axis]
        want = np.tensordot(x, x, axes=(rest, rest)) if rest else np.outer(x, x)
        assert np.array_equal(got[k], want), (tshape, axis)
        assert int(tbl["lds"][k]) == x.shape[axis]
        k += 1
  assert k == len(got)


def test_rows_collapse_to_plain_matrices_where_the_block_spans_the_axis():
  """(130, 3, 64) at block 64: every block spans the middle and the last axis, so no row is segmented;
  (6, 70, 150) cuts both, so its interior blocks are segmented on both sides."""
  pl, _, _ = _build([(130, 3, 64)])
  assert not pl.r1_tbl["m_seg"].any() and not pl.r3_tbl["m_seg"].any()
  pl, _, _ = _build([(6, 70, 150)])
  assert pl.r1_tbl["m_seg"].all() and set(pl.r1_tbl["a_seg_stride"]) == {150}
  assert pl.r3_tbl["m_seg"].all() and set(pl.r3_tbl["c_seg_stride"]) == {70 * 150}
  assert not pl.r2_tbl["m_seg"].any()


# ---- trees without rank-3 leaves: the tables of the parent commit -----------------------------------
_RANK2_TREE = [(96,), (64, 48), (200, 72), (3, 4, 40), (130,), (), (5000, 8)]
# sha256 over the tables TreePlan.build made for _RANK2_TREE before rank-3 rows existed
_RANK2_DIGEST = "aa6845bb704633d570ef0abdb1c1c3bb0005d5346b92e3881edc21a513ef74d0"
_RANK2_ATTRS = ("stats_tbl", "st_param", "st_goff", "stat_dims", "a_tbl", "a_param", "a_goff", "a_stat",
                "a_c_is_res", "a_coff", "b_tbl", "b_param", "b_stat", "b_xoff", "b_coff", "sa_tbl", "sb_tbl",
                "sa_param", "sa_goff", "sa_stat", "sa_xoff", "a_vec_rows")


def _plan_digest(pl):
  h = hashlib.sha256()
  for name in _RANK2_ATTRS:
    v = getattr(pl, name)
    h.update(name.encode())
    h.update(str(v.dtype.descr).encode() if v.dtype.names else str(v.dtype).encode())
    h.update(np.ascontiguousarray(v).tobytes())
  h.update(repr((pl.x_elems, pl.numel, pl.n_stats_of, [tuple(t) for t in pl.tshapes], pl.skipped)).encode())
  return h.hexdigest()


def test_tables_of_a_tree_without_rank3_leaves_are_unchanged():
  skipped = [len(s) < 1 or any(d > 4096 for d in s) for s in _RANK2_TREE]
  pcs = [None if sk else Preconditioner(torch.empty(s, device="meta"), 64, 4096, True)
         for s, sk in zip(_RANK2_TREE, skipped)]
  pl = TreePlan.build(_RANK2_TREE, pcs, skipped)
  assert _plan_digest(pl) == _RANK2_DIGEST
  assert len(pl.r1_tbl) == 0 and pl.r_elems == 0 and pl.scratch_elems == max(pl.x_elems, 1)
