"""The tree plan on trees with merged rank-3 parameters (conv kernels, stacked expert weights): the
every-step path -- one grouped Gram launch, three grouped product launches -- computes bit for bit
what the per-block path computes (Preconditioner.preconditioned_grad: a reshape copy, one product
and an allocation per block and axis, then merge_partitions), functional and donated, float32 and
bfloat16.  Every contraction here is shorter than 512, so neither path splits k and both sum every
element in the same order: the comparison is equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TREE = [(96,), (64, 48), (6, 70, 150), (130, 3, 64), ()]
BF = torch.bfloat16


def _opt(pa, block=64, donate=False, best_effort=False, **kw):
  return pa.distributed_shampoo(0.1, block, preconditioning_compute_steps=2, start_preconditioning_step=2,
                                graft_type=pa.GraftingType.RMSPROP_NORMALIZED,
                                skip_preconditioning_rank_lt=1, donate_state=donate,
                                best_effort_shape_interpretation=best_effort, **kw)


def _tensors(seed, shapes, device, dtype=torch.float32):
  rng = np.random.default_rng(seed)
  return [torch.tensor(rng.standard_normal(s).astype(np.float32), device=device).to(dtype) for s in shapes]


def _spy(monkeypatch):
  from precondition_amd.plan import TreePlan
  calls = []
  orig = TreePlan.apply_preconditioners
  def spy(self, *a, **k):
    calls.append(len(self.r1_tbl))
    return orig(self, *a, **k)
  monkeypatch.setattr(TreePlan, "apply_preconditioners", spy)
  return calls


def _run(pa, shapes, device, steps=5, dtype=torch.float32, params=None, **kw):
  params = _tensors(31, shapes, device, dtype) if params is None else params
  opt = _opt(pa, **kw)
  st = opt.init(params)
  ups, kept = [], []
  for t in range(steps):
    grads = _tensors(500 + t, shapes, device, dtype)
    before = st.stats
    u, st = opt.update(grads, st, params)
    ups.append([x.clone() for x in u])     # (a donated step owns its update buffers)
    kept.append(st.stats is before)
  return ups, st, kept


def _assert_same_run(pa, a, b, what):
  (ups_a, st_a, _), (ups_b, st_b, _) = a, b
  for t, (ua, ub) in enumerate(zip(ups_a, ups_b)):
    for i, (x, y) in enumerate(zip(ua, ub)):
      assert x.dtype == y.dtype and torch.equal(x, y), (what, "update", t, i)
  for i, (sa, sb) in enumerate(zip(st_a.stats, st_b.stats)):
    for x, y in zip(sa.statistics, sb.statistics):
      assert torch.equal(x, y), (what, "statistics", i)
    for x, y in zip(sa.preconditioners, sb.preconditioners):
      assert torch.equal(x, y), (what, "preconditioners", i)
    assert torch.equal(sa.momentum.to_float(), sb.momentum.to_float()), (what, "momentum", i)
    assert torch.equal(sa.diagonal_momentum.to_float(), sb.diagonal_momentum.to_float()), (what, i)


@pytest.fixture(scope="module")
def per_block_run(device):
  """The comparison: the same optimizer with no tree plan (five steps, roots recomputed on the even ones)."""
  import precondition_amd as pa
  from precondition_amd.plan import TreePlan
  mp = pytest.MonkeyPatch()
  mp.setattr(TreePlan, "build", staticmethod(lambda *args: None))
  try:
    return _run(pa, TREE, device)
  finally:
    mp.undo()


def test_plan_path_bit_identical_to_per_block_path(device, monkeypatch, per_block_run):
  import precondition_amd as pa
  calls = _spy(monkeypatch)
  got = _run(pa, TREE, device)
  # the plan applied the preconditioners on every step, rank-3 rows included: 1 + 1 + 6 + 3 blocks
  assert len(calls) == 5 and all(n == 9 for n in calls)
  _assert_same_run(pa, got, per_block_run, "plan vs per-block")


def test_donated_state_bit_identical_and_really_in_place(device, per_block_run):
  import precondition_amd as pa
  got = _run(pa, TREE, device, donate=True)
  _assert_same_run(pa, got, per_block_run, "donated vs per-block")
  # roots are recomputed on the even steps; the odd ones are donated steps, which hand the same
  # state objects back
  assert got[2] == [False, True, False, True, False]


@pytest.mark.parametrize("donate", [False, True], ids=["functional", "donated"])
def test_bf16_gradients_and_parameters_equal_the_float32_run_on_promoted_copies(device, donate):
  import precondition_amd as pa
  params = _tensors(31, TREE, device, BF)
  o32, o16 = _opt(pa), _opt(pa, donate=donate)
  p32 = [p.float() for p in params]
  s32, s16 = o32.init(p32), o16.init(params)
  for t in range(5):
    g = _tensors(500 + t, TREE, device, BF)
    u32, s32 = o32.update([x.float() for x in g], s32, p32)
    before = s16.stats
    u16, s16 = o16.update(g, s16, params)
    for i, (a, b) in enumerate(zip(u32, u16)):
      assert b.dtype == BF and torch.equal(b, a.to(BF)), (t, i)
    if donate and t % 2 == 1:
      assert s16.stats is before, f"step {t}: the bf16 rank-3 tree fell back to the functional path"
  _assert_same_run(pa, ([], s32, None), ([], s16, None), "bf16 vs float32")


@pytest.mark.parametrize("shape,best_effort", [((9, 256, 256), False), ((9, 512, 512), True)],
                         ids=["9x256x256_unmerged", "9x512x512_default_merge"])
def test_conv_kernel_with_true_segments_on_both_sides(device, monkeypatch, shape, best_effort):
  """A [3,3,c,c] conv kernel at block_size 128: blocks [9,128,128] cut the middle AND the last axis, so
  stage 1 reads and stage 3 writes true segments.  merge_small_dims (limit 4096) folds (9,256,256) into
  a rank-2 (2304,256), so that shape runs unmerged; (9,512,512) is what the default merge leaves of
  [3,3,512,512].  Contractions are 9 and 128 long: no split-K on either path, equality."""
  import precondition_amd as pa
  from precondition_amd.plan import TreePlan
  shapes = [shape]
  kw = dict(block=128, best_effort=best_effort, steps=4)
  calls = _spy(monkeypatch)
  got = _run(pa, shapes, device, **kw)
  nblk = (shape[1] // 128) * (shape[2] // 128)
  assert calls == [nblk] * 4
  pl = TreePlan.build(*_plan_args(shapes, 128, best_effort))
  assert pl.r1_tbl["m_seg"].all() and pl.r3_tbl["m_seg"].all()
  monkeypatch.setattr(TreePlan, "build", staticmethod(lambda *args: None))
  ref = _run(pa, shapes, device, **kw)
  assert len(calls) == 4
  _assert_same_run(pa, got, ref, "conv kernel")


def _plan_args(shapes, block, best_effort):
  from precondition_amd.blocking import Preconditioner
  pcs = [Preconditioner(torch.empty(s, device="meta"), block, 4096, best_effort) for s in shapes]
  return shapes, pcs, [False] * len(shapes)
