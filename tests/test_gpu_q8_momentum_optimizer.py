"""best_effort_memory_usage_reduction through the public optimizer with the int8 momentum read and
written where it lies (ps_transform_grads_q8): the functional path, and donate_state=True.

The reference goldens bound both paths with the tolerances of
test_e2e_quantized_state_hip_vs_reference_golden; donated and functional runs are compared bit for
bit; the donated run must hand back the state it was given.
"""
import os

import numpy as np
import pytest
import torch

import precondition_amd as pa
from tests.test_gpu_parity import GOLD, e2e_index
from tests.test_optimizer_host_logic import check_final_state, check_momentum, run_e2e_case

pytestmark = pytest.mark.gpu

_CASES = e2e_index(GOLD, "e2e_quant_index.json")
_MOMENTUM_ONLY = [c for c in _CASES if not c.get("batch_axis")]
_BATCH_AXIS = [c for c in _CASES if c.get("batch_axis")]
TREE = "tree_a_q_momentum_only"   # parameters of rank 2, 1, 3, 2 with recorded gradients for 6 steps


def _z():
  return np.load(os.path.join(GOLD, "e2e_quant.npz"))


@pytest.mark.parametrize("donate", [False, True], ids=["functional", "donated"])
@pytest.mark.parametrize("case", _MOMENTUM_ONLY, ids=lambda c: c["name"])
def test_int8_momentum_kernel_path_vs_reference_golden(case, donate, device):
  assert case["kwargs"]["best_effort_memory_usage_reduction"]
  z = _z()
  st, worst = run_e2e_case(case, z, device, None, extra_kwargs=dict(donate_state=donate))
  assert worst < 6e-3, worst
  check_final_state(case, z, st)
  check_momentum(case, z, st)


def _tree(z, device, gdtype, steps):
  n = 4
  params = tuple(torch.tensor(z[f"{TREE}__param{i}"], device=device) for i in range(n))
  grads = [tuple(torch.tensor(z[f"{TREE}__grad{i}_t{t % 6}"], device=device).to(gdtype) for i in range(n))
           for t in range(steps)]
  return params, grads


def _optimizer(donate, compute_steps=2, **kw):
  # the [70, 33] parameter is skipped (a dimension above 60): grafting update only
  return pa.distributed_shampoo(0.1, 32, preconditioning_compute_steps=compute_steps,
                                start_preconditioning_step=2, skip_preconditioning_dim_size_gt=60,
                                best_effort_memory_usage_reduction=True, donate_state=donate, **kw)


def _leaves(st):
  return [x for x in pa.pytree.tree_leaves(st) if isinstance(x, torch.Tensor)]


def _bits_equal(a, b):
  if a.dtype != b.dtype or a.shape != b.shape:
    return False
  if a.dtype in (torch.float32, torch.int32):
    return torch.equal(a.view(torch.int32).cpu(), b.view(torch.int32).cpu())
  if a.dtype == torch.bfloat16:
    return torch.equal(a.view(torch.int16).cpu(), b.view(torch.int16).cpu())
  return torch.equal(a.cpu(), b.cpu())


@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-3])
@pytest.mark.parametrize("graft", [pa.GraftingType.SGD, pa.GraftingType.ADAGRAD,
                                   pa.GraftingType.RMSPROP_NORMALIZED], ids=lambda g: g.name)
def test_donated_int8_momentum_equals_functional_bit_for_bit(graft, weight_decay, gdtype, device):
  z = _z()
  params, grads = _tree(z, device, gdtype, 6)
  runs = []
  for donate in (False, True):
    opt = _optimizer(donate, graft_type=graft, weight_decay=weight_decay)
    runs.append([opt, opt.init(params)])
  assert runs[1][1].stats[0].momentum.quantized.dtype == torch.int8      # rank 2
  assert runs[1][1].stats[1].momentum.quantized.dtype == torch.float32   # rank 1
  assert runs[1][1].stats[2].momentum.quantized.dtype == torch.int8      # rank 3
  for t, g in enumerate(grads):
    upds = []
    for run in runs:
      upd, run[1] = run[0].update(g, run[1], params)
      upds.append(upd)
    for i, (a, b) in enumerate(zip(*upds)):
      assert a.dtype == gdtype
      assert _bits_equal(a, b), f"step {t}: update {i} differs"
    la, lb = _leaves(runs[0][1]), _leaves(runs[1][1])
    assert len(la) == len(lb)
    for i, (a, b) in enumerate(zip(la, lb)):
      assert _bits_equal(a, b), f"step {t}: state leaf {i} ({a.dtype}, {tuple(a.shape)}) differs"


def test_donated_int8_momentum_state_is_updated_where_it_lies(device):
  """On the steps without a root recompute the donated run hands back the ParameterStats objects
  it was given, with the same code and bucket-size tensors, and holds no more memory after the
  step than before it.  (The first such step after a recompute binds the plan to the new state
  objects and swaps the step's own buffers, so the memory comparison is made on the steps that
  find the plan bound; identity and pointers are checked on every one.)"""
  z = _z()
  steps, every = 8, 4
  params, grads = _tree(z, device, torch.float32, steps)
  opt = _optimizer(True, compute_steps=every, graft_type=pa.GraftingType.RMSPROP_NORMALIZED)
  st = opt.init(params)
  checked = compared = 0
  for t in range(steps):
    before = list(st.stats)
    ptrs = [(s.momentum.quantized.data_ptr(), s.momentum.bucket_size.data_ptr()
             if s.momentum.quantized.dtype == torch.int8 else 0,
             s.diagonal_momentum.quantized.data_ptr(), s.diagonal_momentum.bucket_size.data_ptr()
             if s.diagonal_momentum.quantized.dtype == torch.int8 else 0) for s in before]
    codes0 = before[0].momentum.quantized.clone()
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    upd, st = opt.update(grads[t], st, params)
    torch.cuda.synchronize()
    m1 = torch.cuda.memory_allocated()
    if t % every == 0:
      continue
    checked += 1
    after = list(st.stats)
    assert all(a is b for a, b in zip(after, before)), f"step {t}: new state objects came back"
    now = [(s.momentum.quantized.data_ptr(), s.momentum.bucket_size.data_ptr()
            if s.momentum.quantized.dtype == torch.int8 else 0,
            s.diagonal_momentum.quantized.data_ptr(), s.diagonal_momentum.bucket_size.data_ptr()
            if s.diagonal_momentum.quantized.dtype == torch.int8 else 0) for s in after]
    assert now == ptrs, f"step {t}: momentum tensors moved"
    assert after[0].momentum.quantized.dtype == torch.int8
    assert not torch.equal(after[0].momentum.quantized, codes0), f"step {t}: codes were not updated"
    if t % every >= 2:
      compared += 1
      assert m1 == m0, f"step {t}: {m1 - m0} bytes more are held after the step"
  assert checked == 6 and compared == 4


@pytest.mark.parametrize("case", _BATCH_AXIS[:1], ids=lambda c: c["name"])
def test_int16_second_moment_still_declines_donation(case, device):
  """With a batch axis the statistics and preconditioners are int16: donate_state takes the
  functional path exactly as before, so both runs give the same bits and new state objects."""
  from tests.conftest import single_rank_group
  z = _z()
  group = single_rank_group("nccl")
  ups, states = [], []
  for donate in (False, True):
    u = []
    st, _ = run_e2e_case(case, z, device, None, group=group, extra_kwargs=dict(donate_state=donate),
                         updates_out=u)
    ups.append(u)
    states.append(st)
  for t, (ua, ub) in enumerate(zip(*ups)):
    for i, (a, b) in enumerate(zip(ua, ub)):
      assert _bits_equal(a, b), f"step {t}: update {i} differs"
  for i, (a, b) in enumerate(zip(_leaves(states[0]), _leaves(states[1]))):
    assert _bits_equal(a, b), f"state leaf {i} differs"
  assert states[1].stats[0].statistics[0].quantized.dtype == torch.int16
