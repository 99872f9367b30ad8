"""Pins the references that test_gpu_every_step_exact.py compares the every-step kernels with.
Runs without a GPU.

* `_exact.transform_ref64` (NumPy float64, written from include/ps_api.h and DS:3496-3625)
  against the package's torch float32 restatement `_transform_grad`, which the reference's
  goldens pin (test_optimizer_host_logic.py).  The float64 reference of the GPU tests is thereby
  tied to the reference implementation and not to the kernel.
* the test-side restatement of the split-K heuristic still produces the split counts and
  remainders the GPU case list relies on.
* every integer case satisfies the exactness precondition max(|A| @ |B|) < 2^24.
"""
import numpy as np
import pytest
import torch

from tests import _exact as E
from tests import cpu_backend


class _RecordingBackend:
  """tests/cpu_backend.py (no fused transform: the optimizer takes its torch restatement of
  _transform_grad) that remembers the outputs of the grouped products, i.e. the
  preconditioned gradients the restatement is handed."""

  def __init__(self):
    self.calls = []

  def __getattr__(self, name):
    return getattr(cpu_backend, name)

  def gemm_grouped(self, items):
    cpu_backend.gemm_grouped(items)
    self.calls.append([it[2] for it in items])


def _whole_storage(t):
  return torch.empty(0, dtype=torch.float32).set_(t.untyped_storage())


def _recorded_pgrads(calls, shapes, skipped):
  """The preconditioned gradient of every parameter from the two grouped calls of one update
  (stage a: X = g^T P_L, or the whole product of a vector block; stage b: Y = X^T P_R written
  into blocks of the merged gradient).  Blocks of one parameter share one storage."""
  assert len(calls) == 2
  vec, mat = [], []
  for c in calls[0]:
    if c.shape[0] == 1:
      vec.append(c)
  mat = list(calls[1])
  out = []
  for shape, sk in zip(shapes, skipped):
    if sk:
      out.append(None)
      continue
    pool = vec if len(shape) == 1 else mat
    assert pool, "no recorded product for a preconditioned parameter"
    ptr = pool[0].untyped_storage().data_ptr()
    whole = _whole_storage(pool[0])
    while pool and pool[0].untyped_storage().data_ptr() == ptr:
      pool.pop(0)
    assert whole.numel() == int(np.prod(shape)), (whole.numel(), shape)
    out.append(whole.clone().numpy())
  assert not vec and not mat
  return out


VARIANTS = [
    dict(),
    dict(weight_decay=0.01, nesterov=False, moving_average_for_momentum=True, beta2=0.9,
         clip_by_scaled_gradient_norm=0.3),
    dict(weight_decay=0.02, decoupled_weight_decay=True, decoupled_learning_rate=False, beta1=0.8),
]


def variant_cfg(graft, variant, run_shampoo, lr=0.05):
  """ps_transform_config of the optimizer options of VARIANTS[variant] (the defaults of
  distributed_shampoo: beta1 0.9, beta2 0.999, diagonal_epsilon 1e-10, Nesterov on)."""
  kw = VARIANTS[variant]
  beta2 = kw.get("beta2", 0.999)
  return E.make_cfg(
      graft_type=graft, nesterov=int(kw.get("nesterov", True)),
      moving_average_for_momentum=int(kw.get("moving_average_for_momentum", False)),
      decoupled_learning_rate=int(kw.get("decoupled_learning_rate", True)),
      decoupled_weight_decay=int(kw.get("decoupled_weight_decay", False)),
      run_shampoo=int(run_shampoo), beta1=kw.get("beta1", 0.9), beta2_w1=beta2,
      beta2_w2=beta2 if beta2 == 1.0 else 1.0 - beta2, diagonal_epsilon=1e-10,
      weight_decay=kw.get("weight_decay", 0.0), lr=lr,
      clip_by_scaled_gradient_norm=kw.get("clip_by_scaled_gradient_norm", 0.0) or 0.0)


def _diag_np(state):
  d = state.diagonal_statistics.to_float()
  return d.numpy().copy() if isinstance(d, torch.Tensor) and d.numel() else None


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("graft", [0, 1, 2, 3, 4, 5, 6])
def test_transform_ref64_matches_the_torch_restatement(graft, variant):
  """Every output of the float32 torch restatement lies within 32 u * magnitude of the float64
  restatement: the restatement rounds each of its ~12 elementwise operations once (<= 1 u of
  the magnitude each), its two or three norms are torch's pairwise float32 sums (a few u), and
  its momentum weight is float32(1 - beta1) where the float64 form starts from the float32
  beta1 of ps_transform_config (4 u of one addend at beta1 = 0.9)."""
  import precondition_amd as pa
  import inspect
  rng = np.random.default_rng(100 * graft + variant)
  shapes = [(20, 12), (24,), (40, 3), (7,), (1,)]
  kw = dict(graft_type=pa.GraftingType(graft), start_preconditioning_step=2,
            preconditioning_compute_steps=2, skip_preconditioning_dim_size_gt=30,
            best_effort_shape_interpretation=False)
  kw.update(VARIANTS[variant])
  defaults = inspect.signature(pa.distributed_shampoo).parameters
  # variant_cfg restates these defaults; a changed default must not silently shift the case
  assert defaults["beta1"].default == 0.9 and defaults["beta2"].default == 0.999
  assert defaults["nesterov"].default is True and defaults["diagonal_epsilon"].default == 1e-10
  assert defaults["decoupled_learning_rate"].default is True
  rec = _RecordingBackend()
  opt = pa.distributed_shampoo(0.05, 8, _backend_for_testing=rec, **kw)
  params = [torch.tensor(rng.standard_normal(s).astype(np.float32)) for s in shapes]
  skipped = [any(d > 30 for d in s) for s in shapes]
  assert any(skipped) and not all(skipped)
  state = opt.init(params)
  worst = 0.0
  for t in range(4):
    grads = [torch.tensor(rng.standard_normal(s).astype(np.float32)) for s in shapes]
    step = int(state.count)
    prev = state.stats
    rec.calls = []
    upd, state = opt.update(grads, state, params)
    pgs = _recorded_pgrads(rec.calls, shapes, skipped)
    items = []
    for g, p, st, pg in zip(grads, params, prev, pgs):
      items.append(dict(grad=g.numpy(), pgrad=pg, param=p.numpy(), diag_in=_diag_np(st),
                        mom_in=st.momentum.to_float().numpy().copy(),
                        dmom_in=st.diagonal_momentum.to_float().numpy().copy()))
      if E.has_diag(graft):
        assert items[-1]["diag_in"] is not None
    cfg = variant_cfg(graft, variant, run_shampoo=step >= 2)
    ref = E.transform_ref64(items, cfg)
    if t >= 2 and graft != 0:
      # the recorded operand is a real preconditioned gradient, not the gradient itself
      assert any(pg is not None and not np.allclose(pg, g.numpy().ravel())
                 for pg, g in zip(pgs, grads))
    for i, (r, u, st) in enumerate(zip(ref, upd, state.stats)):
      got = {"upd": u.numpy(), "mom": st.momentum.to_float().numpy(),
             "dmom": st.diagonal_momentum.to_float().numpy()}
      if "diag" in r:
        got["diag"] = st.diagonal_statistics.to_float().numpy()
      for name, (val, mag) in r.items():
        assert np.isfinite(val).all()
        ratio = E.bound_ratio(got[name], val, mag, 32.0)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (graft, variant, t, i, name, ratio)
  print(f"graft {graft} variant {variant}: worst |f32 - f64| / (32 u magnitude) = {worst:.3f}")


def test_transform_ref64_closed_forms():
  """Hand-computed values: the restatement is not only self-consistent."""
  g = np.array([3.0, -4.0, 0.0])
  pg = np.array([0.0, 6.0, 8.0])
  z = np.zeros(3)
  it = dict(grad=g, pgrad=pg, param=None, diag_in=None, mom_in=z, dmom_in=z)
  lr = float(np.float32(0.05))
  r = E.transform_ref64([it], E.make_cfg(graft_type=E.G_SGD))[0]
  assert np.allclose(r["upd"][0], -pg * (5.0 * lr) / 10.0, rtol=1e-15)
  assert np.allclose(r["dmom"][0], g * lr, rtol=1e-15)
  r = E.transform_ref64([it], E.make_cfg(graft_type=E.G_SQRT_N))[0]
  assert np.allclose(r["upd"][0], -pg * (np.sqrt(2.0) * lr) / 10.0, rtol=1e-15)
  r = E.transform_ref64([it], E.make_cfg(graft_type=E.G_NONE))[0]
  assert np.array_equal(r["upd"][0], -pg)
  it_skip = dict(it, pgrad=None)
  r = E.transform_ref64([it_skip], E.make_cfg(graft_type=E.G_SGD, run_shampoo=0))[0]
  assert np.allclose(r["upd"][0], -g * lr, rtol=1e-15)
  # Adagrad with an empty accumulator: u = g / (|g| + eps), zero where g is zero
  it_d = dict(it, diag_in=z)
  r = E.transform_ref64([it_d], E.make_cfg(graft_type=E.G_ADAGRAD, run_shampoo=0))[0]
  assert np.array_equal(r["diag"][0], g * g)
  assert np.allclose(r["upd"][0], -np.sign(g) * lr, rtol=1e-9)
  # magnitudes dominate the values and are equal to them where nothing cancels
  for val, mag in r.values():
    assert (mag >= np.abs(val) * (1 - 1e-15)).all()
  # momentum + coupled weight decay, Nesterov: by hand
  cfg = E.make_cfg(graft_type=E.G_NONE, beta1=0.5, weight_decay=0.25, nesterov=1)
  it_w = dict(grad=g, pgrad=pg, param=np.array([1.0, 2.0, -4.0]), diag_in=None,
              mom_in=np.array([2.0, 2.0, 2.0]), dmom_in=z)
  r = E.transform_ref64([it_w], cfg)[0]
  sw = pg + 0.25 * it_w["param"]
  smom = 1.0 + sw
  assert np.allclose(r["mom"][0], smom, rtol=1e-15)
  assert np.allclose(r["upd"][0], -(sw + 0.5 * smom), rtol=1e-15)
  assert np.allclose(r["upd"][1], np.abs(pg) + np.abs(0.25 * it_w["param"]) +
                     0.5 * (1.0 + np.abs(pg) + np.abs(0.25 * it_w["param"])), rtol=1e-15)


def test_splitk_restatement_keeps_the_case_list_honest():
  """The single-task case list of the grouped product covers split counts of every remainder
  modulo 4, a last split shorter than kchunk and one that is not a multiple of the 16-deep
  K-tile -- with the heuristic as restated from csrc/misc.hip."""
  plans = E.check_split_list()
  one_tile = {k: E.split_plan(1, k) for k in E.GEMM_KS}
  assert one_tile == {512: (2, 256, 256), 640: (2, 384, 256), 1000: (3, 384, 232),
                      1153: (4, 384, 1), 1800: (5, 384, 264), 4096: (16, 256, 256),
                      4100: (11, 384, 260), 50000: (56, 896, 720)}
  # the last split ends at k: every read of a split stays inside the operand
  for ksplit, kchunk, last in plans:
    assert kchunk % 128 == 0 and 0 < last <= kchunk
  for (m, n) in E.GEMM_MN:
    for k in E.GEMM_KS:
      ksplit, kchunk, last = E.split_plan(E.tiles_of(m, n), k)
      assert (ksplit - 1) * kchunk + last == k
  # both sides of the thresholds
  assert E.splitk_for(511, 4096) == 2 and E.splitk_for(512, 4096) == 1
  assert E.splitk_for(1, 511) == 1 and E.splitk_for(1, 512) == 2
  assert E.splitk_for(256, 2047) == 1 and E.splitk_for(256, 2048) == 2
  assert E.splitk_for(1, 1 << 20) == E.KSPLIT_MAX


def test_integer_cases_are_exact_in_float32():
  """|a|, |b| <= 8 and k <= 50 000: every partial sum is an integer below 2^24."""
  rng = np.random.default_rng(0)
  kmax = max(E.GEMM_KS)
  assert 64 * kmax < E.EXACT_LIMIT
  for salt in range(4):
    a = E.int_operand(rng, 37, kmax, salt)
    b = E.int_operand(rng, kmax, 29, salt + 5)
    assert np.abs(a).max() <= 8 and np.abs(b).max() <= 8
    E.assert_exact(E.product_abs_bound(a, b))
    ref = E.int_matmul(a, b)
    assert np.array_equal(ref, a @ b)   # the float64 BLAS shortcut is the int64 product
    assert np.array_equal(ref.astype(np.float32).astype(np.int64), ref)
  pat = E.int_pattern(40, 40)
  assert not np.array_equal(pat, pat.T) and not np.array_equal(pat[1:], pat[:-1])
  with pytest.raises(AssertionError):
    E.assert_exact(float(E.EXACT_LIMIT))
  # statistics: w1 * old + w2 * G with w in {0, 0.5, 1, 2}, |old| <= 8, k <= 50 000
  assert 2 * 8 + 2 * 64 * 50000 < E.EXACT_LIMIT
  # norm probes: perfect squares below 2^24, distinct counts in the hot chunks
  for n in (1, 4095, 4096, 4097, 8192, 256 * 4096, 256 * 4096 + 1, 1024 * 4096):
    for dense in (True, False):
      for twos in (False, True):
        x, root = E.exact_norm_vector(n, dense, twos)
        assert x.size == n and np.abs(x).max() <= 2 and int(np.sum(x * x)) == root * root
        if not dense:
          per = [int(np.count_nonzero(x[c * E.TCHUNK:(c + 1) * E.TCHUNK])) for c in E.hot_chunks(n)]
          assert all(per), (n, per)
          if n >= 1024 * 4096:
            assert len(set(per)) == len(per), per
  assert E.hot_chunks(1024 * 4096) == [0, 255, 256, 257, 511, 512, 1023]


def test_norm_depth_and_ulp_helpers():
  assert E.norm_depth(1) == 35 and E.norm_depth(4096 * 256) == 35
  assert E.norm_depth(4096 * 256 + 1) == 36 and E.norm_depth(38597376) == 16 + 6 + 3 + 37 + 9
  one = np.float32(1.0)
  assert E.ulp_distance([one], [np.nextafter(one, np.float32(2))])[0] == 1
  assert E.ulp_distance([np.float32(-0.0)], [np.float32(0.0)])[0] == 0
  assert E.ulp_distance([-one], [np.nextafter(-one, np.float32(-2))])[0] == 1
