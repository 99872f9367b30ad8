"""bfloat16 gradients read natively by the every-step kernels (ps_*_typed) and by the optimizer.

A bf16 -> float32 widening is exact, so every check here is bit-identity: the typed entry on bf16
storage against the float32 entry on the widened copy (which earlier files pin), or against an
int64 expectation on inputs that are exact in bf16 and float32.  No tolerance appears in this
file.  Kernel outputs are written into sentinel-framed buffers and the frame is checked.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _exact as E
from tests.test_every_step_references import VARIANTS, variant_cfg

pytestmark = pytest.mark.gpu

SENT = -777.25
F32, BF16 = 0, 1
PS_EUNSUPPORTED = -3
BF = torch.bfloat16


def _lib():
  from precondition_amd import _lib as L
  return L.lib()


def _stream():
  return torch.cuda.current_stream().cuda_stream


def _same(a, b, what):
  """Equal element for element, NaNs compared by position."""
  assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
  if torch.equal(a, b):
    return
  na, nb = torch.isnan(a), torch.isnan(b)
  assert torch.equal(na, nb), f"{what}: NaN positions differ"
  x, y = torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b)
  if not torch.equal(x, y):
    bad = (x != y).nonzero()
    raise AssertionError(f"{what}: {len(bad)} of {a.numel()} elements differ; first at {bad[0].tolist()}")


def _normal_bf16(rng, n, dev):
  return torch.from_numpy(np.asarray(rng.standard_normal(n) * 0.02, np.float32)).to(dev).to(BF)


def _ws(nbytes, dev):
  return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def _framed(m, n, dev, fill=None):
  holder = torch.full((m + 2, n + 3), SENT, dtype=torch.float32, device=dev)
  view = holder[1:m + 1, 2:n + 2]
  if fill is not None:
    view.copy_(fill)
  return holder, view


def _frame_intact(holder, what):
  m, n = holder.shape[0] - 2, holder.shape[1] - 3
  h = holder.clone()
  h[1:m + 1, 2:n + 2] = SENT
  assert bool((h == SENT).all()), f"{what}: wrote outside its output"


# ---------------------------------------------------------------------------
# 1 / 2. statistics
# ---------------------------------------------------------------------------
def _stats_case(buf, off, layout, d, k, nseg, ld, seg):
  return dict(buf=buf, off=off, layout=layout, d=d, k=k, nseg=nseg, ld=ld, seg=seg)


def _stats_cases(dev, make):
  """make(numel) -> bf16 device vector.  The case list of the issue, as (buffer, element offset, desc)."""
  cases = []
  for rows, cols in ((256, 512), (197, 1000)):
    g = make(rows * cols)
    cases.append(_stats_case(g, 0, 0, rows, cols, 1, cols, 0))     # axis 0
    cases.append(_stats_case(g, 0, 1, cols, rows, 1, cols, 0))     # axis 1
  g = make(3 * 130 * 96)                                           # middle axis of [3, 130, 96]
  cases.append(_stats_case(g, 0, 0, 130, 96, 3, 96, 130 * 96))
  for d in (1, 3, 128, 1000):                                      # vector blocks: layout 1, k = 1
    cases.append(_stats_case(make(d), 0, 1, d, 1, 1, d, 0))
  g = make(1 + 64 * 100)                                           # odd element offset: 2-byte aligned only
  cases.append(_stats_case(g, 1, 0, 64, 100, 1, 100, 0))
  cases.append(_stats_case(g, 1, 1, 100, 64, 1, 100, 0))
  g = make(70 * 65)                                                # ld % 4 == 1
  cases.append(_stats_case(g, 0, 0, 70, 61, 1, 65, 0))
  cases.append(_stats_case(g, 0, 1, 61, 70, 1, 65, 0))
  return cases


def _run_stats(cases, gbufs, code, olds, w1, w2, in_place, dev):
  """One grouped call; gbufs[i]: the buffer the gradient of case i is read from (bf16 or its float32
  copy).  Returns the holders of the outputs."""
  from precondition_amd._lib import StatsDesc
  L = _lib()
  n = len(cases)
  descs = (StatsDesc * n)()
  holders, keep = [], []
  for dsc, c, gb, old in zip(descs, cases, gbufs, olds):
    d = c["d"]
    holder, out = _framed(d, d, dev, fill=old if in_place else None)
    if in_place:
      sin = out
    else:
      _, sin = _framed(d, d, dev, fill=old)
      keep.append(sin)
    holders.append(holder)
    dsc.g = gb.data_ptr() + c["off"] * gb.element_size()
    dsc.layout, dsc.d, dsc.k, dsc.nseg = c["layout"], d, c["k"], c["nseg"]
    dsc.ld, dsc.seg_stride = c["ld"], c["seg"]
    dsc.stat_in, dsc.stat_out, dsc.lds = sin.data_ptr(), out.data_ptr(), d + 3
  ws = _ws(L.ps_stats_update_grouped_workspace_bytes(descs, n), dev)
  if code is None:
    rc = L.ps_stats_update_grouped_f32(_stream(), descs, n, w1, w2, ws.data_ptr(), ws.numel())
  else:
    rc = L.ps_stats_update_grouped_typed(_stream(), descs, n, code, w1, w2, ws.data_ptr(), ws.numel())
  assert rc == 0, rc
  torch.cuda.synchronize()
  return holders


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("grouped", [True, False])
def test_stats_typed_equals_float32_on_the_widened_copy(grouped, in_place, device):
  rng = np.random.default_rng(11)
  cases = _stats_cases(device, lambda n: _normal_bf16(rng, n, device))
  olds = [torch.from_numpy(np.asarray(rng.standard_normal((c["d"], c["d"])), np.float32)).to(device)
          for c in cases]
  bufs = [c["buf"] for c in cases]
  wide = [b.float() for b in bufs]
  groups = [list(range(len(cases)))] if grouped else [[i] for i in range(len(cases))]
  for idx in groups:
    sel = lambda xs: [xs[i] for i in idx]
    ref = _run_stats(sel(cases), sel(wide), None, sel(olds), 0.999, 0.001, in_place, device)
    got = _run_stats(sel(cases), sel(bufs), BF16, sel(olds), 0.999, 0.001, in_place, device)
    f32 = _run_stats(sel(cases), sel(wide), F32, sel(olds), 0.999, 0.001, in_place, device)
    for i, r, g, f in zip(idx, ref, got, f32):
      _same(g, r, f"statistics case {i} (bf16)")
      _frame_intact(g, f"statistics case {i}")
      _same(f, r, f"statistics case {i} (typed, float32 code)")


@pytest.mark.parametrize("w1,w2", [(1.0, 1.0), (0.5, 2.0), (2.0, 0.5), (0.0, 1.0), (1.0, 0.0)])
def test_stats_typed_exact_integers(w1, w2, device):
  """Integer gradients |g| <= 8 (exact in bf16), integer `old`: equals the int64 expectation."""
  rng = np.random.default_rng(12)
  ints = {}

  def make(n):
    v = E.int_random(rng, (n,))
    t = torch.from_numpy(v.astype(np.float32)).to(device).to(BF)
    ints[t.data_ptr()] = v
    return t

  cases = _stats_cases(device, make)
  olds_i = [E.int_random(rng, (c["d"], c["d"]), -50, 50) for c in cases]
  olds = [torch.from_numpy(o.astype(np.float32)).to(device) for o in olds_i]
  got = _run_stats(cases, [c["buf"] for c in cases], BF16, olds, w1, w2, False, device)
  for i, (c, o, h) in enumerate(zip(cases, olds_i, got)):
    v = ints[c["buf"].data_ptr()]
    gram = np.zeros((c["d"], c["d"]), np.int64)
    for s in range(c["nseg"]):
      base = c["off"] + s * c["seg"]
      if c["layout"] == 0:
        x = np.stack([v[base + r * c["ld"]: base + r * c["ld"] + c["k"]] for r in range(c["d"])])
      else:
        x = np.stack([v[base + r * c["ld"]: base + r * c["ld"] + c["d"]] for r in range(c["k"])]).T
      gram += E.int_matmul(x, x.T).astype(np.int64)
    E.assert_exact(2 * np.abs(o).max() + 2 * 64 * c["k"] * c["nseg"])
    exp = w1 * o.astype(np.float64) + w2 * gram.astype(np.float64)   # halves are exact
    d = c["d"]
    assert np.array_equal(h[1:d + 1, 2:d + 2].cpu().numpy().astype(np.float64), exp), f"case {i}"
    _frame_intact(h, f"statistics case {i}")


# ---------------------------------------------------------------------------
# 3. grouped product
# ---------------------------------------------------------------------------
GEMM_SHAPES = [(128, 128, 128), (197, 1000, 197), (1000, 197, 1000), (768, 768, 768),
               (1, 3, 3), (1, 768, 768), (1, 1000, 1000)]
SPLITK_SHAPE = (128, 128, 4096)
KINDS = [("a", 1, 0), ("b", 0, 0)]   # (bf16 operand, transa, transb)


def _operands(kind, m, n, k, off, dev, values):
  """Stored operands: (A, B) with the bf16 one `off` elements into its buffer.  values(shape) -> float32
  numpy array exactly representable in bf16."""
  which, transa, _ = kind
  a = values((k, m) if transa else (m, k))
  b = values((k, n))

  def put(x, bf):
    t = torch.from_numpy(x.reshape(-1)).to(dev)
    if not bf:
      return t, 0
    buf = torch.zeros(off + t.numel(), dtype=BF, device=dev)
    buf[off:] = t.to(BF)
    return buf, off
  (ab, ao), (bb, bo) = put(a, which == "a"), put(b, which == "b")
  return a, b, ab, ao, bb, bo


def _run_gemm(tasks, a_dt, b_dt, dev, widen=False, entry="typed"):
  """tasks: dicts(kind, m, n, k, ab, ao, bb, bo).  One grouped call; returns (rc, holders)."""
  from precondition_amd._lib import GemmDesc
  L = _lib()
  n_t = len(tasks)
  descs = (GemmDesc * n_t)()
  holders, keep = [], []
  for dsc, t in zip(descs, tasks):
    _, transa, transb = t["kind"]
    ab, bb = (t["ab"].float(), t["bb"].float()) if widen else (t["ab"], t["bb"])
    keep += [ab, bb]
    holder, c = _framed(t["m"], t["n"], dev)
    holders.append(holder)
    dsc.a = ab.data_ptr() + t["ao"] * ab.element_size()
    dsc.b = bb.data_ptr() + t["bo"] * bb.element_size()
    dsc.c = c.data_ptr()
    dsc.m, dsc.n, dsc.k = t["m"], t["n"], t["k"]
    dsc.transa, dsc.transb = transa, transb
    dsc.lda = t["m"] if transa else t["k"]
    dsc.ldb = t["k"] if transb else t["n"]
    dsc.ldc = t["n"] + 3
  ws = _ws(L.ps_gemm_grouped_workspace_bytes(descs, n_t), dev)
  if entry == "f32":
    rc = L.ps_gemm_grouped_f32(_stream(), descs, n_t, ws.data_ptr(), ws.numel())
  else:
    rc = L.ps_gemm_grouped_typed(_stream(), descs, n_t, a_dt, b_dt, ws.data_ptr(), ws.numel())
  torch.cuda.synchronize()
  return rc, holders


def _gemm_tasks(kind, shapes, dev, values, off):
  tasks = []
  for (m, n, k) in shapes:
    a, b, ab, ao, bb, bo = _operands(kind, m, n, k, off, dev, values)
    tasks.append(dict(kind=kind, m=m, n=n, k=k, a=a, b=b, ab=ab, ao=ao, bb=bb, bo=bo))
  return tasks


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "odd_element_offset"])
@pytest.mark.parametrize("kind", KINDS, ids=["A_bf16_transa", "B_bf16_nn"])
def test_gemm_typed_equals_float32_on_the_widened_copy(kind, off, device):
  rng = np.random.default_rng(21)
  values = lambda shape: np.asarray(rng.standard_normal(shape) * 0.02, np.float32).astype(np.float32)
  bfround = lambda x: torch.from_numpy(x).to(BF).float().numpy()
  tasks = _gemm_tasks(kind, GEMM_SHAPES, device, lambda s: bfround(values(s)), off)
  split = _gemm_tasks(kind, [SPLITK_SHAPE], device, lambda s: bfround(values(s)), off)
  dts = (BF16, F32) if kind[0] == "a" else (F32, BF16)
  calls = [tasks, split] + [[t] for t in tasks]      # one grouped call, the split-K shape alone, singly
  for call in calls:
    rc, ref = _run_gemm(call, F32, F32, device, widen=True, entry="f32")
    assert rc == 0, rc
    rc, got = _run_gemm(call, *dts, device)
    assert rc == 0, rc
    for t, r, g in zip(call, ref, got):
      _same(g, r, f"product {kind} {(t['m'], t['n'], t['k'])} of a call of {len(call)}")


@pytest.mark.parametrize("kind", KINDS, ids=["A_bf16_transa", "B_bf16_nn"])
def test_gemm_typed_exact_integers(kind, device):
  rng = np.random.default_rng(22)
  values = lambda shape: E.int_random(rng, shape).astype(np.float32)
  dts = (BF16, F32) if kind[0] == "a" else (F32, BF16)
  for shapes in (GEMM_SHAPES, [SPLITK_SHAPE]):
    tasks = _gemm_tasks(kind, shapes, device, values, 1)
    rc, got = _run_gemm(tasks, *dts, device)
    assert rc == 0, rc
    for t, h in zip(tasks, got):
      a = (t["a"].T if kind[1] else t["a"]).astype(np.int64)
      b = t["b"].astype(np.int64)
      E.assert_exact(E.product_abs_bound(a, b))
      exp = E.int_matmul(a, b).astype(np.float64)
      m, n = t["m"], t["n"]
      assert np.array_equal(h[1:m + 1, 2:n + 2].cpu().numpy().astype(np.float64), exp), (kind, m, n, t["k"])
      _frame_intact(h, f"product {(m, n, t['k'])}")


@pytest.mark.parametrize("a_dt,b_dt,transa,transb", [
    (BF16, F32, 0, 0), (BF16, F32, 0, 1), (BF16, F32, 1, 1),
    (F32, BF16, 1, 0), (F32, BF16, 0, 1), (F32, BF16, 1, 1),
    (BF16, BF16, 0, 0), (BF16, BF16, 1, 0), (BF16, BF16, 0, 1), (BF16, BF16, 1, 1)])
def test_gemm_typed_unsupported_combinations_write_nothing(a_dt, b_dt, transa, transb, device):
  from precondition_amd._lib import GemmDesc
  L = _lib()
  m = n = k = 128
  a = torch.ones(m * k, dtype=BF if a_dt else torch.float32, device=device)
  b = torch.ones(n * k, dtype=BF if b_dt else torch.float32, device=device)
  holder, c = _framed(m, n, device)
  descs = (GemmDesc * 1)()
  d = descs[0]
  d.a, d.b, d.c, d.m, d.n, d.k = a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k
  d.transa, d.transb, d.lda, d.ldb, d.ldc = transa, transb, 128, 128, n + 3
  ws = _ws(L.ps_gemm_grouped_workspace_bytes(descs, 1), device)
  rc = L.ps_gemm_grouped_typed(_stream(), descs, 1, a_dt, b_dt, ws.data_ptr(), ws.numel())
  torch.cuda.synchronize()
  assert rc == PS_EUNSUPPORTED, rc
  assert bool((holder == SENT).all())


# ---------------------------------------------------------------------------
# 4. transform
# ---------------------------------------------------------------------------
T_NAMES = ("grad", "pgrad", "param", "diag_in", "diag_out", "mom_in", "mom_out", "dmom_in", "dmom_out",
           "upd_out")


def _transform(arrs, cfg, codes, dev):
  """codes None: ps_transform_grads_f32; else (grad_dtype, param_dtype) of the typed entry."""
  from precondition_amd._lib import TransformConfig, TransformDesc
  L = _lib()
  n = len(arrs)
  descs = (TransformDesc * n)()
  for d, a in zip(descs, arrs):
    for name in T_NAMES:
      t = a.get(name)
      setattr(d, name, None if t is None or t.numel() == 0 else t.data_ptr())
    d.numel = a["grad"].numel()
  c = TransformConfig()
  for k, v in cfg.items():
    setattr(c, k, v)
  ws = _ws(L.ps_transform_grads_workspace_bytes(descs, n), dev)
  if codes is None:
    rc = L.ps_transform_grads_f32(_stream(), descs, n, C.byref(c), ws.data_ptr(), ws.numel())
  else:
    rc = L.ps_transform_grads_typed(_stream(), descs, n, C.byref(c), codes[0], codes[1], ws.data_ptr(),
                                    ws.numel())
  assert rc == 0, rc
  torch.cuda.synchronize()


T_SIZES = [1, 3, 4096, 4097, 300000, 0]   # parameter 1 has pgrad == NULL


def _transform_tree(dev, seed):
  rng = np.random.default_rng(seed)
  f32 = lambda n, s=1.0: torch.from_numpy(np.asarray(rng.standard_normal(n) * s, np.float32)).to(dev)
  tree = []
  for i, n in enumerate(T_SIZES):
    tree.append(dict(grad=_normal_bf16(rng, n, dev), pgrad=None if i == 1 else f32(n, 0.02),
                     param=_normal_bf16(rng, n, dev), diag_in=f32(n).abs() * 1e-3,
                     mom_in=f32(n, 0.01), dmom_in=f32(n, 0.01)))
  return tree


def _with_outputs(tree, grad_dt, param_dt, dev):
  arrs = []
  for it in tree:
    n = it["grad"].numel()
    a = dict(it)
    a["grad"], a["param"] = it["grad"].to(grad_dt), it["param"].to(param_dt)
    for name in ("mom_out", "dmom_out", "diag_out"):
      a[name] = torch.full((n + 2,), SENT, device=dev)[1:n + 1]
    a["upd_holder"] = torch.full((n + 2,), SENT, dtype=grad_dt, device=dev)
    a["upd_out"] = a["upd_holder"][1:n + 1]
    arrs.append(a)
  return arrs


@pytest.mark.parametrize("param_dt", [BF, torch.float32], ids=["param_bf16", "param_f32"])
@pytest.mark.parametrize("graft", range(7))
def test_transform_typed_equals_float32_on_the_widened_copy(graft, param_dt, device):
  tree = _transform_tree(device, 31 + graft)
  for variant in range(len(VARIANTS)):
    for run_shampoo in (0, 1):
      cfg = variant_cfg(graft, variant, run_shampoo)
      ref = _with_outputs(tree, torch.float32, torch.float32, device)
      _transform(ref, cfg, None, device)
      got = _with_outputs(tree, BF, param_dt, device)
      _transform(got, cfg, (BF16, BF16 if param_dt == BF else F32), device)
      for i, (r, g) in enumerate(zip(ref, got)):
        what = f"graft {graft} variant {variant} run {run_shampoo} parameter {i}"
        for name in ("mom_out", "dmom_out") + (("diag_out",) if E.has_diag(graft) else ()):
          _same(g[name], r[name], f"{what} {name}")
        assert g["upd_out"].dtype == BF
        _same(g["upd_out"], r["upd_out"].to(BF), f"{what} upd_out")
        h, sent = g["upd_holder"], torch.tensor(SENT).to(BF)   # (the sentinel as bf16 stores it)
        assert bool(h[0] == sent) and bool(h[-1] == sent), f"{what}: update frame"


def test_transform_bf16_update_rounding(device):
  """upd = -mom_in exactly (zero gradient, beta1 = 1, no Nesterov, lr = 1, decoupled learning rate,
  skipped preconditioning): the bf16 store is round-to-nearest-even of the float32 value."""
  bits = [0x3F808000, 0x3F818000,            # ties between bf16 neighbours: even and odd lower neighbour
          0x3F808001, 0x3F807FFF,            # just above / below a tie
          0x7F7F0000,                        # the largest finite bf16
          0x7F7F8000, 0x7F7FFFFF,            # round up to infinity
          0x00000000, 0x80000000,            # +-0
          0x00000001, 0x00008000, 0x80018000,  # subnormals (a tie among them)
          0x7F800000, 0xFF800000, 0x7FC00000]  # +-inf, NaN
  mom = torch.from_numpy(np.array(bits, np.uint32).view(np.float32).copy()).to(device)
  n = mom.numel()
  cfg = E.make_cfg(graft_type=E.G_SGD, nesterov=0, moving_average_for_momentum=0,
                   decoupled_learning_rate=1, decoupled_weight_decay=0, run_shampoo=1, beta1=1.0,
                   weight_decay=0.0, lr=1.0)
  a = dict(grad=torch.zeros(n, dtype=BF, device=device), pgrad=None, param=None, diag_in=None,
           mom_in=mom, dmom_in=torch.zeros(n, device=device),
           mom_out=torch.empty(n, device=device), dmom_out=torch.empty(n, device=device),
           upd_out=torch.full((n,), 3.0, dtype=BF, device=device))
  _transform([a], cfg, (BF16, BF16), device)
  _same(a["upd_out"], (-mom).to(BF), "rounded update")
  _same(a["mom_out"], mom, "momentum")


# ---------------------------------------------------------------------------
# 5 - 8. optimizer
# ---------------------------------------------------------------------------
OPT_SHAPES = [(768, 3072), (197, 64), (768,), (3072,), (64,), (5000, 8)]   # the last one is skipped


def _opt(pa, graft, wd, donate, **kw):
  return pa.distributed_shampoo(0.1, 1024, preconditioning_compute_steps=3, start_preconditioning_step=2,
                                graft_type=graft, weight_decay=wd, donate_state=donate,
                                skip_preconditioning_dim_size_gt=4096, **kw)


def _grads_bf16(t, dev, shapes=OPT_SHAPES):
  r = np.random.default_rng(100 + t)
  return [_normal_bf16(r, s, dev) for s in shapes]


def _state_leaves(pa, st):
  return [x for x in pa.pytree.tree_leaves(st) if isinstance(x, torch.Tensor)]


def _assert_states_equal(pa, a, b, what):
  la, lb = _state_leaves(pa, a), _state_leaves(pa, b)
  assert len(la) == len(lb), what
  for i, (x, y) in enumerate(zip(la, lb)):
    assert x.dtype == y.dtype, (what, i, x.dtype, y.dtype)
    _same(x, y, f"{what}: state leaf {i}")


def _graft_types(pa):
  G = pa.GraftingType
  return [G.SGD, G.RMSPROP_NORMALIZED, G.ADAGRAD]


@pytest.mark.parametrize("wd", [0.0, 1e-3], ids=["no_wd", "wd"])
@pytest.mark.parametrize("gi", range(3))
def test_optimizer_bf16_functional_and_donated_equal_the_float32_run(gi, wd, device):
  """Three optimizers on identical inputs: (i) float32 (the test widens gradients / parameters and
  rounds the updates), (ii) bf16 functional, (iii) bf16 donated.  Updates and every state tensor are
  bit-identical after every step; on the non-recompute steps run (iii) really takes the donated step."""
  import precondition_amd as pa
  graft = _graft_types(pa)[gi]
  rng = np.random.default_rng(5)
  params = [_normal_bf16(rng, s, device) for s in OPT_SHAPES]
  params32 = [p.float() for p in params]
  o1, o2, o3 = _opt(pa, graft, wd, False), _opt(pa, graft, wd, False), _opt(pa, graft, wd, True)
  s1, s2, s3 = o1.init(params32), o2.init(params), o3.init(params)
  for t in range(7):
    g = _grads_bf16(t, device)
    u1, s1 = o1.update([x.float() for x in g], s1, params32)
    u2, s2 = o2.update(g, s2, params)
    before = s3.stats
    ptrs = [x.data_ptr() for x in _state_leaves(pa, s3.stats) if x.is_cuda and x.numel()]
    u3, s3 = o3.update(g, s3, params)
    for i, (a, b, c) in enumerate(zip(u1, u2, u3)):
      assert b.dtype == BF and c.dtype == BF, (t, i, b.dtype, c.dtype)
      _same(b, a.to(BF), f"step {t} update {i} (functional)")
      _same(c, a.to(BF), f"step {t} update {i} (donated)")
    _assert_states_equal(pa, s1, s2, f"step {t} functional")
    _assert_states_equal(pa, s1, s3, f"step {t} donated")
    for x in _state_leaves(pa, s3):
      assert x.dtype != BF
    if t % 3 != 0:   # no root recompute: the donated step was taken (state objects and storage kept)
      assert s3.stats is before, f"step {t}: bf16 gradients fell through to the functional path"
      assert ptrs == [x.data_ptr() for x in _state_leaves(pa, s3.stats) if x.is_cuda and x.numel()]


def test_donated_bf16_step_allocates_no_more_than_float32(device):
  import precondition_amd as pa
  rng = np.random.default_rng(6)
  params = [_normal_bf16(rng, s, device) for s in OPT_SHAPES]
  extra = {}
  for name, conv in (("float32", lambda x: x.float()), ("bf16", lambda x: x)):
    prm = [conv(p) for p in params]
    opt = _opt(pa, pa.GraftingType.RMSPROP_NORMALIZED, 1e-3, True)
    st = opt.init(prm)
    grads = [[conv(x) for x in _grads_bf16(t, device)] for t in range(3)]
    for t in range(2):                      # step 0 recomputes, step 1 is the warm-up donated step
      _, st = opt.update(grads[t], st, prm)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    before = st.stats
    _, st = opt.update(grads[2], st, prm)
    torch.cuda.synchronize()
    assert st.stats is before
    extra[name] = torch.cuda.max_memory_allocated() - base
  print("transient bytes of a donated step:", extra)
  assert extra["bf16"] <= extra["float32"], extra


def test_fallbacks_still_promote(device):
  """fp16, mixed dtypes, a strided bf16 gradient and a dtype switch under donate_state: no exception,
  updates in each gradient's dtype, equal to the float32 run after the same rounding."""
  import precondition_amd as pa
  shapes = [(256, 256), (256,)]
  rng = np.random.default_rng(7)
  params = [torch.from_numpy(np.asarray(rng.standard_normal(s) * 0.02, np.float32)).to(device) for s in shapes]
  G = pa.GraftingType.RMSPROP_NORMALIZED

  def base_grads(t):
    return _grads_bf16(t, device, shapes)

  def variants(t):
    g = base_grads(t)
    sq_t = g[0].float().t().contiguous().to(BF)   # storage of the transposed matrix
    return {
        "fp16": [x.to(torch.float16) for x in g],
        "mixed": [g[0].float(), g[1]],
        "strided": [sq_t.t(), g[1]],
        "switch": [x if t % 2 == 0 else x.float() for x in g],
    }

  for name in ("fp16", "mixed", "strided", "switch"):
    for donate in (False, True):
      o_ref, o = _opt(pa, G, 1e-3, False), _opt(pa, G, 1e-3, donate)
      s_ref, s = o_ref.init(params), o.init(params)
      for t in range(5):
        g = variants(t)[name]
        if name == "strided":
          assert not g[0].is_contiguous()
        u_ref, s_ref = o_ref.update([x.float().contiguous() for x in g], s_ref, params)
        u, s = o.update(g, s, params)
        for i, (a, b, x) in enumerate(zip(u_ref, u, g)):
          assert b.dtype == x.dtype, (name, donate, t, i, b.dtype, x.dtype)
          _same(b.contiguous(), a.to(x.dtype), f"{name} donate={donate} step {t} update {i}")
      _assert_states_equal(pa, s_ref, s, f"{name} donate={donate}")
