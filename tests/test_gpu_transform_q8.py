"""ps_transform_grads_q8: the every-step transform on int8 momentum, read and written where it lies.

The yardstick is the composition the functional path ran before the entry existed, on the same
inputs and through the project's golden-pinned entries: ps_dequantize_f32 ->
ps_transform_grads_typed -> ps_quantize_f32.  Every comparison is on bit patterns (int8 codes,
float32 bucket sizes, update, diagonal statistics); no tolerance appears in this file.  Outputs
sit inside sentinel frames, the workspace is filled with garbage before every call, and the
in-place form (codes, bucket sizes and diagonal statistics aliased) runs twice in a row.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_every_step_references import VARIANTS, variant_cfg

pytestmark = pytest.mark.gpu

PS_EINVAL = -1
F32, BF16 = 0, 1
PAD = 64                      # sentinel elements on either side of an output
SENT_F = -777.25
SENT_B = -128                 # a code is never -128
_DIAG_GRAFTS = (2, 3, 4, 6)   # Adagrad, RMSProp, RMSProp normalised, Adagrad normalised

# (shape, int8 momenta?, preconditioned gradient?)
TREE = [
    ((3, 5), True, True),          # cols no multiple of 4
    ((130, 257), True, True),      # 9 chunks, rows straddle chunk borders, odd cols
    ((2, 5000), True, True),       # cols > 4096: a chunk lies inside one row
    ((3, 7, 33), True, True),      # rank 3, cols = 231
    ((64, 64), True, True),        # column ZCOL is zero everywhere: bucket 0, codes 0
    ((300,), False, True),         # float32 momenta (cols = 0)
    ((40, 6), True, False),        # skipped parameter: no preconditioned gradient
    ((0, 4), True, True),          # no elements: null pointers, no work
]
ZSHAPE, ZCOL = (64, 64), 5


def _K():
  from precondition_amd import kernels
  return kernels


def _lib():
  from precondition_amd import _lib as L
  return L.lib()


def _stream():
  return torch.cuda.current_stream().cuda_stream


def _cols(shape):
  return int(np.prod(shape[1:], dtype=np.int64))


def _bits(t):
  """Bit patterns of a tensor, on the host."""
  t = t.detach().contiguous().cpu()
  if t.dtype == torch.float32:
    return t.numpy().view(np.uint32)
  if t.dtype == torch.bfloat16:
    return t.view(torch.int16).numpy()
  return t.numpy()


def _same(a, b, what):
  assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (what, a.dtype, b.dtype, a.shape, b.shape)
  x, y = _bits(a), _bits(b)
  if not np.array_equal(x, y):
    bad = np.argwhere(x != y)
    raise AssertionError(f"{what}: {len(bad)} of {x.size} elements differ; first at {bad[0].tolist()}: "
                         f"{a.cpu()[tuple(bad[0])].item()!r} vs {b.cpu()[tuple(bad[0])].item()!r}")


class Framed:
  """A contiguous tensor of `shape` with sentinel elements on either side (an odd number of them in
  front of int8 codes: codes carry no alignment)."""

  def __init__(self, shape, dtype, dev, fill=None):
    n = int(np.prod(shape, dtype=np.int64))
    pad = PAD - 1 if dtype == torch.int8 else PAD
    self.sent = torch.full((), SENT_B if dtype == torch.int8 else SENT_F, dtype=dtype, device=dev)
    self.holder = self.sent.repeat(n + 2 * pad)
    self.view = self.holder[pad:pad + n].view(shape)
    self.pad = pad
    if fill is not None:
      self.view.copy_(fill)

  def intact(self):
    edge = torch.cat([self.holder[:self.pad], self.holder[self.holder.numel() - self.pad:]])
    return bool((edge == self.sent).all())

  def untouched(self):
    return bool((self.holder == self.sent).all())


def make_tree(seed, gdtype, dev):
  """Inputs of one call: finite, momenta random over the whole code range with random positive
  bucket sizes.  Gradients are exact in bfloat16 when gdtype is, so both runs read the same values."""
  rng = np.random.default_rng(seed)
  tree = []
  for shape, q8, has_pg in TREE:
    f = lambda scale=1.0: (rng.standard_normal(shape) * scale).astype(np.float32)
    grad, pgrad, param = f(0.1), f(0.3), f(0.5)
    diag = np.abs(f(0.05)) + np.float32(1e-4)
    codes = [rng.integers(-127, 128, size=shape).astype(np.int8) for _ in range(2)]
    buckets = [rng.uniform(1e-4, 2e-2, size=shape[1:]).astype(np.float32) for _ in range(2)]
    moms = [f(0.2), f(0.2)]
    if shape == ZSHAPE:
      for a in (grad, pgrad, param, codes[0], codes[1]):
        a[:, ZCOL] = 0
    t = lambda a: torch.from_numpy(a).to(dev)
    it = dict(shape=shape, q8=q8, grad=t(grad).to(gdtype), pgrad=t(pgrad) if has_pg else None,
              param=t(param), diag=t(diag))
    if q8:
      it.update(mom=(t(codes[0]), t(buckets[0])), dmom=(t(codes[1]), t(buckets[1])))
    else:
      it.update(mom=t(moms[0]), dmom=t(moms[1]))
    tree.append(it)
  return tree


def yardstick_step(tree, cfg):
  """One step of dequantize -> float32 transform -> quantize; returns the tree of the next step and
  the updates."""
  K = _K()
  diag = cfg["graft_type"] in _DIAG_GRAFTS
  qi = [i for i, it in enumerate(tree) if it["q8"] and it["grad"].numel()]
  fl = K.dequantize_grouped([(tree[i]["mom"][0], [], tree[i]["mom"][1]) for i in qi] +
                            [(tree[i]["dmom"][0], [], tree[i]["dmom"][1]) for i in qi])
  mom = {i: f for i, f in zip(qi, fl[:len(qi)])}
  dmom = {i: f for i, f in zip(qi, fl[len(qi):])}
  items = []
  for i, it in enumerate(tree):
    empty = torch.empty(it["shape"], dtype=torch.float32, device=it["grad"].device)
    items.append(dict(
        grad=it["grad"], pgrad=it["pgrad"], param=it["param"] if cfg["weight_decay"] != 0 else None,
        diag_in=it["diag"] if diag else None,
        mom_in=mom.get(i, empty) if it["q8"] else it["mom"],
        dmom_in=dmom.get(i, empty) if it["q8"] else it["dmom"]))
  res = K.transform_grads_fused(items, cfg)
  qm = K.quantize_grouped([res[i][2] for i in qi] + [res[i][3] for i in qi], torch.int8)
  nxt, upds = [], []
  for i, (it, (upd, nd, m, d)) in enumerate(zip(tree, res)):
    new = dict(it, diag=nd if diag else it["diag"])
    if i in qi:
      k = qi.index(i)
      new.update(mom=(qm[k][0], qm[k][2]), dmom=(qm[len(qi) + k][0], qm[len(qi) + k][2]))
    elif not it["q8"]:
      new.update(mom=m, dmom=d)
    nxt.append(new)
    upds.append(upd)
  return nxt, upds


def _table(n):
  K = _K()
  from precondition_amd._lib import TransformQ8Desc
  assert K._TQDESC_DT.itemsize == C.sizeof(TransformQ8Desc)
  tbl = np.zeros(n, K._TQDESC_DT)
  return tbl, C.cast(tbl.ctypes.data, C.POINTER(TransformQ8Desc))


def _ptr(t):
  return 0 if t is None or t.numel() == 0 else t.data_ptr()


class Q8Call:
  """Buffers and descriptor table of one ps_transform_grads_q8 call on `tree`.  inplace: the state
  (codes, bucket sizes, diagonal statistics, float32 momenta) lives in the framed buffers and every
  x_out is x_in; otherwise the inputs are the tree's own tensors and only the outputs are framed."""

  def __init__(self, tree, cfg, gdtype, inplace, dev):
    self.tree, self.cfg, self.inplace, self.dev = tree, cfg, inplace, dev
    self.diag = cfg["graft_type"] in _DIAG_GRAFTS
    self.gcode = BF16 if gdtype == torch.bfloat16 else F32
    n = len(tree)
    self.tbl, self.descs = _table(n)
    self.out = []
    t = self.tbl
    for i, it in enumerate(tree):
      sh = it["shape"]
      fill = (lambda x: x) if inplace else (lambda x: None)
      o = dict(upd=Framed(sh, gdtype, dev))
      if self.diag:
        o["diag"] = Framed(sh, torch.float32, dev, fill(it["diag"]))
      if it["q8"]:
        for name in ("mom", "dmom"):
          o[name + "_codes"] = Framed(sh, torch.int8, dev, fill(it[name][0]))
          o[name + "_bucket"] = Framed(sh[1:], torch.float32, dev, fill(it[name][1]))
      else:
        for name in ("mom", "dmom"):
          o[name] = Framed(sh, torch.float32, dev, fill(it[name]))
      self.out.append(o)
      t["numel"][i] = it["grad"].numel()
      if it["grad"].numel() == 0:   # every pointer stays null
        t["cols"][i] = _cols(sh)
        continue
      t["grad"][i], t["pgrad"][i] = _ptr(it["grad"]), _ptr(it["pgrad"])
      t["param"][i] = _ptr(it["param"]) if cfg["weight_decay"] != 0 else 0
      t["upd_out"][i] = _ptr(o["upd"].view)
      if self.diag:
        t["diag_out"][i] = _ptr(o["diag"].view)
        t["diag_in"][i] = t["diag_out"][i] if inplace else _ptr(it["diag"])
      if it["q8"]:
        t["cols"][i] = _cols(sh)
        for name in ("mom", "dmom"):
          t[name + "_codes_out"][i] = _ptr(o[name + "_codes"].view)
          t[name + "_bucket_out"][i] = _ptr(o[name + "_bucket"].view)
          t[name + "_codes_in"][i] = t[name + "_codes_out"][i] if inplace else _ptr(it[name][0])
          t[name + "_bucket_in"][i] = t[name + "_bucket_out"][i] if inplace else _ptr(it[name][1])
      else:
        for name in ("mom", "dmom"):
          t[name + "_out"][i] = _ptr(o[name].view)
          t[name + "_in"][i] = t[name + "_out"][i] if inplace else _ptr(it[name])
    L = _lib()
    self.ws = torch.empty(max(int(L.ps_transform_grads_q8_workspace_bytes(self.descs, n)), 256),
                          dtype=torch.uint8, device=dev)

  def run(self):
    from precondition_amd._lib import TransformConfig
    c = TransformConfig()
    for k, v in self.cfg.items():
      setattr(c, k, v)
    self.ws.fill_(0xFF)   # nothing may be assumed about the workspace
    rc = _lib().ps_transform_grads_q8(_stream(), self.descs, len(self.tree), C.byref(c), self.gcode, F32,
                                      self.ws.data_ptr(), self.ws.numel())
    torch.cuda.synchronize()
    return rc

  def check(self, want_tree, want_upd, what):
    for i, (o, w, u) in enumerate(zip(self.out, want_tree, want_upd)):
      tag = f"{what}, parameter {i} {w['shape']}"
      for name, f in o.items():
        assert f.intact(), f"{tag}: the frame of {name} was written"
      _same(o["upd"].view, u, tag + " update")
      if self.diag:
        _same(o["diag"].view, w["diag"], tag + " diagonal statistics")
      if w["q8"]:
        if w["grad"].numel() == 0:
          continue
        for name in ("mom", "dmom"):
          _same(o[name + "_bucket"].view, w[name][1], f"{tag} {name} bucket sizes")
          _same(o[name + "_codes"].view, w[name][0], f"{tag} {name} codes")
      else:
        for name in ("mom", "dmom"):
          _same(o[name].view, w[name], f"{tag} {name}")


_REF = {}


def _reference(graft, variant, run_shampoo, gdtype, dev):
  """The yardstick's two steps for one configuration, computed once and left unchanged."""
  key = (graft, variant, run_shampoo, gdtype)
  if key not in _REF:
    cfg = variant_cfg(graft, variant, run_shampoo)
    tree = make_tree(1000 * graft + 10 * variant + run_shampoo, gdtype, dev)
    s1, u1 = yardstick_step(tree, cfg)
    s2, u2 = yardstick_step(s1, cfg)
    torch.cuda.synchronize()
    _REF[key] = (cfg, tree, (s1, u1), (s2, u2))
  return _REF[key]


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("run_shampoo", [0, 1])
@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("graft", range(7))
def test_q8_entry_is_the_three_call_composition_bit_for_bit(graft, variant, run_shampoo, gdtype, inplace,
                                                            device):
  cfg, tree, (s1, u1), (s2, u2) = _reference(graft, variant, run_shampoo, gdtype, device)
  # the zero column of the yardstick: bucket size 0 and codes 0 (QU:89-90)
  zi = [it["shape"] for it in tree].index(ZSHAPE)
  for name in ("mom", "dmom"):
    assert float(s1[zi][name][1][ZCOL]) == 0.0 and not bool(s1[zi][name][0][:, ZCOL].any())
  call = Q8Call(tree, cfg, gdtype, inplace, device)
  assert call.run() == 0
  call.check(s1, u1, "step 1")
  if inplace:
    # again from where the first call left the state: a bucket size or a diagonal statistic written
    # before its last read, or maxima left over in the workspace, show here
    assert call.run() == 0
    call.check(s2, u2, "step 2")


def _invalid_cases():
  def null(field):
    def f(tbl, i):
      tbl[field][i] = 0
    return f

  def ragged(tbl, i):
    tbl["cols"][i] = 7        # 130 * 257 is no multiple of 7
  def negative(tbl, i):
    tbl["cols"][i] = -1
  def odd_grad(tbl, i):
    tbl["grad"][i] += 1
  def odd_upd(tbl, i):
    tbl["upd_out"][i] += 1
  cases = [(n, null(n), F32) for n in ("mom_codes_in", "mom_codes_out", "mom_bucket_in", "mom_bucket_out",
                                       "dmom_codes_in", "dmom_codes_out", "dmom_bucket_in",
                                       "dmom_bucket_out")]
  cases += [("numel_not_a_multiple_of_cols", ragged, F32), ("negative_cols", negative, F32),
            ("odd_bf16_grad", odd_grad, BF16), ("odd_bf16_upd", odd_upd, BF16)]
  return cases


@pytest.mark.parametrize("name,spoil,gcode", _invalid_cases(), ids=[c[0] for c in _invalid_cases()])
def test_q8_invalid_descriptor_is_refused_and_writes_nothing(name, spoil, gcode, device):
  gdtype = torch.bfloat16 if gcode == BF16 else torch.float32
  cfg = variant_cfg(3, 1, 1)
  tree = make_tree(7, gdtype, device)
  call = Q8Call(tree, cfg, gdtype, False, device)
  spoil(call.tbl, 1)          # the [130, 257] parameter, behind a valid one
  assert call.run() == PS_EINVAL
  for i, o in enumerate(call.out):
    for what, f in o.items():
      assert f.untouched(), f"{name}: {what} of parameter {i} was written"


def test_q8_float32_momentum_needs_its_pointers(device):
  """cols == 0 keeps the float32 entry's rule: a null momentum pointer is PS_EINVAL."""
  cfg = variant_cfg(1, 0, 1)
  tree = make_tree(8, torch.float32, device)
  call = Q8Call(tree, cfg, torch.float32, False, device)
  call.tbl["dmom_in"][5] = 0
  assert call.run() == PS_EINVAL
  assert all(f.untouched() for o in call.out for f in o.values())
