"""Round 6 (GPU): parity against the reference's TRUE arithmetic (float32 LAPACK), stream groups of the
staged Newton execution, the per-step qualification of the donated path.

* eigh roots: the default solver's error metric (DS:1017-1021) next to a true ssyevd's at 1024 / 2048 rows;
* ps_newton_root_batched_opt_f32: the stream groups (newton_driver) do not change a bit;
* distributed_shampoo(donate_state=True): a gradient that is a strided VIEW with the bound data_ptr and shape
  takes the functional path instead of being read as contiguous.
All through the C-ABI (ctypes), against oracle/ (test infrastructure).
"""
import os

import numpy as np
import pytest
import torch

from oracle import shampoo_oracle as orc

pytestmark = pytest.mark.gpu


def K():
  from precondition_amd import kernels
  return kernels


def wishart(n, k, seed):
  g = np.random.default_rng(seed).standard_normal((n, k)).astype(np.float32)
  return (g @ g.T).astype(np.float32)


@pytest.mark.parametrize("n", [1024, 2048])
def test_eigh_error_metric_within_1p5x_of_true_float32_lapack(n, device):
  """inverse_pth_root_errors of an eigh root (DS:1017-1021: max|u^T D u - diag(e)|) on a BASELINE-configs[2]
  style block (Wishart, lambda_max ~ 1.2e4 at 2048 rows): the build's value is at most 1.5 x what the
  reference's own arithmetic (float32 ssyevd + sgemm, oracle lapack="f32") reports -- the select at
  DS:2936-2950 is an ABSOLUTE err >= 0.1, so a metric inflated by the build's own rounding would discard
  preconditioners the reference keeps (2.7 x until round 6: one float32 chain over k for the diagonal of
  u^T (D u)).  The root itself within 2e-5 of the oracle's and at ssyevd's distance from float64."""
  a = wishart(n, 2 * n, 2048 + n)
  h_ref, m_ref = orc.matrix_inverse_pth_root_eigh(a, 2)
  roots, met = K().matrix_inverse_pth_root_batched([torch.tensor(a, device=device)], [2], eigh=True)
  met = met.cpu().numpy()
  assert met[0, 5] == 0                                             # stayed on the tridiagonalisation path
  assert met[0, 0] <= 1.5 * m_ref["inverse_pth_root_errors"], (met[0, 0], m_ref["inverse_pth_root_errors"])
  assert met[0, 0] < 0.1
  h = roots[0].cpu().numpy()
  assert np.linalg.norm(h - h_ref) / np.linalg.norm(h_ref) < 2e-5
  truth = orc.eigh_root_float64(a, 2)
  tn = np.linalg.norm(truth)
  assert np.linalg.norm(h - truth) / tn <= 1.25 * np.linalg.norm(h_ref - truth) / tn + 2e-6


def test_newton_stream_groups_do_not_change_a_bit(device, monkeypatch):
  """The staged execution deals the blocks of a call to stream groups (2 by default when sizes / exponents
  are mixed): every group runs the same launches for its blocks on a stream of its own.  Roots, iteration
  counts and every metrics column are bit-identical for 1, 2, 3 and 4 groups, with blocks that converge
  at different steps, a retried block, an all-padding block and a hint."""
  rng = np.random.default_rng(3)
  q, _ = np.linalg.qr(rng.standard_normal((256, 256)))
  graded = ((q * 1e5 ** (-np.arange(256) / 255.0)) @ q.T)
  graded = ((graded + graded.T) / 2).astype(np.float32)
  # an indefinite block: the first tries diverge whatever the rounding (3 tries, tests/test_gpu_parity.py)
  q24, _ = np.linalg.qr(np.random.default_rng(7).standard_normal((24, 24)))
  e24 = np.linspace(1, 0.1, 24); e24[-1] = -3e-5
  rank1 = (q24 * e24) @ q24.T
  rank1 = ((rank1 + rank1.T) / 2).astype(np.float32)
  mats = [wishart(512, 2048, 1), wishart(384, 1536, 2), graded, wishart(200, 800, 4), rank1,
          wishart(640, 700, 5), np.eye(10, dtype=np.float32), wishart(130, 520, 6)]
  ps = [4, 2, 4, 2, 4, 4, 4, 8]
  pads = [512, 384, 256, 200, 24, 640, 0, 130]
  ts = [torch.tensor(m, device=device) for m in mats]
  outs = {}
  for groups in ("1", "2", "3", "4"):
    monkeypatch.setenv("PS_NEWTON_GROUPS", groups)
    for hint in (None, [8.0, 7.0, 30.0, 7.0, 1.0, 12.0, 0.0, 9.0]):
      r, m = K().matrix_inverse_pth_root_batched(ts, ps, pads, options=None if hint is None else {"iters_hint": hint})
      outs[(groups, hint is None)] = ([x.clone() for x in r], m.clone())
  for nohint in (True, False):
    r1, m1 = outs[("1", nohint)]
    assert m1.cpu().numpy()[4, 4] == 3 and m1.cpu().numpy()[2, 1] > m1.cpu().numpy()[0, 1]   # retries; different step counts
    for groups in ("2", "3", "4"):
      r, m = outs[(groups, nohint)]
      # (the all-padding block's lambda_max is 0 / 0 = NaN, as in the reference: compare NaNs as equal)
      assert np.array_equal(m.cpu().numpy(), m1.cpu().numpy(), equal_nan=True), groups
      for x, y in zip(r, r1):
        assert torch.equal(x, y), groups
  monkeypatch.delenv("PS_NEWTON_GROUPS")
  r, m = K().matrix_inverse_pth_root_batched(ts, ps, pads)       # the default (mixed call: 2 groups)
  assert np.array_equal(m.cpu().numpy(), outs[("1", True)][1].cpu().numpy(), equal_nan=True)
  for i, (a, p, pad) in enumerate(zip(mats, ps, pads)):             # and the oracle, as ever
    h_ref, m_ref = orc.matrix_inverse_pth_root(a, p, padding_start=pad)
    if np.linalg.norm(h_ref) > 0:
      # (blocks 2 and 5 -- cond 1e5, a nearly square Wishart -- stop within rounding of the 1e-6 threshold: +-1 step)
      assert abs(m.cpu().numpy()[i, 1] - m_ref["inverse_pth_root_iters"]) <= (1 if i in (2, 5) else 0), i
      assert m.cpu().numpy()[i, 4] == m_ref["total_retries"], i


def test_donated_step_strided_gradient_view_takes_the_functional_path(device):
  """plan.DonatedStep binds raw pointers.  A gradient that arrives as a `.t()` view of a square buffer has the
  data_ptr and shape of the bound one but other strides: it must not be read as contiguous.  The step
  (qualifies(): checked every step, before the pointer comparison) takes the functional path, which copies
  the view; updates equal a functional optimizer's bit for bit before, at and after that step."""
  import precondition_amd as pa
  rng = np.random.default_rng(1)
  shapes = [(256, 256), (256,), (128, 384)]
  params = [torch.from_numpy(np.asarray(rng.standard_normal(s) * 0.05, np.float32)).to(device) for s in shapes]
  bufs = [torch.empty(s, dtype=torch.float32, device=device) for s in shapes]   # gradients live in fixed buffers

  def grads_at(t, view):
    r = np.random.default_rng(50 + t)
    for b, s in zip(bufs, shapes):
      b.copy_(torch.from_numpy(np.asarray(r.standard_normal(s) * 0.05, np.float32)))
    return [bufs[0].t() if view else bufs[0], bufs[1], bufs[2]]

  outs = {}
  for donate in (False, True):
    opt = pa.distributed_shampoo(0.1, 512, preconditioning_compute_steps=4, start_preconditioning_step=1,
                                 graft_type=pa.GraftingType.RMSPROP_NORMALIZED, donate_state=donate)
    st = opt.init(params)
    ups = []
    for t in range(6):
      upd, st = opt.update(grads_at(t, view=(t == 3)), st, params)   # step 3: same data_ptr, transposed strides
      ups.append([u.clone() for u in upd])
    outs[donate] = ups
  for t, (a, b) in enumerate(zip(outs[False], outs[True])):
    for x, y in zip(a, b):
      assert torch.equal(x, y), t
  # the view really differs from reading the buffer as contiguous
  assert not torch.equal(bufs[0].t().contiguous(), bufs[0])


def test_expired_power_iteration_restart_with_stream_groups(device, monkeypatch):
  """The recovery path of an expired resident power iteration (tests/test_gpu_round3.py) in a call that runs
  TWO stream groups (mixed sizes): the driver notices the expiry at its first host wait, joins the side
  stream, queues the whole front again on the caller's stream, forks again and starts every group over.
  Same bits as an undisturbed call (the streaming power iteration is bit-identical to the resident one)."""
  import ctypes as C
  from precondition_amd import _lib
  L = _lib.lib()

  def health():
    e, c, r = C.c_uint(), C.c_int(), C.c_int()
    assert L.ps_power_iteration_health(C.addressof(e), C.addressof(c), C.addressof(r)) == 0
    return e.value, c.value, r.value

  L.ps_power_iteration_reset_health()
  arrs = [wishart(512, 2048, 400 + i) for i in range(6)] + [wishart(384, 1536, 410 + i) for i in range(6)]
  ps = [4] * 6 + [2] * 6
  ts = [torch.tensor(a, device=device) for a in arrs]
  r0, m0 = K().matrix_inverse_pth_root_batched(ts, ps)
  r0 = [x.clone() for x in r0]
  m0 = m0.clone()
  assert health()[0] == 0
  monkeypatch.setenv("PS_PI_TIMEOUT_MS", "0")
  try:
    r1, m1 = K().matrix_inverse_pth_root_batched(ts, ps)
    torch.cuda.synchronize()
    expired, _, resident = health()
    assert expired > 0 and resident == 0, (expired, resident)
    assert np.isfinite(m1.cpu().numpy()[:, :5]).all()
    # column 6 (power-iteration steps) and everything else: the same
    assert np.array_equal(m1.cpu().numpy(), m0.cpu().numpy())
    for x, y in zip(r1, r0):
      assert torch.equal(x, y)
  finally:
    monkeypatch.delenv("PS_PI_TIMEOUT_MS")
    L.ps_power_iteration_reset_health()
  assert health() == (0, 0, 1)


@pytest.mark.parametrize("d,rank,bsz,factor", [(1024, 8, 3, False), (2048, 64, 2, False), (1024, 20, 2, True)])
def test_fd_update_one_library_call_equals_the_step_by_step_path(d, rank, bsz, factor, device):
  """ps_fd_update_batched_f32 (SURVEY 8(b)'s ps_fd_update_batched; DS:1123-1290 for a group of factors in ONE
  call: preparation, every outer round of the subspace iteration, deflation / masks / packing) against the
  step-by-step Python-driven path (one_call=False: the same library calls issued one by one + torch
  elementwise ops): two chained updates, the packed sketches agree to float32 rounding (the eigenpairs come from
  the same calls on the same start block; only the column norms of the finish are summed in another order), and
  both match the oracle's SVD-based update (float32 sgesdd) through what the optimizer uses."""
  from precondition_amd import low_rank
  from tests.test_optimizer_host_logic import packed_matches
  rng = np.random.default_rng(d + rank)
  outs = {}
  grads = []
  for t in range(2):
    gs = []
    for j in range(bsz):
      g = rng.standard_normal((d, 2 * d)).astype(np.float32) * np.float32(1.0 + 0.3 * t)
      g[:rank + 2] *= np.linspace(6.0, 2.0, rank + 2)[:, None].astype(np.float32)   # a separated leading subspace
      gs.append(g)
    grads.append(gs)
  for one_call in ("1", "0"):
    prevs = [torch.zeros((d, rank + 2), dtype=torch.float32, device=device) for _ in range(bsz)]
    chain = []
    for t in range(2):
      calls = []
      for j in range(bsz):
        g = torch.tensor(grads[t][j], device=device)
        gram = K().matmul(g, g, transb=True)
        if factor:   # a factor R with R R^T = Gram (what the reference keeps in its statistics slot)
          e, v = torch.linalg.eigh(gram.double().cpu())
          new_grad = (v * e.clamp_min(0).sqrt()).float().to(device).contiguous()
        else:
          new_grad = gram
        calls.append(dict(new_grad=new_grad, p=4, rank=rank, ridge_epsilon=1e-6, decay=0.999, padding_start=d,
                          prev=prevs[j], new_grad_is_gram=not factor))
      res = low_rank._fd_update_root_batched(calls, one_call=one_call == "1")
      prevs = [r[0] for r in res]
      chain.append([p_.cpu().numpy() for p_ in prevs])
    outs[one_call] = chain
  for t in range(2):
    for a, b in zip(outs["1"][t], outs["0"][t]):
      assert a.shape == b.shape == (d, rank + 2)
      if t == 0:
        assert np.allclose(a[:, -2:], b[:, -2:], rtol=5e-6, atol=0), np.abs(a[:, -2:] - b[:, -2:]).max()
        assert np.abs(a[:, :rank] - b[:, :rank]).max() <= 1e-5                # unit vectors, same signs
      else:
        # the second update starts from sketches that differ in the last bits of their normalisation: the small
        # eigensolver may then return an eigenvector with the other sign -- compare what the optimizer uses
        assert np.allclose(a[:, -2:], b[:, -2:], rtol=5e-5, atol=0), np.abs(a[:, -2:] - b[:, -2:]).max()
        assert packed_matches(a, b, rank, tol=1e-3)
      assert a[-1, -2] == b[-1, -2]
  # and the oracle (float32 LAPACK) on the first factor of the first update
  g0 = grads[0][0]
  gram0 = (g0.astype(np.float64) @ g0.astype(np.float64).T)
  w, v = np.linalg.eigh(gram0)
  fac = (v * np.sqrt(np.maximum(w, 0))).astype(np.float32)
  ref = orc.fd_update_root(fac, 4, rank, ridge_epsilon=1e-6, error_tolerance=1e-6, relative_matrix_epsilon=True,
                           decay=0.999, padding_start=d, prev=np.zeros((d, rank + 2), np.float32))
  assert packed_matches(outs["1"][0][0], ref, rank, tol=2e-3)


_TQ6 = {8: torch.int8, 16: torch.int16}


@pytest.mark.parametrize("shape,bits,extract", [
    ((1024, 1024), 16, True), ((768, 768), 8, True), ((512, 320), 16, False), ((100, 132), 16, False),
    ((1000, 260), 8, False), ((96, 96), 16, True), ((64, 4), 8, False), ((1024, 8192), 16, False),
    ((2048, 2048), 16, True), ((3072, 768), 8, False), ((1500, 260), 16, False), ((4096, 64), 8, False),
    ((4100, 64), 16, False), ((1, 151296), 8, False), ((3, 20000), 16, False), ((40, 5004), 8, False)])
def test_quantize_register_strips_on_rounding_boundaries_and_extreme_scales(shape, bits, extract, device):
  """quant_strip_kernel (matrices of 64 ... 1024 rows, one read): its division is the IEEE sequence with the
  column-only part hoisted, its rounding a magic-constant add.  Inputs aimed at exactly those steps: elements AT
  and one ulp either side of (k + 1/2) * bucket (round half to even decides), columns scaled by 2^-80 ... 2^80
  (outside [2^-60, 2^60] a wavefront takes the plain division), denormals, exact zeros, zero columns, row counts
  that are not multiples of 32 and column counts that are not multiples of 64; tall matrices (1025 ... 4096 rows:
  parts of 1024 rows on different workgroups that merge their column maxima; 4100 rows: the two-pass kernels);
  wide and short ones ([1, 197, 768] embeddings: ranges of columns, one workgroup each).  Codes, diagonal and bucket sizes
  bit-identical to the oracle's (numpy float32 division is correctly rounded; np.round is half-even)."""
  from oracle import quantization_oracle as qorc
  from tests.quant_inputs import rounding_boundary_input
  x = rounding_boundary_input(shape, bits, extract)
  npdt = np.int8 if bits == 8 else np.int16
  oq, od, ob = qorc.quantize(x, npdt, extract)
  q, d, b = K().quantize_grouped([torch.tensor(x, device=device)], _TQ6[bits], extract)[0]
  assert np.array_equal(b.cpu().numpy().view(np.uint32), np.asarray(ob, np.float32).view(np.uint32))
  bad = np.argwhere(q.cpu().numpy() != oq)
  assert bad.size == 0, (len(bad), bad[:4], [(x[i, j], ob[j]) for i, j in bad[:4]])
  if extract:
    assert np.array_equal(d.cpu().numpy().view(np.uint32), od.view(np.uint32))


def test_quantize_strip_queue_mixed_tensors_bit_exact(device):
  """One call with more strips than workgroups (the persistent kernel takes the rest from its queue and loads the
  NEXT strip while it encodes the current one): tensors of different heights, widths and code widths in one
  descriptor list, every code / bucket size / diagonal entry against the oracle."""
  from oracle import quantization_oracle as qorc
  rng = np.random.default_rng(66)
  shapes = [(1024, 1024), (768, 768), (64, 4096), (100, 132), (3072, 768), (512, 320), (1000, 260), (96, 96),
            (256, 2048), (2048, 2048), (1500, 128)] * 4
  xs = []
  for i, (r, c) in enumerate(shapes):
    x = (rng.standard_normal((r, c)) * np.exp(rng.uniform(-6, 6, size=c))).astype(np.float32)
    if r == c:
      x = (x + x.T).astype(np.float32)
    x[rng.uniform(size=x.shape) < 0.03] = 0.0
    xs.append(np.ascontiguousarray(x))
  assert sum((c + 63) // 64 for _, c in shapes) > 2 * 256
  for bits, extract_square in ((16, True), (8, False)):
    npdt = np.int8 if bits == 8 else np.int16
    group = [x for x in xs if (x.shape[0] == x.shape[1]) == extract_square] if extract_square else xs
    out = K().quantize_grouped([torch.tensor(x, device=device) for x in group], _TQ6[bits], extract_square)
    for x, (q, d, b) in zip(group, out):
      oq, od, ob = qorc.quantize(x, npdt, extract_square)
      assert np.array_equal(q.cpu().numpy(), oq), x.shape
      assert np.array_equal(b.cpu().numpy().view(np.uint32), np.asarray(ob, np.float32).view(np.uint32)), x.shape
      if extract_square:
        assert np.array_equal(d.cpu().numpy().view(np.uint32), od.view(np.uint32)), x.shape


def test_quantize_tall_strips_next_to_a_busy_stream(device):
  """Parts of a tall strip wait for each other on the device (quant_strip_kernel's team step).  With another stream
  keeping most of the chip busy the parts of a team become resident at different times: the wait must neither hang
  nor expire (an expired wait publishes NaN bucket sizes), and the codes stay the oracle's."""
  from oracle import quantization_oracle as qorc
  rng = np.random.default_rng(67)
  xs = [np.ascontiguousarray((rng.standard_normal((3072, 768)) * np.exp(rng.uniform(-3, 3, size=768))).astype(np.float32))
        for _ in range(6)]
  ts = [torch.tensor(x, device=device) for x in xs]
  a = torch.randn((6144, 6144), device=device)
  side = torch.cuda.Stream(device=device)
  torch.cuda.synchronize()
  with torch.cuda.stream(side):
    for _ in range(40):
      a = torch.nn.functional.normalize(a @ a, dim=0)      # ~3 ms each: the chip stays busy for the whole test
  outs = []
  for _ in range(20):
    outs.append(K().quantize_grouped(ts, torch.int8, False))
  torch.cuda.synchronize()
  ref = [qorc.quantize(x, np.int8, False) for x in xs]
  for out in (outs[0], outs[-1]):
    for (q, d, b), (oq, od, ob) in zip(out, ref):
      assert torch.isfinite(b).all()
      assert np.array_equal(b.cpu().numpy().view(np.uint32), np.asarray(ob, np.float32).view(np.uint32))
      assert np.array_equal(q.cpu().numpy(), oq)


def test_fd_update_two_interleaved_groups_do_not_change_a_bit(device, monkeypatch):
  """ps_fd_update_batched_f32 runs a call as resumable per-group runs (begin / step / finish); with the developer
  switch PS_FD_GROUPS=2 a call of >= 4 factors becomes two groups on two streams whose rounds interleave.  Factors
  are independent: the packed sketches and convergence flags are bit-identical to the one-group run, on two chained
  updates of five factors (groups of 3 + 2)."""
  d, rank, bsz = 1024, 24, 5
  rng = np.random.default_rng(77)
  grams = []
  for t in range(2):
    gs = []
    for j in range(bsz):
      g = rng.standard_normal((d, 2 * d)).astype(np.float32)
      g[:rank + 2] *= np.linspace(6.0, 2.0, rank + 2)[:, None].astype(np.float32)
      gt = torch.tensor(g, device=device)
      gs.append(K().matmul(gt, gt, transb=True))
    grams.append(gs)
  b = int(K().lib().ps_fd_block_columns(rank, d))
  x0 = torch.randn((bsz, d, b), generator=torch.Generator(device="cpu").manual_seed(1729)).to(device)
  outs = {}
  for groups in ("1", "2"):
    monkeypatch.setenv("PS_FD_GROUPS", groups)
    prev = torch.zeros((bsz, d, rank + 2), dtype=torch.float32, device=device)
    chain = []
    for t in range(2):
      res = K().fd_update_batched(grams[t], prev, 4, rank, 0.999, 1e-6, 1e-6, True, x0)
      assert res is not None
      out, conv, info = res
      chain.append((out.cpu().numpy().copy(), conv.cpu().numpy().copy()))
      prev = out.clone()
    outs[groups] = chain
  monkeypatch.delenv("PS_FD_GROUPS")
  for (o1, c1), (o2, c2) in zip(outs["1"], outs["2"]):
    assert np.array_equal(c1, c2)
    assert np.array_equal(o1.view(np.uint32), o2.view(np.uint32))


def test_quantize_tall_strips_repeated_calls_never_read_a_stale_maximum(device):
  """The parts of a tall strip merge their column maxima with atomics and then count themselves in; a part that
  counted itself in before its merges were PERFORMED let a team mate read a stale maximum (wrong codes in ~1 % of
  the calls until the merges became returning atomics whose results are awaited).  600 grouped calls of tall
  matrices, every one against the oracle's codes and bucket sizes."""
  from oracle import quantization_oracle as qorc
  rng = np.random.default_rng(68)
  shapes = [(2048, 2048), (2500, 1000), (3072, 768), (1025, 128)]
  xs = [np.ascontiguousarray((rng.standard_normal(s) * np.exp(rng.uniform(-4, 4, size=s[1]))).astype(np.float32))
        for s in shapes]
  ts = [torch.tensor(x, device=device) for x in xs]
  ref = [qorc.quantize(x, np.int16, False) for x in xs]
  refq = [torch.tensor(r[0], device=device) for r in ref]
  refb = [torch.tensor(np.asarray(r[2], np.float32), device=device) for r in ref]
  bad = 0
  for _ in range(600):
    for i, (q, d, b) in enumerate(K().quantize_grouped(ts, torch.int16, False)):
      bad += int(not (torch.equal(q, refq[i]) and torch.equal(b.view(torch.int32), refb[i].view(torch.int32))))
  assert bad == 0, bad
