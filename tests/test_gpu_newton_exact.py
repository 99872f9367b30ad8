"""Per-element tests of the coupled-Newton inverse p-th root (csrc/newton.hip: newton_stage_kernel
and newton_persistent_kernel over gemm_core.hip.h) and integer exactness of ps_mat_power_f32.

The end-to-end Newton tests compare relative Frobenius norms of a self-correcting iteration: a
tile that is slightly wrong in one step is pulled back by the next ones, and a handful of wrong
elements vanish in a norm over n^2.  Here the expected output is known per element
(tests/_newton_exact.py, pinned to the oracle on the CPU by test_newton_exact_references.py):

Family 1, diagonal blocks, BIT FOR BIT.  Preconditions: relative_matrix_epsilon = False (ridge =
ridge_epsilon = 2^-4), d_i in {1, 2, 3, 4} times one power of two, so that sum (d_i + ridge)^2 is
exact in any order (asserted per case by _newton_exact.exact_sumsq); z is then reproducible and
h0 = powf(z, 1/p) is one of three candidates (the host's value and its two float32 neighbours;
p = 1: h0 = z only) -- ONE candidate must reproduce EVERY diagonal element of the block.  Also
asserted: exact zeros off the diagonal and from padding_start on, an untouched sentinel frame
around the output, the metrics error / iters / retries / total_iters equal to the emulation, and
the error ratio EQUAL to it (the device's division is the correctly rounded __fdiv_rn; no 1-ulp
allowance is needed or given).  Device-side assumptions this rests on: correctly rounded sqrtf
and division, fl(a * b) from the float32 MFMA chain for a single non-zero term, no flush to zero
of these well-scaled operands, powf within 1 ulp of the host's.

Family 2, dense blocks A = 64 I + E (E in {-1, 0, 1}), ridge_epsilon = 0, num_iters = k in
{1, 2, 3}: no later step corrects an error made in those k.  sumsq is an exact integer below 2^24
(asserted), so M0, Mi0 and H1 = fl(h0 Mi0) are known exactly: k = 1 is bit for bit (which also
fixes the h0 candidate), k = 2, 3 are compared element by element with a float64 evaluation of
the same steps under the bound derived in _newton_exact (any summation order; on the symmetric
path plus the mirror / averaging terms).  The bound is derived; the observed ratio is printed for
information.  With ridge 0 every try is the same computation, and a try is repeated while its
error is above 0.05: PS_M_RETRIES is 6 there (1 where k steps already bring max|M - I| below 0.05,
which the well-conditioned small blocks do for p >= 4, k = 3), PS_M_ITERS is k.

symmetry='assume' is a promise a non-symmetric block breaks, so that block runs under 'verify' and
'general' only; averaged_err_threshold (an opt-in) and the bf16 product modes are not covered.

Observed on an MI355X (50 tests, 7 s):
  Family 1: all four device-side assumptions held; every block matched one h0 candidate bit for
    bit in every option set (about 75 % the host's powf, the rest one neighbour up or down), the
    error ratio always equal.  One fault found and fixed: powf(z, 1.0f) is not the identity on the
    device (n = 513, p = 1, z = 0.059479553: h0 one ulp low, every element explained by that shift
    alone); pth_root_of_scale now returns z for p = 1.
  Family 2: k = 1 bit for bit everywhere; worst err / bound 0.41 at k = 2 (n = 512) and 0.22 at
    k = 3, the symmetric path and the full products within 0.03 of each other; 'verify' gave the
    bits of 'general' on every non-symmetric block.
"""
import functools

import numpy as np
import pytest
import torch

from tests import _newton_exact as N
from tests._exact import ulp_distance

pytestmark = pytest.mark.gpu

SENT = -777.25
M_ERROR, M_ITERS, M_RATIO, M_RETRIES, M_TOTAL = 0, 1, 2, 4, 5

DIAG_SIZES = [1, 2, 127, 128, 129, 255, 256, 257, 384, 511, 513, 1024, 1025]
DIAG_PS = [1, 2, 3, 4, 6, 8, 16]
DENSE_SIZES = [96, 128, 129, 257, 384, 512, 1024]
DENSE_PS = [1, 2, 3, 4, 8]

EXEC_ACCUM = [(e, a) for e in ("staged", "persistent") for a in ("segmented", "chain")]
# (name, options, symmetry, hint marks every block fast).  products = f32 everywhere (the default;
# the bf16 split modes are not exact on these inputs and out of scope).
OPTION_SETS = [
    ("staged-segmented", dict(execution="staged", accumulation="segmented"), "verify", False),
    ("staged-chain", dict(execution="staged", accumulation="chain"), "verify", False),
    ("persistent-segmented", dict(execution="persistent", accumulation="segmented"), "verify", False),
    ("persistent-chain", dict(execution="persistent", accumulation="chain"), "verify", False),
    ("averaged-0", dict(averaged_steps=0), "verify", False),
    ("averaged-100", dict(averaged_steps=100), "verify", False),
    ("persistent-averaged-100", dict(execution="persistent", averaged_steps=100), "verify", False),
    ("assume", dict(), "assume", False),
    ("general", dict(), "general", False),
    ("persistent-general-chain", dict(execution="persistent", accumulation="chain"), "general", False),
    ("hint-fast", dict(), "verify", True),
    ("persistent-hint-fast", dict(execution="persistent"), "verify", True),
]
OPTION_IDS = [o[0] for o in OPTION_SETS]


def K():
  from precondition_amd import kernels
  return kernels


# ---------------------------------------------------------------------------
# embedding: blocks inside larger buffers, garbage in the padding, framed outputs
# ---------------------------------------------------------------------------
_GARBAGE = (float("nan"), float("inf"), -1e30, float("-inf"))


class Embedded:
  """One block of effective size n inside an n_full x n_full input (padding_start = n < n_full
  for three idx out of four), lda > n_full, non-finite or large garbage everywhere outside
  [0, n)^2, and an output that is a strided view (ldo > n_full, offset 1 or 4 floats, so both the
  float4 and the scalar copy-out run) of a sentinel-filled holder with a frame on all sides."""

  def __init__(self, block, idx, dev):
    n = block.shape[0]
    self.n = n
    pad = (0, 3, 4 + (-n) % 4, 5)[idx % 4]
    self.n_full = nf = n + pad
    lda = nf + (1, 4, 7)[idx % 3]
    buf = torch.full((nf, lda), _GARBAGE[idx % 4], dtype=torch.float32, device=dev)
    buf[:n, :n] = torch.from_numpy(np.ascontiguousarray(block, np.float32)).to(dev)
    self.a = buf[:, :nf]
    self.off = off = (4, 1)[idx % 2]
    self.holder = torch.full((nf + 2, nf + off + (4 - nf % 4) % 4 + (0, 3)[idx % 2]), SENT,
                             dtype=torch.float32, device=dev)
    self.out = self.holder[1:nf + 1, off:off + nf]

  def expected_holder(self, root):
    exp = np.full(tuple(self.holder.shape), SENT, np.float32)
    exp[1:self.n_full + 1, self.off:self.off + self.n_full] = 0.0
    exp[1:self.n + 1, self.off:self.off + self.n] = root
    return exp

  def result(self):
    return self.holder.cpu().numpy()

  def root(self, holder=None):
    h = self.result() if holder is None else holder
    return h[1:self.n + 1, self.off:self.off + self.n]


def _call(embs, ps, options, symmetry, fast, num_iters, ridge):
  opts = dict(options)
  opts["products"] = "f32"
  if fast:
    opts["iters_hint"] = np.ones(len(embs), np.float32)   # in [1, fast_max_iters]: no averaged steps
  _, metrics = K().matrix_inverse_pth_root_batched(
      [e.a for e in embs], list(ps), [e.n for e in embs], num_iters=num_iters, ridge_epsilon=ridge,
      relative_matrix_epsilon=False, out=[e.out for e in embs], symmetry=symmetry, options=opts)
  torch.cuda.synchronize()
  return metrics.cpu().numpy()


def _same_f32(a, b):
  a, b = np.float32(a), np.float32(b)
  return bool(a == b) or bool(np.isnan(a) and np.isnan(b))


def _assert_holder(got, exp, what):
  """Whole holder: values equal everywhere (frame, zeros, root), the root's bits equal."""
  if not np.array_equal(got, exp):
    bad = np.argwhere(got != exp)
    r, c = bad[0]
    raise AssertionError(f"{what}: {len(bad)} of {got.size} holder elements differ; first at ({r}, {c}): "
                         f"got {got[r, c]!r}, expected {exp[r, c]!r}; rows {bad[:, 0].min()}..{bad[:, 0].max()}, "
                         f"cols {bad[:, 1].min()}..{bad[:, 1].max()}")


# ---------------------------------------------------------------------------
# Family 1: diagonal blocks
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _diag_expect(kind, n, p, salt, shift):
  return N.diag_root_emulate(N.diag_spectrum(n, kind, salt), p, N.DIAG_RIDGE, shift=shift)


def _check_diag_block(emb, kind, p, salt, mrow, what, tally):
  got = emb.result()
  diag = np.ascontiguousarray(np.diagonal(emb.root(got)))
  matched = None
  for shift in N.h0_shifts(p):
    exp_d, exp_m = _diag_expect(kind, emb.n, p, salt, shift)
    if ulp_distance(diag, exp_d).max() == 0:
      matched = shift
      break
  if matched is None:
    exp_d, _ = _diag_expect(kind, emb.n, p, salt, 0)
    dist = ulp_distance(diag, exp_d) if np.all(np.isfinite(diag)) else None
    raise AssertionError(f"{what}: the diagonal matches none of the h0 candidates {N.h0_shifts(p)}; against "
                         f"the host's powf: max ulp distance {None if dist is None else dist.max()}, first "
                         f"elements got {diag[:4]!r} expected {exp_d[:4]!r}")
  tally[matched] = tally.get(matched, 0) + 1
  _assert_holder(got, emb.expected_holder(np.diag(exp_d)), what)
  assert _same_f32(mrow[M_ERROR], exp_m["error"]), (what, "error", mrow, exp_m)
  assert mrow[M_ITERS] == exp_m["iters"], (what, "iters", mrow, exp_m)
  assert mrow[M_RETRIES] == exp_m["retries"], (what, "retries", mrow, exp_m)
  assert mrow[M_TOTAL] == exp_m["total_iters"], (what, "total_iters", mrow, exp_m)
  # equal, not within 1 ulp: __fdiv_rn is the correctly rounded division the host does
  assert _same_f32(mrow[M_RATIO], exp_m["ratio"]), (what, "error ratio", mrow, exp_m)


def _diag_grid():
  """(kind, n, p, salt) of the mixed call: every size x every exponent on the 'full' spectrum,
  plus the equal / spread / retry blocks at the sizes around the tile edges."""
  cases = [("full", n, p, n + p) for n in DIAG_SIZES for p in DIAG_PS]
  for kind in ("equal", "spread", "retry"):
    for j, n in enumerate((2, 129, 256, 513, 1025)):
      for p in (DIAG_PS[j % 7], DIAG_PS[(j + 3) % 7], 4):
        cases.append((kind, n, p, n + p))
  return cases


def _diag_embed(cases, dev):
  return [Embedded(np.diag(N.diag_spectrum(n, kind, salt)), i, dev)
          for i, (kind, n, p, salt) in enumerate(cases)]


@pytest.mark.parametrize("name,options,symmetry,fast", OPTION_SETS, ids=OPTION_IDS)
def test_diag_mixed_call(device, name, options, symmetry, fast):
  """All sizes, exponents and spectra in ONE call, per option set, against the same expectation."""
  cases = _diag_grid()
  embs = _diag_embed(cases, device)
  metrics = _call(embs, [c[2] for c in cases], options, symmetry, fast, 100, N.DIAG_RIDGE)
  tally = {}
  for i, (emb, (kind, n, p, salt)) in enumerate(zip(embs, cases)):
    _check_diag_block(emb, kind, p, salt, metrics[i], (name, kind, n, p), tally)
  assert any(c[0] == "retry" and metrics[i][M_RETRIES] == 2 for i, c in enumerate(cases))
  assert any(c[0] == "spread" and metrics[i][M_ITERS] > 10 for i, c in enumerate(cases))
  print(f"[{name}] {len(cases)} diagonal blocks; h0 candidate (shift in float32 neighbours of the host's "
        f"powf) -> blocks: {dict(sorted(tally.items()))}")


@pytest.mark.parametrize("n", DIAG_SIZES)
def test_diag_single_block_calls(device, n):
  """Every size x exponent as a call of its own, both executions x both accumulations; the
  staged-segmented result of each is then compared bit for bit with the same block inside a mixed
  call of all exponents and spectra of this size."""
  tally = {}
  single = {}
  cases = [("full", n, p, n + p) for p in DIAG_PS]
  cases += [(kind, n, 4, n + 4) for kind in ("equal", "spread")] + ([("retry", n, 2, n + 2)] if n >= 2 else [])
  for i, (kind, _, p, salt) in enumerate(cases):
    for execution, accumulation in EXEC_ACCUM:
      if kind != "full" and (execution, accumulation) != EXEC_ACCUM[0] and n not in (129, 1025):
        continue
      emb = Embedded(np.diag(N.diag_spectrum(n, kind, salt)), i + EXEC_ACCUM.index((execution, accumulation)), device)
      m = _call([emb], [p], dict(execution=execution, accumulation=accumulation), "verify", False, 100,
                N.DIAG_RIDGE)
      _check_diag_block(emb, kind, p, salt, m[0], (execution, accumulation, kind, n, p), tally)
      if (execution, accumulation) == EXEC_ACCUM[0]:
        single[i] = (emb.root().copy(), m[0].copy())
  embs = [Embedded(np.diag(N.diag_spectrum(n, kind, salt)), i + 1, device)
          for i, (kind, _, p, salt) in enumerate(cases)]
  metrics = _call(embs, [c[2] for c in cases], {}, "verify", False, 100, N.DIAG_RIDGE)
  for i, emb in enumerate(embs):
    root, mrow = single[i]
    assert np.array_equal(emb.root().view(np.int32), root.view(np.int32)), ("mixed != single", cases[i])
    assert np.array_equal(metrics[i][:6].view(np.int32), mrow[:6].view(np.int32)), ("metrics", cases[i])
  print(f"n={n}: h0 candidate -> calls: {dict(sorted(tally.items()))}")


# ---------------------------------------------------------------------------
# Family 2: dense blocks, step-limited
# ---------------------------------------------------------------------------
def _dense_ps(n):
  return [4] if n == 1024 else DENSE_PS


@functools.lru_cache(maxsize=None)
def _dense_block(n, p, symmetric):
  return N.dense_case(n, 100 * n + p, symmetric)


@functools.lru_cache(maxsize=16)
def _dense_expect(n, p, symmetric, shift, sym_path):
  """(init, [(H64_k, E_k)], errs of the float32 restatement) for k = 1..3."""
  init = N.dense_init(_dense_block(n, p, symmetric), p, shift)   # asserts the exact sumsq
  return init, N.dense_bound(init, 3, symmetric=sym_path), N.dense_steps_f32(init, 3)[1]


def _find_shift(root, n, p, symmetric, what):
  for shift in N.h0_shifts(p):
    init = N.dense_init(_dense_block(n, p, symmetric), p, shift)
    if np.array_equal(root.view(np.int32), init["H1"].view(np.int32)):
      return shift
  init = N.dense_init(_dense_block(n, p, symmetric), p, 0)
  bad = np.argwhere(root != init["H1"])
  raise AssertionError(f"{what}: H_1 = fl(h0 Mi0) matches none of the h0 candidates; against the host's powf "
                       f"{len(bad)} of {root.size} elements differ, first at {tuple(bad[0])}")


def _check_dense_metrics(mrow, k, errs, what):
  assert mrow[M_ITERS] == k, (what, mrow)
  assert mrow[M_RATIO] < 1.2, (what, mrow)        # the try converges: H_k is what is returned
  retries = 6 if mrow[M_ERROR] > 0.05 else 1     # the loop control's own decision ...
  if abs(float(errs[k - 1]) - 0.05) > 0.005:      # ... which the restatement predicts off the edge
    assert retries == (6 if errs[k - 1] > 0.05 else 1), (what, mrow, errs)
  assert mrow[M_RETRIES] == retries and mrow[M_TOTAL] == retries * k, (what, mrow)


@pytest.mark.parametrize("n", DENSE_SIZES)
def test_dense_step_limited(device, n):
  """Every exponent of this size (and one non-symmetric block, p = 4) in one call per option set
  and k.  k = 1: bit for bit.  k = 2, 3: |H_k - H64_k| <= E_k element by element.  The
  non-symmetric block must come out of symmetry='verify' with the bits of 'general'.

  Observed worst err / bound on an MI355X: see the module docstring."""
  blocks = [(p, True) for p in _dense_ps(n)] + [(4, False)]
  shifts = {}
  worst = {}
  nonsym_bits = {}
  saw6 = False
  for name, options, symmetry, fast in OPTION_SETS:
    for k in (1, 2, 3):
      # symmetry='assume' is a promise the non-symmetric block would break: it stays out of that call
      called = [b for b in blocks if b[1] or symmetry != "assume"]
      embs = [Embedded(_dense_block(n, p, s), 2 * i + k, device) for i, (p, s) in enumerate(called)]
      metrics = _call(embs, [b[0] for b in called], options, symmetry, fast, k, 0.0)
      for i, (emb, (p, s)) in enumerate(zip(embs, called)):
        what = (name, n, p, "symmetric" if s else "non-symmetric", k)
        got = emb.result()
        root = np.ascontiguousarray(emb.root(got))
        if (p, s) not in shifts:
          assert k == 1
          shifts[(p, s)] = _find_shift(root, n, p, s, what)
        sym_path = s and symmetry != "general"
        init, bound, errs = _dense_expect(n, p, s, shifts[(p, s)], sym_path)
        _check_dense_metrics(metrics[i], k, errs, what)
        saw6 |= metrics[i][M_RETRIES] == 6
        if k == 1:
          _assert_holder(got, emb.expected_holder(init["H1"]), what)
          assert np.array_equal(root.view(np.int32), init["H1"].view(np.int32)), what
        else:
          ref64, e = bound[k - 1]
          _assert_holder(got, emb.expected_holder(root), what)    # frame and padding
          r = N.worst_ratio(root, ref64, e)
          key = (k, "symmetric path" if sym_path else "full products")
          worst[key] = max(worst.get(key, 0.0), r)
          if r > 1.0:
            err = np.abs(root.astype(np.float64) - ref64)
            bad = np.argwhere(err > e)
            raise AssertionError(f"{what}: {len(bad)} elements outside the derived bound, worst err / bound "
                                 f"{r:.3g}; first at {tuple(bad[0])}, rows {bad[:, 0].min()}..{bad[:, 0].max()}, "
                                 f"cols {bad[:, 1].min()}..{bad[:, 1].max()}")
          if sym_path:
            assert np.array_equal(root, root.T), (what, "the symmetric path's result is not bitwise symmetric")
        if not s and name in ("staged-segmented", "general"):
          nonsym_bits[(name, k)] = root.copy()
  for k in (1, 2, 3):
    assert np.array_equal(nonsym_bits[("staged-segmented", k)].view(np.int32),
                          nonsym_bits[("general", k)].view(np.int32)), ("verify != general", n, k)
  assert saw6
  print(f"n={n}: h0 candidates {shifts}; worst err / bound " +
        ", ".join(f"k={k} {path}: {v:.3f}" for (k, path), v in sorted(worst.items())))


def test_dense_mixed_call_equals_single_block_calls(device):
  """All sizes and exponents in one call (k = 2 and 3, default options): every block bit for bit
  what its single-block call returns (whose elements test_dense_step_limited bounds)."""
  blocks = [(n, p, True) for n in DENSE_SIZES for p in _dense_ps(n)] + [(129, 4, False), (384, 3, False)]
  for k in (2, 3):
    embs = [Embedded(_dense_block(n, p, s), i, device) for i, (n, p, s) in enumerate(blocks)]
    metrics = _call(embs, [b[1] for b in blocks], {}, "verify", False, k, 0.0)
    for i, (n, p, s) in enumerate(blocks):
      one = Embedded(_dense_block(n, p, s), i + 1, device)
      m1 = _call([one], [p], {}, "verify", False, k, 0.0)
      assert np.array_equal(embs[i].root().view(np.int32), one.root().view(np.int32)), (n, p, s, k)
      assert np.array_equal(metrics[i][:6].view(np.int32), m1[0][:6].view(np.int32)), (n, p, s, k)


# ---------------------------------------------------------------------------
# ps_mat_power_f32: integer exactness
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,density", N.MAT_POWER_CASES)
def test_mat_power_integer_exact(device, n, p, density):
  """Entries in {-1, 0, 1}, max |A|^q < 2^24 for q <= p (asserted by the case builder): A^p is
  the int64 power exactly, whatever the summation order.  ldm and ldo above n, sentinel frame."""
  from precondition_amd import _lib
  a, ref = N.mat_power_int_case(n, p, density)
  L = _lib.lib()
  for case, (ldm_pad, off) in enumerate(((3, 1), (4, 4))):
    src = torch.full((n, n + ldm_pad), float("nan"), dtype=torch.float32, device=device)
    src[:, :n] = torch.from_numpy(a.astype(np.float32)).to(device)
    holder = torch.full((n + 2, n + off + 3), SENT, dtype=torch.float32, device=device)
    out = holder[1:n + 1, off:off + n]
    ws = torch.empty(max(int(L.ps_mat_power_workspace_bytes(n, p)), 256), dtype=torch.uint8, device=device)
    rc = L.ps_mat_power_f32(torch.cuda.current_stream().cuda_stream, src.data_ptr(), n, n + ldm_pad, p,
                            out.data_ptr(), holder.stride(0), ws.data_ptr(), ws.numel())
    assert rc == 0, rc
    torch.cuda.synchronize()
    exp = np.full(tuple(holder.shape), SENT, np.float64)
    exp[1:n + 1, off:off + n] = ref
    _assert_holder(holder.cpu().numpy().astype(np.float64), exp, (n, p, case))
