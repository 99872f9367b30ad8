"""pi_block_kernel (one workgroup per block of up to 512 x 512) against the library's own streaming
execution of the same inputs (pi_mv_kernel / pi_red_kernel), BIT FOR BIT: lambda, iters, stop_iter
and the iterate.  The kernel's contract is that it repeats the streaming kernels add for add
(precondition_amd/csrc/power_iter.hip.h); its row sums are reduced sixteen at a time by a transposing butterfly,
and this file is what pins that the butterfly keeps every row's summation tree.

Expected values come from the streaming execution and from the float64 loop of tests/_pi_exact.py
only; nothing is compared with an earlier output of the kernel under test.  All blocks of a size
run in ONE batched call (six workgroups at once): a symmetric block, one made asymmetric in a single
off-diagonal element (full mat-vec paths), one cut by padding_start with NaN behind it, a Wishart
block that needs all 100 steps, a block with one dominant eigenvalue that stops by the tolerance
rule, and an all-zero block (0 / 0 of DS:634).  Sizes: t = 2, 3, 4 tiles per side (t = 3 has an odd
number of off-diagonal tiles: one thread group idles a round), edges that are no multiple of 4,
padding inside the last tile.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _pi_exact as P

pytestmark = pytest.mark.gpu

SIZES = (129, 200, 256, 257, 384, 511, 512)
NUM_ITERS, TOL = 100, 1e-6
STREAMING = {"power_iteration": "streaming"}

# Seed of the Wishart block G G^T (G: n x n standard normal) per size: the first whose float64 run
# takes all 100 steps with every |ds| >= 64 ulp(lambda).  tol is below one ulp of s here, so float32
# stops early only if two consecutive s agree exactly; its s is off by a few ulp at most
# (sqrt(n) u s is 1.4 ulp at n = 512), which 64 ulp keeps well away.  Chosen from float64 alone.
WISHART_SEED = {129: 2, 200: 9, 256: 0, 257: 1, 384: 2, 511: 0, 512: 2}
# Steps of the float64 reference on `dominant(n)`, recorded: |ds| falls by 100 per step (eigenvalue
# ratio 1 / 10, squared) and passes tol = 1e-6 in step 6 or 7.  s is 0.625: tol is 16.8 float32 ulp
# of it, so the few ulp by which the float32 s of a converged iterate still moves stay below tol and
# the float32 executions stop within a step of these counts -- far below 30.  (At diag(10, 1, ...)
# itself one ulp of s is 0.95 tol: the float32 s may flicker by two ulp for all 100 steps.)
DOMINANT_STEPS64 = {129: 6, 200: 7, 256: 7, 257: 7, 384: 7, 511: 7, 512: 7}
EARLY_LIMIT = 30

# PiBlock (power_iter.hip.h), the first array of the workspace: 72 bytes, as int32 words
PB_WORDS, PB_N, PB_STOP_ITER, PB_ITERS = 18, 3, 11, 13


def wishart(n, seed):
  g = np.random.default_rng([21, seed, n]).standard_normal((n, n)).astype(P.F32)
  a = (g @ g.T).astype(P.F32)
  return np.ascontiguousarray(np.triu(a) + np.triu(a, 1).T)


def dominant(n):
  """diag(10, 1, ..., 1) plus symmetric noise of 1e-3, all of it divided by 16 (exact)."""
  g = np.random.default_rng([22, 0, n]).uniform(-1e-3, 1e-3, (n, n)).astype(P.F32)
  a = np.triu(g) + np.triu(g, 1).T
  a[np.arange(n), np.arange(n)] += 1.0
  a[0, 0] += 9.0
  return np.ascontiguousarray((a / 16.0).astype(P.F32))


@functools.lru_cache(maxsize=None)
def batch_of(n):
  """[(name, matrix, padding_start)] of size n, and the float64 runs the test needs."""
  pad = n - 3
  blocks = (("symmetric", P.matrix("sym", n), n),
            ("one asymmetric element", P.single_defect(n, 1, n - 1), n),
            ("padding_start below n", P.padded("sym", n, pad), pad),
            ("wishart", wishart(n, WISHART_SEED[n]), n),
            ("dominant", dominant(n), n),
            ("zero", np.zeros((n, n), P.F32), n))
  refs = {"wishart": P.reference64(blocks[3][1], n, NUM_ITERS, TOL),
          "dominant": P.reference64(blocks[4][1], n, NUM_ITERS, TOL)}
  return blocks, refs


def run(mats, pads, options):
  """P.run_pi, returning the PiBlock words of the workspace as well."""
  from precondition_amd import _lib
  L = _lib.lib()
  batch, dev = len(mats), mats[0].device
  i32 = lambda xs: np.ascontiguousarray(np.asarray(xs, dtype=np.int32))
  n, lda, pad = i32([m.shape[0] for m in mats]), i32([P.ld_of(m) for m in mats]), i32(pads)
  ldv = int(n.max())
  lam = torch.full((batch,), P.SENTINEL, dtype=torch.float32, device=dev)
  its = torch.full((batch,), P.SENTINEL_IT, dtype=torch.int32, device=dev)
  V = torch.full((batch, ldv), P.SENTINEL, dtype=torch.float32, device=dev)
  ws = torch.zeros(max(int(L.ps_power_iteration_workspace_bytes(batch, n.ctypes.data)), 256),
                   dtype=torch.uint8, device=dev)
  ptrs = np.ascontiguousarray(np.asarray([m.data_ptr() for m in mats], dtype=np.uint64))
  popt, _keep = _lib.make_options(options)
  with torch.cuda.device(dev):
    rc = L.ps_power_iteration_batched_opt_f32(
        torch.cuda.current_stream().cuda_stream, ptrs.ctypes.data, n.ctypes.data, lda.ctypes.data,
        pad.ctypes.data, batch, NUM_ITERS, TOL, lam.data_ptr(), its.data_ptr(), V.data_ptr(), ldv,
        _lib.symmetry_code("verify"), ws.data_ptr(), ws.numel(), C.byref(popt))
    torch.cuda.synchronize()
  assert rc == 0
  pb = ws[:4 * PB_WORDS * batch].cpu().numpy().view(np.int32).reshape(batch, PB_WORDS)
  assert np.array_equal(pb[:, PB_N], pad), "PiBlock layout changed: update the PB_* words"
  return lam.cpu().numpy(), its.cpu().numpy(), V.cpu().numpy(), pb[:, PB_STOP_ITER].copy(), pb[:, PB_ITERS].copy()


def health():
  from precondition_amd import _lib
  e, c, r = C.c_uint(), C.c_int(), C.c_int()
  assert _lib.lib().ps_power_iteration_health(C.addressof(e), C.addressof(c), C.addressof(r)) == 0
  return e.value, c.value, r.value


def bits(x):
  return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("n", SIZES)
def test_block_kernel_repeats_the_streaming_kernels_bit_for_bit(device, n):
  from precondition_amd import _lib
  blocks, refs = batch_of(n)
  # float64, on the CPU: the cases are what their names say
  assert refs["wishart"].iters == NUM_ITERS
  assert min(st["ds"] for st in refs["wishart"].steps) >= 64 * refs["wishart"].lam * 2.0 ** -23
  assert refs["dominant"].iters == DOMINANT_STEPS64[n] < EARLY_LIMIT
  mats = [torch.from_numpy(np.array(a)).to(device) for _, a, _ in blocks]
  pads = [pad for _, _, pad in blocks]
  want = run(mats, pads, STREAMING)
  _lib.lib().ps_power_iteration_reset_health()
  assert health() == (0, 0, 1)
  got = run(mats, pads, None)
  assert health()[0] == 0, "a wait expired: the call fell back to the streaming kernels"
  lam, its, V, stop, pb_its = want
  for b, (name, _, pad) in enumerate(blocks):
    tag = (n, name)
    print(tag, "streaming: lambda", lam[b], "iters", its[b], "block kernel: lambda", got[0][b],
          "iters", got[1][b], "iterate words that differ", int((bits(V[b]) != bits(got[2][b])).sum()))
    # the streaming execution itself, against float64 and its own bookkeeping
    assert stop[b] == its[b] - 1 and pb_its[b] == its[b], tag
    assert (V[b, pad:] == P.SENTINEL).all(), tag
    if name == "zero":
      assert its[b] == 1 and lam[b] == 0.0 and np.isnan(V[b, :pad]).all(), tag
    else:
      assert np.isfinite(lam[b]) and np.isfinite(V[b, :pad]).all(), tag
    if name == "wishart":
      assert its[b] == NUM_ITERS, tag
    if name == "dominant":
      assert its[b] < EARLY_LIMIT, tag
    # the kernel under test: the same bits
    assert bits(got[0])[b] == bits(lam)[b], (tag, "lambda", float(got[0][b]), float(lam[b]))
    assert got[1][b] == its[b], (tag, "iters", int(got[1][b]), int(its[b]))
    assert got[3][b] == stop[b] and got[4][b] == pb_its[b], (tag, "stop_iter", int(got[3][b]), int(stop[b]))
    assert np.array_equal(bits(got[2][b]), bits(V[b])), (tag, "iterate")
