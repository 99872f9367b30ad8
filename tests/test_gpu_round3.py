"""Round-3 GPU tests (through the C-ABI):

* the register-resident power iteration (DS:595-652) next to a kernel that holds half of the
  CUs on another stream: correct (bit-identical to the streaming execution) when the team mates
  become resident late, and -- with a short deadline -- the bounded waits expire, the Newton
  root re-runs the call on the streaming kernels and still matches the oracle, and the process
  stays on the streaming execution until the health record is reset;
* ps_collective_in_flight switches the resident execution off while an asynchronous gather is
  in flight (what comm.sharded_inverse_pth_roots brackets its RCCL calls with);
* the eigh root path of blocks of more than 128 rows (DS:943-1030): one-sided block Jacobi on the
  Cholesky factor against the oracle's LAPACK root, the fallback for inputs that are not
  positive definite, mixed batches, and both executions of the sweep loop;
* ps_diag_mfma_clock returns a plausible clock; ps_diag_mfma_mix shows the VALU / MFMA trade;
* round-3 product kernel: roots of symmetric inputs are bitwise symmetric; the K-loop variants and
  the traced kernel are bit-identical.
"""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

from oracle import shampoo_oracle as orc

pytestmark = pytest.mark.gpu


def K():
  from precondition_amd import kernels
  return kernels


def L():
  from precondition_amd import _lib
  return _lib.lib()


def wishart(n, k, seed):
  g = np.random.default_rng(seed).standard_normal((n, k)).astype(np.float32)
  return (g @ g.T).astype(np.float32)


def health():
  e, c, r = C.c_uint(), C.c_int(), C.c_int()
  assert L().ps_power_iteration_health(C.addressof(e), C.addressof(c), C.addressof(r)) == 0
  return e.value, c.value, r.value


def hold_half_of_the_cus(stream, ms, cus=128):   # or most of them
  """`cus` workgroups of 1024 threads with 150 KB of LDS each: one per CU, and nothing of the
  resident power iteration (13 KB of LDS per workgroup) fits beside one."""
  assert L().ps_diag_spin(stream.cuda_stream, cus, 1024, 150 * 1024, float(ms)) == 0


# ---------------------------------------------------------------------------
def test_collective_in_flight_switches_resident_execution_off(device):
  L().ps_power_iteration_reset_health()
  assert health() == (0, 0, 1)
  assert L().ps_collective_in_flight(1) == 1
  assert health() == (0, 1, 0)
  a = torch.tensor(wishart(256, 1024, 5), device=device)
  lam_stream, _ = K().power_iteration_batched([a])     # streaming kernels
  assert L().ps_collective_in_flight(-1) == 0
  assert health() == (0, 0, 1)
  lam_res, _ = K().power_iteration_batched([a])        # resident kernel
  assert torch.equal(lam_stream, lam_res)              # same arithmetic, bit for bit


def test_resident_power_iteration_beside_a_kernel_holding_most_cus(device, monkeypatch):
  """A kernel on another stream holds 250 of the 256 CUs for 150 ms.  Workgroups are dealt to
  the XCDs round-robin and an XCD without a free CU dispatches nothing, so teams of the resident
  launch are split until the filler ends: the team mates that did become resident wait (bounded:
  5 s by default), the iteration is delayed, and nothing else happens -- eigenvalues equal the
  streaming execution's bit for bit, no wait expires.  (Next to a filler on HALF of the CUs the
  launch is not even delayed: the free slots hold a prefix of the teams.)"""
  L().ps_power_iteration_reset_health()
  mats = [torch.tensor(wishart(512, 2048, 100 + i), device=device) for i in range(160)]
  monkeypatch.setenv("PS_PI_RESIDENT", "0")
  lam_ref, it_ref = K().power_iteration_batched(mats)
  monkeypatch.setenv("PS_PI_RESIDENT", "1")
  torch.cuda.synchronize()
  side = torch.cuda.Stream(device=device)
  hold_half_of_the_cus(side, 150.0, cus=250)
  time.sleep(0.01)
  t0 = time.perf_counter()
  lam, it = K().power_iteration_batched(mats)
  torch.cuda.current_stream().synchronize()
  delayed = time.perf_counter() - t0   # normally > 50 ms (the filler holds 250 CUs for 150 ms): not asserted, it is
  # the scheduler's behaviour, not the library's -- what must hold is the result and the absence of an expired wait
  assert delayed < 5.0
  torch.cuda.synchronize()
  assert torch.equal(lam, lam_ref) and torch.equal(it, it_ref)
  assert health()[0] == 0
  # half of the CUs held: usually no delay at all (the free slots hold a prefix of the teams), but
  # since round 4 a team lives inside ONE XCD, and when the filler's workgroups fill whole XCDs
  # the teams dealt to those wait for it: bounded by the filler, never an expired wait
  hold_half_of_the_cus(side, 150.0, cus=128)
  time.sleep(0.01)
  t0 = time.perf_counter()
  lam, it = K().power_iteration_batched(mats)
  torch.cuda.current_stream().synchronize()
  assert time.perf_counter() - t0 < 1.0
  torch.cuda.synchronize()
  assert torch.equal(lam, lam_ref) and health()[0] == 0


def test_expired_resident_wait_falls_back_to_streaming_in_the_same_call(device, monkeypatch):
  """The recovery path of an expired wait.  (On this hardware a filler kernel could not be made
  to split a team for longer than a deadline: workgroups start in launch order, and with most
  CUs held the whole launch simply starts late -- previous test (dev scripts of round 3, see the git history).  The
  expiry is therefore forced: PS_PI_TIMEOUT_MS=0 makes every wait count as expired.)  The
  resident launch gives up at once (counted in pinned host memory, eigenvalues NaN), the Newton
  root driver sees the count move at its first host wait and runs the call again on the
  streaming kernels: roots and iteration counts match the oracle, nothing is NaN, and the
  process stays on the streaming execution until the record is reset."""
  L().ps_power_iteration_reset_health()
  arrs = [wishart(512, 2048, 300 + i) for i in range(24)]
  mats = [torch.tensor(a, device=device) for a in arrs]
  monkeypatch.setenv("PS_PI_TIMEOUT_MS", "0")
  roots, met = K().matrix_inverse_pth_root_batched(mats, [4] * len(mats))
  torch.cuda.synchronize()
  met = met.cpu().numpy()
  expired, _, resident = health()
  assert expired > 0 and resident == 0, (expired, resident)
  assert np.isfinite(met[:, :5]).all()
  for i in (0, 23):
    h_ref, m_ref = orc.matrix_inverse_pth_root(arrs[i], 4)
    h = roots[i].cpu().numpy()
    assert np.linalg.norm(h - h_ref) / np.linalg.norm(h_ref) < 5e-5
    assert met[i, 1] == m_ref["inverse_pth_root_iters"] and met[i, 4] == m_ref["total_retries"]
    assert np.isclose(met[i, 3], m_ref["max_eigen_value"], rtol=2e-5)
  # the eigh root driver recovers the same way (its first host wait is behind the Cholesky
  # factorisation); the process is already on the streaming execution here, so force a new expiry
  L().ps_power_iteration_reset_health()
  big = [torch.tensor(wishart(256, 1024, 7), device=device)]
  r_e, m_e = K().matrix_inverse_pth_root_batched(big, [2], eigh=True)
  assert health()[0] > 0
  h_ref, _ = orc.matrix_inverse_pth_root_eigh(big[0].cpu().numpy(), 2)
  assert np.linalg.norm(r_e[0].cpu().numpy() - h_ref) / np.linalg.norm(h_ref) < 1e-4
  # a standalone call has no host wait to recover at: with a real expiry its result would be NaN,
  # which is why the process stays on the streaming execution after the first one
  monkeypatch.delenv("PS_PI_TIMEOUT_MS")
  lam, _ = K().power_iteration_batched(mats)
  assert np.array_equal(lam.cpu().numpy(), met[:, 3])
  L().ps_power_iteration_reset_health()
  assert health() == (0, 0, 1)


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,p", [(256, 1024, 2), (384, 768, 4), (1000, 2000, 2), (200, 800, 2)])
def test_eigh_root_cholesky_jacobi_vs_oracle(n, k, p, device):
  """matrix_inverse_pth_root_eigh (DS:943-1030) through the one-sided block Jacobi on the
  Cholesky factor (csrc/eigh_cj.hip.h; n = 200 pads to 256) against the oracle's LAPACK root:
  1e-4 on the root (north_star's bar), error metric of the same size as LAPACK's."""
  a = wishart(n, k, n + p)
  h_ref, m_ref = orc.matrix_inverse_pth_root_eigh(a, p)
  roots, met = K().matrix_inverse_pth_root_batched([torch.tensor(a, device=device)], [p], eigh=True,
                                                   options={"eigh_solver": "one_sided"})
  h = roots[0].cpu().numpy()
  met = met.cpu().numpy()
  assert np.linalg.norm(h - h_ref) / np.linalg.norm(h_ref) < 1e-4
  assert np.abs(h - h.T).max() <= 1e-5 * np.abs(h).max()
  lam = float(np.linalg.eigvalsh(a.astype(np.float64)).max())
  assert met[0, 0] < 1e-5 * lam and met[0, 0] < 0.1, met[0]
  assert 3 <= met[0, 5] <= 24   # sweeps


def test_eigh_root_two_sided_fallback_for_indefinite_input(device, monkeypatch):
  """An input that is not positive definite after the ridge (eigenvalues -0.5 ... 2) cannot be
  Cholesky-factored: the block is handed to the blocked two-sided solver inside the same call,
  next to a positive definite block that stays on the one-sided path; both match the oracle."""
  rng = np.random.default_rng(9)
  q, _ = np.linalg.qr(rng.standard_normal((256, 256)))
  bad = ((q * np.linspace(-0.5, 2.0, 256)) @ q.T)
  bad = ((bad + bad.T) / 2).astype(np.float32)
  good = wishart(256, 1024, 3)
  mats = [torch.tensor(good, device=device), torch.tensor(bad, device=device),
          torch.tensor(wishart(300, 900, 4), device=device)]
  # default solver (round 5): the tridiagonalisation path keeps the two positive definite blocks and
  # hands the indefinite one to the Jacobi solvers (Cholesky breakdown -> two-sided) inside the call
  for opts in (None, {"eigh_solver": "one_sided"}):
    roots, met = K().matrix_inverse_pth_root_batched(mats, [2, 2, 2], eigh=True, options=opts)
    for m, h in zip(mats, roots):
      h_ref, _ = orc.matrix_inverse_pth_root_eigh(m.cpu().numpy(), 2)
      rel = np.linalg.norm(h.cpu().numpy() - h_ref) / np.linalg.norm(h_ref)
      assert rel < 2e-4, (opts, rel)
  # the same batch on the two-sided solver alone
  roots2, _ = K().matrix_inverse_pth_root_batched(mats, [2, 2, 2], eigh=True,
                                                  options={"eigh_solver": "two_sided"})
  assert torch.allclose(roots[1], roots2[1], rtol=0, atol=2e-4 * float(roots2[1].abs().max()))


def test_eigh_root_one_stream_and_two_streams_agree(device):
  """The two stream groups sweep disjoint blocks: results do not depend on the interleaving."""
  mats = [torch.tensor(wishart(256 + 128 * (i % 2), 1024, 40 + i), device=device) for i in range(5)]
  r1, m1 = K().matrix_inverse_pth_root_batched(mats, [2] * 5, eigh=True,
                                               options={"eigh_solver": "one_sided", "eigh_streams": 1})
  r2, m2 = K().matrix_inverse_pth_root_batched(mats, [2] * 5, eigh=True,
                                               options={"eigh_solver": "one_sided", "eigh_streams": 2})
  for a, b in zip(r1, r2):
    assert torch.equal(a, b)
  assert torch.equal(m1, m2)


def test_newton_bf16x6_products_opt_in_mode(device, monkeypatch):
  """PS_NEWTON_PRODUCTS=bf16x6 (three-way bf16 split, six partial products on the bf16 MFMA,
  exact float32 products for the last steps): float32-faithful, NOT the parity path -- roots
  within 1e-4 of the oracle (north_star's bar) and of the default mode, iteration and retry
  counts equal to the default mode's (and the oracle's) on well- and ill-conditioned blocks; blocks that are not exactly
  symmetric run the float32 products in the same launch (bit-identical to the default mode)."""
  rng = np.random.default_rng(5)
  arrs = [wishart(512, 2048, 70), wishart(384, 1536, 71), wishart(1000, 1100, 72)]
  q, _ = np.linalg.qr(rng.standard_normal((640, 640)))
  graded = (q * 1e4 ** (-np.arange(640) / 639.0)) @ q.T
  arrs.append(((graded + graded.T) / 2).astype(np.float32))
  mats = [torch.tensor(a, device=device) for a in arrs]
  ps = [4, 2, 4, 4]
  r32, m32 = K().matrix_inverse_pth_root_batched(mats, ps)
  r16, m16 = K().matrix_inverse_pth_root_batched(mats, ps, options={"products": "bf16x6"})
  m32, m16 = m32.cpu().numpy(), m16.cpu().numpy()
  differs = False
  for i, (a, p) in enumerate(zip(arrs, ps)):
    h_ref, m_ref = orc.matrix_inverse_pth_root(a, p)
    h16, h32 = r16[i].cpu().numpy(), r32[i].cpu().numpy()
    scale = 1e-4 if i != 2 else 5e-3   # 1000 x 1100 Wishart: cond ~1e6, both modes ~1e-3 apart
    assert np.linalg.norm(h16 - h_ref) / np.linalg.norm(h_ref) < scale, i
    assert np.linalg.norm(h16 - h32) / np.linalg.norm(h32) < scale, i
    # same stop decisions as the default mode; the oracle's count is equal too except where the
    # 1e-6 threshold is within rounding of the last error (the cond ~1e6 block: +-1)
    assert abs(m16[i, 1] - m32[i, 1]) <= (1 if i == 2 else 0), (i, m16[i], m32[i])
    assert abs(m16[i, 1] - m_ref["inverse_pth_root_iters"]) <= (1 if i == 2 else 0), i
    assert m16[i, 4] == m_ref["total_retries"] == m32[i, 4], i
    differs |= not np.array_equal(h16, h32)
  assert differs, "the opt-in mode did not run"
  # an asymmetric block takes the float32 products (plain chains: the split-product kernels carry
  # no second accumulator set): bit-identical to the float32 mode with accumulation = "chain"
  asym = arrs[0].copy(); asym[3, 7] *= 1.0001
  a_d = torch.tensor(asym, device=device)
  x16, _ = K().matrix_inverse_pth_root_batched([a_d], [4], options={"products": "bf16x6"})
  x32, _ = K().matrix_inverse_pth_root_batched([a_d], [4], options={"accumulation": "chain"})
  assert torch.equal(x16[0], x32[0])


def test_diag_mfma_clock(device):
  ghz, tf = C.c_double(), C.c_double()
  rc = L().ps_diag_mfma_clock(torch.cuda.current_stream().cuda_stream, 200.0,
                              C.addressof(ghz), C.addressof(tf))
  assert rc == 0
  assert 1.0 < ghz.value < 2.6, ghz.value
  # an MFMA-only loop reaches most of the fp32 MFMA peak at the clock it runs at
  cus = torch.cuda.get_device_properties(device).multi_processor_count
  assert tf.value > 0.8 * cus * 4 * 64 * ghz.value / 1e3, (tf.value, ghz.value)


def test_diag_mfma_mix(device):
  """VALU work between fp32 MFMAs costs MFMA throughput (what the K-loop design rests on)."""
  st = torch.cuda.current_stream().cuda_stream
  tf = {}
  for nv in (0, 64):
    v = C.c_double()
    assert L().ps_diag_mfma_mix(st, nv, 0, 1, C.byref(v)) == 0
    tf[nv] = v.value
  assert tf[0] > 100.0 and tf[64] < 0.9 * tf[0], tf
  v = C.c_double()
  assert L().ps_diag_mfma_mix(st, 5, 0, 1, C.byref(v)) != 0   # unsupported mix


@pytest.mark.parametrize("n,k,p", [(300, 900, 4), (512, 2048, 2), (1000, 1100, 4), (96, 400, 4)])
def test_newton_root_of_symmetric_input_is_bitwise_symmetric(n, k, p, device):
  """Round 3: the iterates of an exactly symmetric block are bitwise symmetric (mirror store off
  the diagonal, (X + X^T)/2 inside the diagonal tiles of the M and H updates), which is what
  allows the product kernel to read the right operand transposed.  Observable at the boundary:
  the returned root equals its transpose bit for bit, and still matches the oracle (DS:702)."""
  a = wishart(n, k, 300 + n)
  a_d = torch.tensor(a, device=device)
  r, m = K().matrix_inverse_pth_root_batched([a_d], [p])
  h = r[0]
  assert torch.equal(h, h.t().contiguous())
  h_ref, m_ref = orc.matrix_inverse_pth_root(a, p)
  rel = np.linalg.norm(h.cpu().numpy() - h_ref) / np.linalg.norm(h_ref)
  assert rel < (5e-3 if n == 1000 else 1e-4), rel   # 1000 x 1100: cond ~1e6 (two f32 evaluations differ)
  assert abs(float(m[0, 1]) - m_ref["inverse_pth_root_iters"]) <= (1 if n == 1000 else 0)


def test_newton_product_kernel_variants_bit_identical_and_trace(device, monkeypatch, tmp_path):
  """The explicitly pipelined K loop (default), the compiler-scheduled one (PS_NEWTON_PIPE=0) and
  the traced kernel (PS_NEWTON_TRACE) compute the same bits; the trace holds one 64-byte record
  per tile with ordered time stamps."""
  arrs = [wishart(512, 2048, 80), wishart(384, 768, 81), wishart(130, 600, 82)]
  asym = wishart(256, 512, 83); asym[2, 9] *= 1.0001     # a block that is not exactly symmetric
  arrs.append(asym)
  mats = [torch.tensor(a, device=device) for a in arrs]
  ps = [4, 2, 4, 4]
  # (the developer variants exist for the two-register-set kernel: accumulation = "chain")
  chain = {"accumulation": "chain"}
  r1, m1 = K().matrix_inverse_pth_root_batched(mats, ps, options=chain)
  monkeypatch.setenv("PS_NEWTON_PIPE", "0")
  r0, m0 = K().matrix_inverse_pth_root_batched(mats, ps, options=chain)
  monkeypatch.delenv("PS_NEWTON_PIPE")
  path = tmp_path / "stage_trace.bin"
  monkeypatch.setenv("PS_NEWTON_TRACE", str(path))
  rt, mt = K().matrix_inverse_pth_root_batched(mats, ps, options=chain)
  monkeypatch.delenv("PS_NEWTON_TRACE")
  for i in range(len(mats)):
    assert torch.equal(r1[i], r0[i]) and torch.equal(r1[i], rt[i]), i
  assert torch.equal(m1, m0) and torch.equal(m1, mt)
  rec = np.fromfile(str(path), dtype=np.uint64).reshape(-1, 8)
  assert len(rec) > 0
  t0, t3 = rec[:, 3].astype(np.int64), rec[:, 6].astype(np.int64)
  assert np.all(t3 >= t0)
  ran = rec[:, 5] > 0                                   # tiles that executed a K loop
  assert ran.any()
  tf, tk = rec[ran, 4].astype(np.int64), rec[ran, 5].astype(np.int64)
  assert np.all(tf >= t0[ran]) and np.all(tk >= tf) and np.all(t3[ran] >= tk)


@pytest.mark.parametrize("m,k,n", [(300, 256, 96), (512, 1024, 64), (128, 32, 7)])
def test_bf16_gemm_tile_blocked_left_operand_bit_identical(m, k, n, device):
  """ps_convert_f32_to_bf16 mode 2 + ps_gemm_bf16_desc.a_tiled (the covariance layout of the FD
  branch, DS:1123-1290's products): the same product bit for bit as the row-major operand, with
  and without the lo parts, for row counts that are not a multiple of the tile."""
  g = torch.Generator(device=device).manual_seed(m + k + n)
  a = torch.randn((m, k), generator=g, device=device)
  b = torch.randn((n, k), generator=g, device=device)
  b16 = K().to_bf16(b, split=True)
  row = K().to_bf16(a, split=True)
  til = K().to_bf16(a, split=True, tiled=True)
  for split in (True, False):
    c0 = torch.empty((m, n), device=device); c1 = torch.full((m, n), float("nan"), device=device)
    bb = (b16[0], b16[1] if split else None)
    K().gemm_bf16_grouped([((row[0], row[1] if split else None), bb, c0)])
    t = K().TiledBf16(til.hi, til.lo if split else None, m, k)
    K().gemm_bf16_grouped([(t, bb, c1)])
    assert torch.equal(c0, c1), split
    ref = (a.double() @ b.double().t()).float()
    tol = 2e-4 if split else 3e-2
    assert float((c1 - ref).norm() / ref.norm()) < tol


# ---------------------------------------------------------------------------
def _two_rank_gpu_worker(rank, world, port, ret):
  import sys
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  if root not in sys.path:
    sys.path.insert(0, root)
  import torch.distributed as dist
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  dist.init_process_group("gloo", rank=rank, world_size=world)
  try:
    from precondition_amd import comm
    dev = torch.device("cuda:0")
    sizes = [256, 384, 256, 200, 512, 256, 384]          # odd count: a padding slot on 2 ranks
    exps = [4, 2, 4, 4, 2, 4, 2]
    stats = [torch.tensor(wishart(n, 4 * n, 900 + i), device=dev) for i, n in enumerate(sizes)]
    base, base_m = comm.sharded_inverse_pth_roots(stats, exps, group=None)
    out = {}
    for ownership in ("reference", "lpt"):
      for overlap in (False, True):
        roots, met = comm.sharded_inverse_pth_roots(
            stats, exps, group=dist.group.WORLD, ownership=ownership, overlap=overlap,
            overlap_min_bytes=0)
        torch.cuda.synchronize()
        # (column 6, the power-iteration step count, is 0 where a phase was handed its largest
        # eigenvalues by the hoisted power iteration)
        ok = (all(torch.equal(a, b) for a, b in zip(roots, base)) and
              torch.equal(met[:, :6], base_m[:, :6]))
        out[(ownership, overlap)] = bool(ok)
    ret[rank] = out
  finally:
    dist.destroy_process_group()


def test_two_ranks_share_one_gpu_hip_roots_gathered_over_gloo(device):
  """The N > 1 product path on GPU tensors with the HIP kernels: two processes (one GPU, so the
  process group is gloo and the gather is staged through the host -- RCCL refuses two ranks on
  one device) own disjoint statistics, root them with ps_newton_root_batched_f32 and gather: every
  rank ends with the single-process roots and metrics bit for bit, in list order, for both
  ownership modes and for the one- and two-phase (overlap) layouts."""
  import socket
  import torch.multiprocessing as mp
  s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
  ctx = mp.get_context("spawn")
  mgr = ctx.Manager()
  ret = mgr.dict()
  mp.spawn(_two_rank_gpu_worker, args=(2, port, ret), nprocs=2, join=True)
  for rank in range(2):
    assert all(ret[rank].values()), (rank, dict(ret[rank]))
