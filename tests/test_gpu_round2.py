"""Round-2 parity tests of the HIP path (through the C-ABI):

* inputs that are NOT symmetric (dequantized int16 statistics, DS:2746-2772) through
  the power iteration and the Newton root against the oracle's full products — the
  reference's functions take any square matrix (DS:595, DS:845-846);
* the persistent dataflow execution of the Newton root against the staged one
  (bit-identical: same tile code, same summation orders);
* BASELINE.json configs[3]: the ViT-B/16 parameter tree (395 statistics of sizes
  768 / 1024 / 1000 / 197, p = 2 and 4 in ONE batch) through
  comm.sharded_inverse_pth_roots with LPT ownership (DS:2816-2950).
"""
import os

import numpy as np
import pytest
import torch

from oracle import quantization_oracle as qorc
from oracle import shampoo_oracle as orc

pytestmark = pytest.mark.gpu


def K():
  from precondition_amd import kernels
  return kernels


def wishart(n, k, seed):
  g = np.random.default_rng(seed).standard_normal((n, k)).astype(np.float32)
  return (g @ g.T).astype(np.float32)


def dequantized_int16(a):
  """What the reference roots in the int16 state mode: to_float(quantize(A)) with the
  diagonal kept aside (DS:2746-2772).  Column scales make it asymmetric."""
  q, d, b = qorc.quantize(a, np.int16, True)
  return np.ascontiguousarray(qorc.to_float(q, d, b, np.int16, True), dtype=np.float32)


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,seed", [(96, 4, 1), (200, 2, 2), (384, 4, 3), (130, 4, 4)])
def test_asymmetric_input_power_iteration_and_newton_vs_oracle(n, p, seed, device):
  a = dequantized_int16(wishart(n, 4 * n, seed))
  assert np.abs(a - a.T).max() > 0, "the test input must not be symmetric"
  a_d = torch.tensor(a, device=device)
  # power iteration: full mat-vec (DS:631-639)
  _, lam_ref, _ = orc.power_iteration(a)
  lam, its = K().power_iteration_batched([a_d])
  assert np.isclose(float(lam[0]), float(lam_ref), rtol=2e-5), (float(lam[0]), float(lam_ref))
  # Newton root: full products (DS:845-846)
  h_ref, m_ref = orc.matrix_inverse_pth_root(a, p)
  roots, met = K().matrix_inverse_pth_root_batched([a_d], [p])
  met = met.cpu().numpy()
  h = roots[0].cpu().numpy()
  rel = np.linalg.norm(h - h_ref) / np.linalg.norm(h_ref)
  assert rel < 5e-5, rel
  assert met[0, 1] == m_ref["inverse_pth_root_iters"], (met[0], m_ref)
  assert met[0, 4] == m_ref["total_retries"]
  # 'general' = the same full products: bit-identical to what 'verify' decided
  roots_g, met_g = K().matrix_inverse_pth_root_batched([a_d], [p], symmetry="general")
  assert torch.equal(roots_g[0], roots[0]) and torch.equal(met_g, torch.tensor(met, device=device))
  # the symmetric fast path on this input would be a different (wrong) computation
  if n > 128:  # (a single 128x128 tile has nothing to mirror)
    roots_s, _ = K().matrix_inverse_pth_root_batched([a_d], [p], symmetry="assume")
    assert not torch.equal(roots_s[0], roots[0])


def test_symmetry_verify_equals_assume_on_symmetric_input_and_mixed_batch(device):
  """A batch mixing exactly symmetric and asymmetric blocks: each block takes its own
  path, and the symmetric ones are bit-identical to a call that assumes symmetry."""
  sym = [wishart(n, 4 * n, 10 + i) for i, n in enumerate((64, 257, 300))]
  asym = [dequantized_int16(wishart(n, 4 * n, 20 + i)) for i, n in enumerate((130, 256))]
  mats = [sym[0], asym[0], sym[1], asym[1], sym[2]]
  ps = [4, 4, 2, 4, 4]
  mats_d = [torch.tensor(m, device=device) for m in mats]
  roots, met = K().matrix_inverse_pth_root_batched(mats_d, ps)
  roots_a, met_a = K().matrix_inverse_pth_root_batched(
      [mats_d[0], mats_d[2], mats_d[4]], [4, 2, 4], symmetry="assume")
  for i, j in enumerate((0, 2, 4)):
    assert torch.equal(roots[j], roots_a[i])
    assert torch.equal(met[j], met_a[i])
  for j in (1, 3):
    h_ref, m_ref = orc.matrix_inverse_pth_root(mats[j], ps[j])
    h = roots[j].cpu().numpy()
    assert np.linalg.norm(h - h_ref) / np.linalg.norm(h_ref) < 5e-5
    assert float(met[j, 1]) == m_ref["inverse_pth_root_iters"]


# ---------------------------------------------------------------------------
def _mixed_batch():
  sizes = [16, 130, 64, 257, 96, 512, 33, 200, 1, 48, 640, 24]
  ps = [4, 2, 4, 4, 8, 4, 6, 2, 4, 3, 4, 4]
  mats = [wishart(n, 4 * n, 100 + i) for i, n in enumerate(sizes)]
  pads = list(sizes)
  mats[2] = orc.pad_square_matrix(mats[2], 80); pads[2] = 64
  mats[6] = orc.pad_square_matrix(mats[6], 40); pads[6] = 33
  # an all-padding block (DST:400-408) and an indefinite one that walks the retry ladder
  mats.append(np.eye(10, dtype=np.float32)); ps.append(4); pads.append(0)
  rng = np.random.default_rng(7)
  q, _ = np.linalg.qr(rng.standard_normal((24, 24)))
  e = np.linspace(1, 0.1, 24); e[-1] = -1e-3
  bad = (q * e) @ q.T
  mats[11] = ((bad + bad.T) / 2).astype(np.float32)
  return mats, ps, pads


def test_persistent_execution_bit_identical_to_staged(device):
  mats, ps, pads = _mixed_batch()
  mats_d = [torch.tensor(m, device=device) for m in mats]
  out = {}
  old = os.environ.get("PS_NEWTON_PERSISTENT")
  try:
    for mode in ("1", "0"):
      os.environ["PS_NEWTON_PERSISTENT"] = mode
      roots, met = K().matrix_inverse_pth_root_batched(mats_d, ps, pads)
      torch.cuda.synchronize()
      out[mode] = ([r.clone() for r in roots], met.clone())
  finally:
    if old is None:
      os.environ.pop("PS_NEWTON_PERSISTENT", None)
    else:
      os.environ["PS_NEWTON_PERSISTENT"] = old
  for i in range(len(mats)):
    assert torch.equal(out["1"][0][i], out["0"][0][i]), i
  # NaN-safe comparison of the metrics tables
  a, b = out["1"][1].cpu().numpy(), out["0"][1].cpu().numpy()
  assert np.array_equal(a, b, equal_nan=True), (a, b)
  assert a[11, 4] == 5.0  # the retry ladder ran inside the persistent kernel
  assert a[12, 0] == 0.0 and not out["1"][0][12].any()


@pytest.fixture
def persistent_mode():
  old = os.environ.get("PS_NEWTON_PERSISTENT")
  os.environ["PS_NEWTON_PERSISTENT"] = "1"
  yield
  if old is None:
    os.environ.pop("PS_NEWTON_PERSISTENT", None)
  else:
    os.environ["PS_NEWTON_PERSISTENT"] = old


def test_persistent_execution_repeated_calls_and_many_small_blocks(device, persistent_mode):
  """Queue state is re-initialised by every call; 600 small blocks of mixed exponents
  keep every queue busy with many more blocks than resident workgroups per queue."""
  rng = np.random.default_rng(5)
  sizes = rng.integers(1, 200, size=600)
  ps = rng.choice([1, 2, 3, 4, 6, 8], size=600)
  mats = [wishart(int(n), int(2 * n + 8), 1000 + i) for i, n in enumerate(sizes)]
  mats_d = [torch.tensor(m, device=device) for m in mats]
  r1, m1 = K().matrix_inverse_pth_root_batched(mats_d, [int(p) for p in ps])
  r2, m2 = K().matrix_inverse_pth_root_batched(mats_d, [int(p) for p in ps])
  assert torch.equal(m1, m2)
  for x, y in zip(r1, r2):
    assert torch.equal(x, y)
  m1 = m1.cpu().numpy()
  n_off = 0
  for i in rng.choice(600, size=24, replace=False):
    h_ref, m_ref = orc.matrix_inverse_pth_root(mats[i], int(ps[i]))
    h = r1[i].cpu().numpy()
    assert np.linalg.norm(h - h_ref) / np.linalg.norm(h_ref) < 5e-5, (i, sizes[i], ps[i])
    # iteration counts exact, +-1 where the 1e-6 threshold is within rounding
    d_it = abs(m1[i, 1] - m_ref["inverse_pth_root_iters"])
    assert d_it == 0 or (d_it == 1 and max(m1[i, 0], m_ref["inverse_pth_root_errors"]) < 3e-6), (
        i, m1[i], m_ref)
    n_off += int(d_it)
    assert m1[i, 4] == m_ref["total_retries"]
  assert n_off <= 2


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("persistent", ["0", "1"])
def test_vit_b_tree_recompute(device, persistent, monkeypatch):
  """BASELINE.json configs[3] on one rank: bench.py's VitBWorkload (the 200-leaf ViT-B/16
  tree, block_size 1024 -> 395 statistics, 4 warm statistics steps) through
  comm.sharded_inverse_pth_roots(ownership="lpt").  Every block: the root's own
  residual max|H^p (A + ridge I) - I| (float64 check of the float32 result), symmetry,
  finiteness; a 1000^2, a 197^2, a 768^2 / p = 2 and a 1024^2 / p = 4 block against the
  oracle with equal iteration and retry counts (reference: DS:2816-2950)."""
  import bench
  from precondition_amd import comm
  monkeypatch.setenv("PS_NEWTON_PERSISTENT", persistent)
  vw = bench.VitBWorkload(0, 1, device, None)
  assert vw.n_stats == 395
  vw.stats_step()
  flat = [s for st in vw.stats for s in st]
  roots, metrics = comm.sharded_inverse_pth_roots(flat, vw.exps, group=None, ownership="lpt",
                                                 pi_first=True)
  torch.cuda.synchronize()
  met = metrics.cpu().numpy()
  assert met.shape == (395, 8)
  census = {}
  for s, p in zip(flat, vw.exps):
    census[(int(s.shape[0]), p)] = census.get((int(s.shape[0]), p), 0) + 1
  assert census == {(768, 4): 172, (768, 2): 112, (1024, 4): 72, (1024, 2): 36,
                    (1000, 4): 1, (1000, 2): 1, (197, 4): 1}
  assert np.isfinite(met[:, 0]).all() and (met[:, 0] < 0.1).all(), "a block failed"
  worst = 0.0
  for i, (a, h, p) in enumerate(zip(flat, roots, vw.exps)):
    assert torch.isfinite(h).all()
    # off-diagonal tiles are mirrored exactly; inside the 128x128 diagonal tiles h_ij and
    # h_ji are separately rounded dot products
    assert (h - h.T).abs().max() <= 1e-4 * h.abs().max(), (i, float((h - h.T).abs().max()), float(h.abs().max()))
    ridge = 1e-6 * max(float(met[i, 3]), 1e-25) * 10.0 ** (met[i, 4] - 1)
    d = a.double() + ridge * torch.eye(a.shape[0], dtype=torch.float64, device=device)
    hp = torch.linalg.matrix_power(h.double(), p)
    res = (hp @ d - torch.eye(a.shape[0], dtype=torch.float64, device=device)).abs().max()
    worst = max(worst, float(res))
    # the metric the kernel reports is max|M - I| of its own iterate; the float64
    # residual of the float32 root adds the rounding of H^p D at this conditioning
    assert float(res) < 2e-2, (i, tuple(a.shape), p, float(res), met[i])
  sample = {}
  for i, (s, p) in enumerate(zip(flat, vw.exps)):
    sample.setdefault((int(s.shape[0]), p), i)
  for key in ((1000, 4), (197, 4), (768, 2), (1024, 4)):
    i = sample[key]
    a = flat[i].cpu().numpy()
    h_ref, m_ref = orc.matrix_inverse_pth_root(a, key[1])
    h = roots[i].cpu().numpy()
    rel = np.linalg.norm(h - h_ref) / np.linalg.norm(h_ref)
    # These statistics come from 5 steps on ONE gradient: rank 768 in up to 1024 dimensions
    # plus the 1e-6 initial diagonal, cond ~7e3 at p = 4.  North_star's bar: 1e-4 against the
    # oracle.  And, graded against the float64 closed form, the build may not be further from it
    # than the oracle's own float32 evaluation (NumPy/OpenBLAS): rounds 1-3 summed every product
    # as ONE fmaf chain over k and sat at 1.3-1.6 x the oracle's error; round 4 sums in segments
    # of 128 (gemm_core.hip.h SEG_K, ps_options.accumulation) and sits at 0.5-0.6 x.
    ridge = 1e-6 * max(float(met[i, 3]), 1e-25) * 10.0 ** (met[i, 4] - 1)
    w64, v64 = np.linalg.eigh(a.astype(np.float64))
    h64 = (v64 * (np.maximum(w64, 0) + ridge) ** (-1.0 / key[1])) @ v64.T
    e_build = np.linalg.norm(h - h64) / np.linalg.norm(h64)
    e_oracle = np.linalg.norm(h_ref - h64) / np.linalg.norm(h64)
    # (where the oracle itself is further than 1e-4 from float64 -- 1.2e-4 on the 1000^2 / 1024^2
    # p = 4 blocks -- no float32 implementation can be within 1e-4 of BOTH: the float64 root decides)
    if e_oracle <= 1e-4:
      assert rel <= 1e-4, (key, rel, e_build, e_oracle)
    assert e_build <= 1.0 * e_oracle, (key, rel, e_build, e_oracle)
    assert met[i, 1] == m_ref["inverse_pth_root_iters"], (key, met[i], m_ref)
    assert met[i, 4] == m_ref["total_retries"], (key, met[i], m_ref)
    assert np.isclose(met[i, 3], m_ref["max_eigen_value"], rtol=2e-5)


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d1024_r8", "d2048_r64"])
def test_fd_update_root_subspace_path_vs_reference_golden(name, device, monkeypatch):
  """Full-size Frequent-Directions chains (BASELINE configs[4] path): at d >= 1024
  _fd_update_root takes the leading rank+1 eigenpairs from the block subspace method
  (MFMA products) instead of the reference's SVD of [sqrt(decay) W | R] (DS:1193).  Every
  step is replayed from the REFERENCE's previous sketch and compared with its packed
  result as DST:770-885 do: inverted / deflated eigenvalues, tail and const by value,
  eigenvectors through the projector they span (tests/golden/low_rank_big.npz, generated by
  tools/gen_golden.py from the reference's own _fd_update_root)."""
  import json
  from precondition_amd import low_rank, subspace
  from tests.test_oracle_golden import GOLD, fd_big_grad
  from tests.test_optimizer_host_logic import packed_matches
  z = np.load(os.path.join(GOLD, "low_rank_big.npz"))
  with open(os.path.join(GOLD, "low_rank_big_index.json")) as f:
    c = [c for c in json.load(f) if c["name"] == name][0]
  calls = []
  real = subspace.top_eigenpairs_batched
  monkeypatch.setattr(subspace, "top_eigenpairs_batched",
                      lambda *a, **k: (calls.append(1), real(*a, **k))[1])
  # (round 6: the block method of a supported shape runs inside ONE library call, ps_fd_update_batched_f32)
  from precondition_amd import kernels as _kern
  real_one = _kern.fd_update_batched
  def _spy_one(*a, **k):
    res = real_one(*a, **k)
    if res is not None:
      calls.append(1)
    return res
  monkeypatch.setattr(_kern, "fd_update_batched", _spy_one)
  rng = np.random.default_rng(c["seed"])
  d, r = c["d"], c["rank"]
  prev = torch.zeros((d, r + 2), device=device)
  for t in range(c["steps"]):
    g = torch.tensor(fd_big_grad(d, r, t, rng), device=device)
    gram = low_rank.gram_of_block(g, 0)
    new, _ = low_rank._fd_update_root(
        gram, c["p"], rank=r, ridge_epsilon=c["ridge"], error_tolerance=0.0,
        relative_matrix_epsilon=c["rel"], decay=c["decay"], padding_start=d, prev=prev,
        new_grad_is_gram=True)
    ref = z[f"fd_{name}__new{t}"]
    got = new.cpu().numpy()
    assert packed_matches(got, ref, r, tol=2e-3), (name, t)
    # tail ~ cutoff^2 accumulates exactly as in the reference (DST:829-885)
    assert np.isclose(got[1, -1], ref[1, -1], rtol=1e-3)
    prev = torch.tensor(ref, device=device)
  assert len(calls) == c["steps"], "the block subspace method must have run"


# ---------------------------------------------------------------------------
def test_gemm_bf16_grouped_vs_fp64(device):
  """bf16-MFMA products of the FD branch: single bf16 operands (2^-9) and hi/lo pairs
  (2^-17) against float64, asymmetric operands, ragged n, several problems in one launch."""
  rng = np.random.default_rng(3)
  items, refs, tols = [], [], []
  for (m, n, k), split in (((256, 96, 512), True), ((128, 128, 64), False), ((384, 40, 1024), True),
                           ((200, 96, 256), False)):
    a = rng.standard_normal((m, k)).astype(np.float32)
    b = rng.standard_normal((k, n)).astype(np.float32)   # the tall-skinny iterate [k, n]
    a_d, b_d = torch.tensor(a, device=device), torch.tensor(b, device=device)
    c = torch.full((m, n), float("nan"), device=device)
    items.append((K().to_bf16(a_d, split=split), K().to_bf16(b_d, split=split, transpose=True), c))
    refs.append(a.astype(np.float64) @ b.astype(np.float64))
    tols.append(3e-5 if split else 8e-3)
  # the conversion itself: hi = RNE bf16, hi + lo reproduces x to 2^-17
  hi, lo = items[0][0]
  a0 = torch.tensor(rng.standard_normal((4, 4)).astype(np.float32), device=device)
  assert torch.equal(K().to_bf16(a0)[0], a0.to(torch.bfloat16))
  K().gemm_bf16_grouped(items)
  for (_, _, c), ref, tol in zip(items, refs, tols):
    got = c.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < tol, tol


# ---------------------------------------------------------------------------
def test_fd_diagnostics_vs_reference_golden(device):
  """FDDiagnostics (DS:197-335) of _fd_update_root in factor mode against the values the
  reference's own code produced (tests/golden/fd_metrics.npz), and the Gram-matrix mode of
  the optimizer: the same numbers where they are defined, NaN for the four quantities that
  depend on which factor R of the Gram matrix the caller holds."""
  import json
  from precondition_amd import low_rank
  from tests.test_oracle_golden import GOLD
  z = np.load(os.path.join(GOLD, "fd_metrics.npz"))
  with open(os.path.join(GOLD, "fd_metrics_index.json")) as f:
    idx = json.load(f)
  factor_only = {"new_grad_abs_max", "new_grad_sparsity", "new_grad_col_sparsity", "entrywise_err"}
  for c in idx:
    nm, r = c["name"], c["rank"]
    for t in range(c["steps"]):
      fac = torch.tensor(z[f"{nm}__factor{t}"], device=device)
      prev = torch.tensor(z[f"{nm}__prev{t}"], device=device)
      ref = dict(zip(c["fields"], z[f"{nm}__fd{t}"].tolist()))
      for use_gram in (False, True):
        src = low_rank.kernels.matmul(fac, fac, transb=True) if use_gram else fac
        new, tm = low_rank._fd_update_root(
            src, c["p"], rank=r, ridge_epsilon=1e-6, error_tolerance=0.0,
            relative_matrix_epsilon=True, decay=c["decay"], padding_start=c["padding_start"],
            prev=prev, generate_training_metrics=True, generate_fd_metrics=True,
            new_grad_is_gram=use_gram)
        got = {k: float(getattr(tm.fd, k)) for k in c["fields"]}
        for k, v in ref.items():
          if use_gram and k in factor_only:
            assert np.isnan(got[k]), (k, got[k])
          elif k == "max_ortho_err":
            assert got[k] < 1e-5
          elif k in ("square_frob", "heuristic_frob"):
            # trace(C) - sum of the kept s_i^2: a difference of large numbers in float32
            assert np.isclose(got[k], v, rtol=2e-3, atol=1e-4 * ref["total_frob"]), (k, got[k], v)
          else:
            assert np.isclose(got[k], v, rtol=2e-3, atol=1e-6), (nm, t, use_gram, k, got[k], v)


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shard_a_default_d1", "shard_a_rmsprop_wd_d1",
                                  "shard_a_int8_momentum_d1"])
def test_sharded_optimizer_state_api_hip_vs_reference_golden(name, device):
  """shard_optimizer_states (the reference's pjit-mode API, DS:2162-2583) on the HIP path
  against goldens generated from the reference's own sharded_init_fn / sharded_update_fn
  (tools/gen_golden.py gen_e2e_sharded): every update of every step, the final stacked padded
  statistics / preconditioners / exponents and the per-parameter local state."""
  from tests.test_optimizer_host_logic import (_sharded_index, check_sharded_final_state,
                                               run_sharded_case)
  gold = os.path.join(os.path.dirname(__file__), "golden")
  z = np.load(os.path.join(gold, "e2e_sharded.npz"))
  case = [c for c in _sharded_index(gold, 1) if c["name"] == name][0]
  st, worst = run_sharded_case(case, z, device, None)   # None => HIP kernels
  # In pjit mode the update of step t uses the roots of step t - 1 (DS:2443-2452), i.e. of
  # statistics with one sample fewer: with preconditioning from step 1 on (rmsprop case) the
  # first roots are of rank-1 + 1e-6 I matrices (cond ~1e7), where two float32 evaluations that
  # differ in the rounding order of the Gram update are 5e-3 apart (the oracle-backed CPU run of
  # the same logic, same NumPy arithmetic as the golden, is within 1e-3); int8 momentum adds
  # flipped codes (1/127 of a column maximum) that are carried into the next update.
  assert worst < 1e-2, worst
  check_sharded_final_state(case, z, st, tol_p=2e-2)


def test_stats_vector_blocks_stream_path(device):
  """Statistics of vector blocks (k = 1) take the streaming path of the grouped launch:
  fl(fl(w1*old) + fl(w2*fl(g_i*g_j))) bit for bit (what the MFMA path returns for one k),
  for aligned and unaligned statistics, ragged sizes, both operand layouts, in place."""
  from precondition_amd import kernels as K
  rng = np.random.default_rng(21)
  w1, w2 = np.float32(0.999), np.float32(0.001)
  items, wants = [], []
  for d, pad, as_column in ((768, 0, False), (260, 0, False), (131, 1, False), (1024, 0, True),
                            (129, 3, True), (5, 0, False)):
    gv = rng.standard_normal(d).astype(np.float32)
    if as_column:   # [d, 1] block, axis 0: element stride = leading dimension
      g, axis = torch.tensor(gv.reshape(d, 1), device=device), 0
    else:           # [d] block: contiguous elements
      g, axis = torch.tensor(gv, device=device), 0
    old = rng.standard_normal((d, d)).astype(np.float32)  # asymmetric on purpose
    buf = torch.zeros((d, d + pad), device=device)
    stat = buf[:, :d]
    stat.copy_(torch.tensor(old))
    items.append((g, axis, stat, stat))
    wants.append((w1 * old) + (w2 * np.outer(gv, gv).astype(np.float32)))
  K.stats_update_grouped(items, float(w1), float(w2))
  for (g, axis, stat, _), want in zip(items, wants):
    assert np.array_equal(stat.cpu().numpy(), want), tuple(g.shape)
  # the single-statistic entry point (MFMA path) agrees bit for bit
  d = 260
  gv = torch.tensor(rng.standard_normal(d).astype(np.float32), device=device)
  old = torch.tensor(rng.standard_normal((d, d)).astype(np.float32), device=device)
  one = K.gram_weighted_update(old, gv, 0, 0.9, 0.1)
  grp = old.clone()
  K.stats_update_grouped([(gv, 0, grp, grp)], 0.9, 0.1)
  assert torch.equal(one, grp)


def test_stats_interior_and_edge_tiles_agree(device):
  """Interior tiles of aligned statistics run the unguarded K loop and 16-byte epilogues, edge
  tiles / unaligned statistics the guarded ones: same products in the same order, so a block
  and the same block embedded in a ragged or unaligned problem agree bit for bit."""
  from precondition_amd import kernels as K
  rng = np.random.default_rng(22)
  for axis in (0, 1):
    d, k = 384, 256
    shape = (d, k) if axis == 0 else (k, d)
    g = torch.tensor(rng.standard_normal(shape).astype(np.float32), device=device)
    old = torch.tensor(rng.standard_normal((d, d)).astype(np.float32), device=device)
    fast = torch.empty_like(old)
    K.stats_update_grouped([(g, axis, old, fast)], 0.9, 0.1)
    # unaligned statistic (leading dimension d + 1): guarded path throughout
    buf_in = torch.zeros((d, d + 1), device=device); buf_in[:, :d] = old
    buf_out = torch.zeros((d, d + 1), device=device)
    K.stats_update_grouped([(g, axis, buf_in[:, :d], buf_out[:, :d])], 0.9, 0.1)
    assert torch.equal(buf_out[:, :d], fast)
    # gram part exactly symmetric, and the oracle within float32 accumulation noise
    gram = torch.empty_like(old)
    K.stats_update_grouped([(g, axis, torch.zeros_like(old), gram)], 0.0, 1.0)
    assert torch.equal(gram, gram.T)
    ref = orc.gram_weighted_update(old.cpu().numpy(), g.cpu().numpy(), axis, 0.9, 0.1)
    assert np.allclose(fast.cpu().numpy(), ref, rtol=1e-5, atol=1e-4)
    # a contraction length that is not a whole number of K-tiles: guarded K loop
    k2 = 250
    g2 = g[:, :k2] if axis == 0 else g[:k2, :]
    out2 = torch.empty_like(old)
    K.stats_update_grouped([(g2, axis, old, out2)], 0.9, 0.1)
    ref2 = orc.gram_weighted_update(old.cpu().numpy(), g2.cpu().numpy(), axis, 0.9, 0.1)
    assert np.allclose(out2.cpu().numpy(), ref2, rtol=1e-5, atol=1e-4)


def test_gemm_grouped_one_row_products_stream_path(device):
  """m = 1 products (preconditioner applied to a vector block, DS:1707 with a [d] gradient)
  take the matrix-vector path of the grouped launch; checked against float64 for aligned,
  ragged and unaligned operands, both storages of the row vector, next to ordinary tiles."""
  from precondition_amd import kernels as K
  rng = np.random.default_rng(23)
  items, refs = [], []
  for d, n, pad, col_vec in ((768, 768, 0, True), (1024, 1024, 0, False), (300, 517, 0, True),
                             (129, 131, 1, False), (64, 40, 3, True), (2000, 128, 0, False)):
    a = rng.standard_normal(d).astype(np.float32)
    b = rng.standard_normal((d, n)).astype(np.float32)
    bt = torch.zeros((d, n + pad), device=device)[:, :n]
    bt.copy_(torch.tensor(b))
    if col_vec:   # stored [d, 1], transa: op(a) = [1, d]
      at, ta = torch.tensor(a.reshape(d, 1), device=device), True
    else:         # stored [1, d]
      at, ta = torch.tensor(a.reshape(1, d), device=device), False
    c = torch.full((1, n), float("nan"), device=device)
    items.append((at, bt, c, ta, False))
    refs.append(a.astype(np.float64) @ b.astype(np.float64))
  # an ordinary product in the same launch group
  a2 = rng.standard_normal((256, 384)).astype(np.float32)
  b2 = rng.standard_normal((256, 200)).astype(np.float32)
  c2 = torch.empty((384, 200), device=device)
  items.append((torch.tensor(a2, device=device), torch.tensor(b2, device=device), c2, True, False))
  K.gemm_grouped(items)
  for (at, bt, c, _, _), ref in zip(items[:-1], refs):
    got = c.cpu().numpy()[0].astype(np.float64)
    scale = np.sqrt(at.numel())
    assert np.all(np.isfinite(got))
    assert np.max(np.abs(got - ref)) < 2e-5 * scale, (at.shape, bt.shape)
  ref2 = a2.astype(np.float64).T @ b2.astype(np.float64)
  assert np.max(np.abs(c2.cpu().numpy() - ref2)) < 2e-4


def test_update_tree_plan_bit_identical_to_per_block_path(device, monkeypatch):
  """The per-tree plan (descriptor tables from shapes, block pointers = gradient pointer +
  offset) issues the same kernels on the same operands as the per-block path: updates and
  state are bit-identical over several steps incl. a preconditioner recompute, on a tree with
  vector, matrix, blocked (ragged) and skipped parameters."""
  import precondition_amd as pa
  from precondition_amd.plan import TreePlan
  rng = np.random.default_rng(31)
  shapes = [(96,), (64, 48), (200, 72), (3, 4, 40), (130,), ()]
  params = [torch.tensor(rng.standard_normal(s).astype(np.float32), device=device) for s in shapes]

  def run(plan):
    if not plan:   # no tree plan: the optimizer takes the per-block path
      monkeypatch.setattr(TreePlan, "build", staticmethod(lambda *args: None))
    opt = pa.distributed_shampoo(0.1, 64, preconditioning_compute_steps=2,
                                 start_preconditioning_step=2,
                                 graft_type=pa.GraftingType.RMSPROP_NORMALIZED,
                                 skip_preconditioning_rank_lt=1)
    st = opt.init(params)
    g_rng = np.random.default_rng(5)
    ups = []
    for _ in range(5):
      grads = [torch.tensor(g_rng.standard_normal(s).astype(np.float32), device=device)
               for s in shapes]
      u, st = opt.update(grads, st, params)
      ups.append(u)
    return ups, st

  ups_a, st_a = run(True)
  ups_b, st_b = run(False)
  for ua, ub in zip(ups_a, ups_b):
    for x, y in zip(ua, ub):
      assert torch.equal(x, y)
  for sa, sb in zip(st_a.stats, st_b.stats):
    for x, y in zip(sa.statistics, sb.statistics):
      assert torch.equal(x, y)
    for x, y in zip(sa.preconditioners, sb.preconditioners):
      assert torch.equal(x, y)
    assert torch.equal(sa.momentum.to_float(), sb.momentum.to_float())


def test_power_iteration_resident_bit_identical_to_streaming(device, monkeypatch):
  """The resident execution of the power iteration (tiles in registers, team hand-off through
  tagged granules) and the streaming one (two launches per step) run the same arithmetic:
  lambda and step counts are bit-identical on mixed sizes (1 ... 1024, ragged, all-padding),
  early stops, repeated calls on a reused workspace, and on asymmetric inputs; both agree
  with the oracle."""
  from precondition_amd import kernels as K
  gen = torch.Generator(device=device).manual_seed(7)
  sizes = [1, 5, 127, 128, 129, 197, 300, 512, 768, 1000, 1024, 260, 64] * 2
  mats, pads = [], []
  for i, s in enumerate(sizes):
    g = torch.randn((s, 2 * s), generator=gen, device=device)
    a = (g @ g.T).contiguous()
    if i % 5 == 0:   # a dominant eigenvalue: the loop stops early (DS:639)
      a = a + 50.0 * s * torch.ones((s, s), device=device) / s
      a = 0.5 * (a + a.T)
    mats.append(a)
    pads.append(s if i != 3 else 0)   # one all-padding block
  asym = [m + 0.01 * torch.randn(m.shape, generator=gen, device=device) for m in mats]

  def run(resident):
    monkeypatch.setenv("PS_PI_RESIDENT", "1" if resident else "0")
    out = []
    for _ in range(2):   # second call: stale granules in the reused workspace must not match
      lam, its = K.power_iteration_batched(mats, padding_starts=pads)
      lam_a, its_a = K.power_iteration_batched(asym, padding_starts=pads)
      out.append((lam.cpu().numpy(), its.cpu().numpy(), lam_a.cpu().numpy(), its_a.cpu().numpy()))
    return out

  res, stream = run(True), run(False)
  for r, s_ in zip(res, stream):
    for x, y in zip(r, s_):
      assert np.array_equal(x, y, equal_nan=True)
  lam, its = res[0][0], res[0][1]
  assert np.isnan(lam[3]) and its[3] == 1
  assert its.min() < 100 and its.max() == 100
  for i in (1, 5, 9, 10):
    _, ref, _ = orc.power_iteration(mats[i].cpu().numpy(), 100, 1e-6)
    assert np.isclose(lam[i], ref, rtol=2e-5)


def test_fd_cfg5_full_size_vs_oracle(device):
  """BASELINE configs[4] at its full size: rank-64 Frequent-Directions updates of a 4096-dim
  factor (bf16x3 products by default), two chained updates, each compared with the oracle's
  fd_update_root (DS:1123-1290: LAPACK SVD of [sqrt(decay) W | R]) on the same inputs."""
  from precondition_amd import low_rank
  from tests.test_optimizer_host_logic import packed_matches
  d, r, p = 4096, 64, 4
  rng = np.random.default_rng(4096)
  prev = np.zeros((d, r + 2), np.float32)
  for t in range(2):
    g = rng.standard_normal((d, d)).astype(np.float32) * np.float32(1.0 + 0.3 * t)
    g[:r + 2] *= np.linspace(6.0, 2.0, r + 2)[:, None].astype(np.float32)
    ref = orc.fd_update_root(g, p, r, ridge_epsilon=1e-6, error_tolerance=0.0,
                             relative_matrix_epsilon=True, decay=0.999, padding_start=d,
                             prev=prev)
    gram = low_rank.gram_of_block(torch.tensor(g, device=device), 0)
    new, _ = low_rank._fd_update_root(
        gram, p, rank=r, ridge_epsilon=1e-6, error_tolerance=0.0, relative_matrix_epsilon=True,
        decay=0.999, padding_start=d, prev=torch.tensor(prev, device=device),
        new_grad_is_gram=True)
    got = new.cpu().numpy()
    assert packed_matches(got, ref, r, tol=2e-3), t
    assert np.isclose(got[1, -1], ref[1, -1], rtol=1e-3)
    prev = ref


def test_power_iteration_concurrent_streams(device):
  """Two host threads on two streams: at most one resident launch is in flight at a time (the
  other call takes the streaming execution), results stay bit-identical to a serial call."""
  import threading
  from precondition_amd import kernels as K
  gen = torch.Generator(device=device).manual_seed(11)
  mats = []
  for s in [512] * 24 + [300, 129, 64]:
    g = torch.randn((s, 2 * s), generator=gen, device=device)
    mats.append((g @ g.T).contiguous())
  ref_lam, ref_its = K.power_iteration_batched(mats)
  torch.cuda.synchronize()
  ref_lam, ref_its = ref_lam.cpu().numpy(), ref_its.cpu().numpy()
  out, errs = {}, []

  def worker(k):
    try:
      st = torch.cuda.Stream(device=device)
      with torch.cuda.stream(st):
        res = []
        for _ in range(6):
          lam, its = K.power_iteration_batched(mats)
          res.append((lam, its))
        st.synchronize()
      out[k] = [(l.cpu().numpy(), i.cpu().numpy()) for l, i in res]
    except Exception as e:  # pragma: no cover
      errs.append(e)

  ts = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
  for t in ts: t.start()
  for t in ts: t.join()
  assert not errs, errs
  for k in range(2):
    for lam, its in out[k]:
      assert np.array_equal(lam, ref_lam) and np.array_equal(its, ref_its)


@pytest.mark.parametrize("n,kind,p", [(169, "graded", 4), (512, "graded", 2), (260, "lowrank", 2),
                                      (1024, "graded", 4), (64, "graded", 2), (96, "graded", 4),
                                      (128, "lowrank", 4), (100, "lowrank", 2)])
def test_eigh_root_accuracy_on_graded_spectra_vs_true_float32_lapack(n, kind, p, device):
  """The eigh root (DS:943-1030) on spectra graded over six decades / rank-deficient + ridge, every error
  measured against the float64 closed form of the same float32 matrix (oracle.eigh_root_float64):

    default solver ("auto"): at or below the error of the reference's own arithmetic, a TRUE float32
      ssyevd (oracle lapack="f32"; rounds 1-5 compared with NumPy's float64-internal eigh by mistake).
      n > 128 keeps the tridiagonalisation path's result (no Jacobi sweep), n <= 128 is the LDS-resident
      Jacobi solver;
    "accurate": the Jacobi hand-over for ill-conditioned blocks -- near the float64-internal LAPACK
      result (the bar of rounds 2-5, unchanged), decades below ssyevd."""
  from precondition_amd import kernels as K
  rng = np.random.default_rng(n + p)
  if kind == "lowrank":
    g = rng.standard_normal((n, n // 4)); a = g @ g.T
  else:
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    a = (q * 10.0 ** rng.uniform(-4, 2, n)) @ q.T
  a = ((a + a.T) / 2).astype(np.float32)
  truth = orc.eigh_root_float64(a, p)
  tn = np.linalg.norm(truth)
  h32, m32 = orc.matrix_inverse_pth_root_eigh(a, p, lapack="f32")
  h64, _ = orc.matrix_inverse_pth_root_eigh(a, p, lapack="f64")
  e_ssyevd, e_yard = np.linalg.norm(h32 - truth) / tn, np.linalg.norm(h64 - truth) / tn
  assert e_ssyevd > 20 * e_yard                                   # these inputs tell the two apart
  t = torch.tensor(a, device=device)
  roots, met = K.matrix_inverse_pth_root_batched([t], [p], [n], eigh=True)
  e_auto = np.linalg.norm(roots[0].cpu().numpy().astype(np.float64) - truth) / tn
  assert e_auto < 1.25 * e_ssyevd + 2e-6, (e_auto, e_ssyevd)
  met = met.cpu().numpy()
  if n > 128:
    assert met[0, 5] == 0, "auto keeps the fast path's result: no Jacobi sweep"
  # the reference's error metric (DS:1017-1021) of the build's eigenpairs is of ssyevd's size
  assert met[0, 0] < 4 * m32["inverse_pth_root_errors"] + 1e-6 * float(np.abs(a).max()), (met[0, 0], m32)
  roots, met = K.matrix_inverse_pth_root_batched([t], [p], [n], eigh=True, options={"eigh_solver": "accurate"})
  e_acc = np.linalg.norm(roots[0].cpu().numpy().astype(np.float64) - truth) / tn
  # (rank-deficient + ridge: the null-space cluster sits at the kink of max(e, ridge)^(-1/p); the Jacobi
  # solvers are 5e-4 ... 1e-3 from the float64 root there, ssyevd 1e-2 ... 2e-2)
  assert (e_acc < 6 * e_yard + 2e-4 or e_acc < 0.1 * e_ssyevd) and e_acc < 2e-3, (e_acc, e_yard, e_ssyevd)
  assert e_acc < 0.5 * e_ssyevd
  if n > 128:
    assert met.cpu().numpy()[0, 5] > 0, "accurate: the ill-conditioned block was handed to the Jacobi solver"


def test_comm_entry_points_one_rank_rccl(device):
  """Seam (iii) at the C-ABI (DS:2876-2877): ps_comm_* resolve RCCL at run time; a one-rank
  communicator gathers a buffer into itself (N > 1 needs more GPUs than a test box has; the
  same calls with world > 1 are what a non-torch host issues)."""
  import ctypes as C
  from precondition_amd import _lib
  L = _lib.lib()
  uid = (C.c_char * 128)()
  rc = L.ps_comm_unique_id(uid)
  assert rc == 0, L.ps_comm_last_error()
  comm = C.c_void_p()
  with torch.cuda.device(device):
    rc = L.ps_comm_init(C.byref(comm), 0, 1, uid)
    assert rc == 0, L.ps_comm_last_error()
    send = torch.arange(4096, dtype=torch.float32, device=device)
    recv = torch.zeros_like(send)
    st = torch.cuda.current_stream().cuda_stream
    rc = L.ps_comm_allgather(st, comm, send.data_ptr(), recv.data_ptr(), send.numel() * 4)
    assert rc == 0, L.ps_comm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(send, recv)
    assert L.ps_comm_destroy(comm) == 0
  assert L.ps_comm_allgather(st, None, send.data_ptr(), recv.data_ptr(), 16) == -1
