#!/usr/bin/env python3
"""bench.py — preconditioner-recompute benchmark (BASELINE.json metric).

A "step" is one preconditioner recompute over one batch of synthetic
statistics blocks: power iteration + coupled-Newton inverse p-th root for every
block (libprecondition_amd.so), plus, for N > 1, the RCCL all-gather that leaves
every rank holding every root (the reference's DS:2876).  Inputs are resident
in HBM before the timed region.  Default workload = BASELINE.json configs[1]:
256 independent 512x512 blocks per GPU, p = 4 (weak scaling: each rank owns its
own 256 blocks).  The north_star's 64 x 1024^2 set is measured beside it and
reported under "headline_1024".

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times --steps steps and prints the
line (metric / value / unit / ms_per_step / dtype ...).  Everything else -- the un-hinted pass,
parity samples against the oracle, the in-library kernel profile and rooflines, the live clock
probe, the multi-GPU self-diagnosis, the headline_1024 / ViT-B / eigh / FD / quantized-state /
bf16x6 legs and the CPU baseline -- runs only with --full.  --dump-outputs DIR writes what the
timed path returned in its last step as .npy files (see dump_outputs).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak

# SELFTEST is False in every run of this file.  tests/bench_selftest_launcher.py (the gloo test of
# the N > 1 control flow) imports this module, replaces the numerical kernels of
# precondition_amd.kernels from the TEST side, shrinks WORKLOADS, sets this flag and calls main():
# rank set-up, the two-phase async all-gather step, barriers, max-over-ranks timing, the ViT-B
# strong-scaling leg and the JSON line then run on CPU tensors over gloo.  Nothing in this file
# can reach the oracle except cpu_baseline(); the line such a run prints says
# "data": "selftest-cpu".
SELFTEST = False


def _sync():
  if not SELFTEST:
    torch.cuda.synchronize()


WORKLOADS = {
    # name: (blocks per GPU, n, k of the Wishart factor, p, seed)
    "cfg2_256x512_p4": (256, 512, 2048, 4, 1234),
    "headline_64x1024_p4": (64, 1024, 4096, 4, 1024),
    "eigh_cfg3_64x2048_p2": (64, 2048, 4096, 2, 2048),
}


def c_of_p(p):
  """Algorithmic products per Newton step: c(2)=3, c(4)=4, ..."""
  return int(np.floor(np.log2(p))) + bin(p).count("1") - 1 + 2


def make_blocks(name, rank, dev):
  """A_b = G_b G_b^T, G_b ~ N(0,1) [n, k] from numpy default_rng(seed + rank)."""
  from precondition_amd import kernels as K
  nb, n, k, p, seed = WORKLOADS[name]
  rng = np.random.default_rng(seed + 1000003 * rank)
  stats = torch.zeros((nb, n, n), dtype=torch.float32, device=dev)
  chunk = 8 if n >= 2048 else 16
  for b0 in range(0, nb, chunk):
    g = rng.standard_normal((min(chunk, nb - b0), n, k), dtype=np.float32)
    g_d = torch.from_numpy(g).to(dev)
    items = [(g_d[i], 0, stats[b0 + i], stats[b0 + i]) for i in range(g_d.shape[0])]
    K.stats_update_grouped(items, 0.0, 1.0)  # S <- 0*S + 1*G G^T on the MFMA path
    _sync()
  return stats, p


class Workload:

  def __init__(self, name, rank, world, dev, multi=None):
    self.name = name
    self.world = world
    self.multi = (world > 1) if multi is None else multi
    self.stats, self.p = make_blocks(name, rank, dev)
    nb, n = self.stats.shape[0], self.stats.shape[1]
    self.nb, self.n = nb, n
    self.roots = torch.empty_like(self.stats)
    self.gathered = (torch.empty((world * nb, n, n), dtype=torch.float32, device=dev)
                     if self.multi else None)
    self.metrics = None
    self._ps = np.full(nb, self.p, np.int32)
    self._pads = np.full(nb, n, np.int32)
    self.hint = None       # host copy of the previous recompute's iteration counts
    self.options = {}      # per-call modes (ps_options), e.g. {"products": "bf16x6"}

  def refresh_hint(self):
    """What the optimizer does once per recompute (its failure select reads the metrics table on
    the host, DS:2936-2950): last recompute's inverse_pth_root_iters become the next call's
    ps_options.iters_hint.  Called outside the timed region (one sync + a [blocks] D2H copy)."""
    if self.metrics is not None and not self.name.startswith("eigh"):
      self.hint = self.metrics[:, 1].detach().cpu().numpy().astype(np.float32)

  def _roots(self, lo, hi, max_ev=None):
    from precondition_amd import kernels as K
    opts = dict(self.options)
    if self.hint is not None:
      opts["iters_hint"] = self.hint[lo:hi]
    # the reference's stacked form xs[b, n, n] (DS:2742): no per-block Python objects
    _, m = K.matrix_inverse_pth_root_batched(
        self.stats[lo:hi], self._ps[:hi - lo], padding_starts=self._pads[:hi - lo],
        out=self.roots[lo:hi], eigh=self.name.startswith("eigh"), max_ev=max_ev,
        options=opts or None)
    return m

  def split_point(self):
    """First-part size of the two-phase step.  Only the SECOND part's all-gather is exposed, so it should be small,
    but not below one full round of tiles on the 512 resident workgroup slots of a stage launch (T(T+1)/2 tiles per
    block), nor below a tenth of the batch.  Measured on cfg2 (tools/dev_r6_two_phase_cost.py, roots of both parts
    without the power iteration): 128 / 128 13.5 ms, 192 / 64 13.75, 204 / 52 13.6, 230 / 26 13.8 -- the position
    costs +-0.2 ms, the exposed share of a ~4.5 ms gather at world 8 far more."""
    t = (self.n + 127) // 128
    tpb = t * (t + 1) // 2
    second = max(-(-512 // tpb), self.nb // 10, 1)
    if second > self.nb // 2:
      second = self.nb // 2
    return max(1, self.nb - second)

  def compute(self):
    """This rank's roots only (no collective)."""
    self.metrics = self._roots(0, self.nb)

  def step(self):
    if not self.multi:
      self.compute()
      return
    # N > 1: the batch is rooted in two halves so that the RCCL all-gather of the
    # first half's roots (NCCL-side stream, async) runs under the second half's
    # Newton iterations (measured cost of the split on one GPU: +3 % at 512^2,
    # +4 % at 1024^2).  `gathered` is laid out [part][rank][block].
    # The power iteration (100 short HBM-bound launches) runs ONCE over the whole batch
    # and both halves take their largest eigenvalue from it: split halves of it would
    # sit on the launch-latency floor (split cost 1.4 -> 0.5 ms at 512^2; results are
    # bit-identical, same kernels).
    import torch.distributed as dist
    from precondition_amd import kernels as K
    h = self.split_point()
    per = self.n * self.n
    g = self.gathered.view(-1)
    handles = []
    ms = []
    lam = None
    if not self.name.startswith("eigh"):
      lam, _ = K.power_iteration_batched(list(self.stats.unbind(0)),
                                         padding_starts=[self.n] * self.nb)
    parts = ((0, h), (h, self.nb))

    def gather(lo, hi):
      off = self.world * lo * per   # parts are laid out one after the other: [part][rank][block]
      out = g[off: off + self.world * (hi - lo) * per]
      inp = self.roots[lo:hi].reshape(-1)
      if dist.get_backend() == "gloo":  # dev only (see main): stage through the host
        tmp = torch.empty(out.numel(), dtype=torch.float32)
        dist.all_gather_into_tensor(tmp, inp.cpu())
        out.copy_(tmp)
      else:
        handles.append(dist.all_gather_into_tensor(out, inp, async_op=True))

    side_by_side = (lam is not None and self.stats.is_cuda and dist.get_backend() != "gloo" and
                    not os.environ.get("PS_BENCH_SEQUENTIAL_PARTS"))
    if side_by_side:
      # The two parts as two root calls SIDE BY SIDE: part 2 from a second host thread on a second stream (the
      # library's calls release the GIL and keep their host state per thread), part 1 on a high-priority stream so that
      # it finishes first -- its kernels' tails and ramps are filled by part 2's, its all-gather runs under the rest of
      # part 2.  One after the other the two calls cost 2 ms more than one call of the whole batch (a second set of
      # setup / ramps / host work: tools/dev_r6_two_phase_cost.py).  Collectives stay on this thread, in a fixed order.
      # (ONE extra stream and ONE persistent side thread per process, shared with the optimizer's exchange: comm.py)
      from precondition_amd import comm
      s1, s2 = comm.high_priority_stream(self.stats.device), torch.cuda.current_stream()
      ready = torch.cuda.Event(); ready.record()          # behind the power iteration
      res, err = [None, None], []

      def run(k, stream):
        try:
          lo, hi = parts[k]
          with torch.cuda.stream(stream):
            stream.wait_event(ready)
            res[k] = self._roots(lo, hi, lam[lo:hi])
        except Exception as e:  # pylint: disable=broad-except
          err.append(e)

      t2 = comm.side_worker().submit(run, 1, s2)
      run(0, s1)
      with torch.cuda.stream(s1):
        gather(*parts[0])
      t2.result()
      if err:
        raise err[0]
      with torch.cuda.stream(s2):
        gather(*parts[1])
      s2.wait_stream(s1)
      ms = res
    else:
      for lo, hi in parts:
        ms.append(self._roots(lo, hi, None if lam is None else lam[lo:hi]))
        gather(lo, hi)
    for w in handles:
      w.wait()
    self.metrics = torch.cat(ms, dim=0)

  def check_gathered_order(self, rank):
    """After step(): `gathered` is laid out [half][rank][block]; this rank's own roots must
    sit in its rank's slots of both halves (DS:2876: all_gather returns rank order)."""
    if self.gathered is None:
      return True
    h = self.split_point()
    per = self.n * self.n
    g = self.gathered.view(-1)
    ok = True
    for k, (lo, hi) in enumerate(((0, h), (h, self.nb))):
      off = self.world * lo * per + rank * (hi - lo) * per
      ok &= bool(torch.equal(g[off: off + (hi - lo) * per], self.roots[lo:hi].reshape(-1)))
    return ok

  def flops(self):
    """Algorithmic FLOPs of the last step on this rank (c(p) * 2n^3 per
    Newton step)."""
    it = self.metrics[:, 5].double().sum().item()  # PS_M_TOTAL_ITERS
    return it * c_of_p(self.p) * 2.0 * float(self.n) ** 3

  def executed_flops(self):
    """FLOPs the MFMA pipe actually executes for them: the product kernels compute only
    the upper tile triangle of each symmetric product."""
    it = self.metrics[:, 5].double().mean().item()
    return self.flops() * executed_fraction(self.n, self.p, it, self.metrics[:, 7].double().mean().item())


# ---------------------------------------------------------------------------
# BASELINE.json configs[3]: ViT-B/16 parameter tree, block_size 1024, one full
# recompute step = statistics update of every block + 395 roots (+ all-gather).
# Strong scaling: the 395 statistics are partitioned over the ranks (LPT).
VIT_B_SHAPES = (
    [[16, 16, 3, 768], [768], [1, 1, 768], [1, 197, 768]] +
    12 * [[768], [768], [768, 12, 64], [12, 64], [768, 12, 64], [12, 64],
          [768, 12, 64], [12, 64], [12, 64, 768], [768], [768], [768],
          [768, 3072], [3072], [3072, 768], [768]] +
    [[768], [768], [768, 1000], [1000]])


class VitBWorkload:

  def __init__(self, rank, world, dev, group):
    from precondition_amd.blocking import Preconditioner
    self.group, self.world = group, world
    self.pcs, self.grads, self.stats, self.exps = [], [], [], []
    rng = np.random.default_rng(7)
    shapes, bs, merge = VIT_B_SHAPES, 1024, 4096
    if SELFTEST:  # same tree, every dimension / 32 (tests only)
      shapes = [[max(1, d // 32) if d > 16 else d for d in sh] for sh in VIT_B_SHAPES]
      bs, merge = 32, 128
    for shape in shapes:
      g = torch.from_numpy((rng.standard_normal(shape) * 0.02).astype(np.float32)).to(dev)
      pc = Preconditioner(g, bs, merge, True)
      st = [1e-6 * torch.eye(s[0], dtype=torch.float32, device=dev)
            for s in pc.shapes_for_preconditioners()]
      self.pcs.append(pc); self.grads.append(g); self.stats.append(st)
      self.exps.extend([pc.exponent_for_preconditioner()] * len(st))
    self.n_stats = sum(len(s) for s in self.stats)
    # owner-only statistics: a rank updates just the statistics it roots
    from precondition_amd import comm
    sizes = [int(s.shape[0]) for st in self.stats for s in st]
    owner = comm.ownership_table(sizes, self.exps, world, "lpt")
    self.mine = [o == rank for o in owner]
    self.metrics = None
    self.hint = None
    self.stats_flops = 0.0  # whole tree (all ranks together)
    for pc, g in zip(self.pcs, self.grads):
      for blk in pc.partitioned_blocks(g):
        for d in blk.shape:
          self.stats_flops += 2.0 * d * blk.numel()
    for _ in range(4):  # warm statistics (beta2 = 0.999)
      self.stats_step()

  def stats_executed_flops(self):
    """FLOPs the statistics kernel executes: tiles (i <= j) of each d x d Gram matrix."""
    f = 0.0
    for pc, g in zip(self.pcs, self.grads):
      for blk in pc.partitioned_blocks(g):
        for d in blk.shape:
          t = (d + 127) // 128
          f += 2.0 * d * blk.numel() * (t + 1) / (2.0 * t)
    return f

  def stats_step(self, subset=None):
    """subset: None = every statistic; "vector" = only the statistics of blocks whose contraction
    length is 1 (d x d outer products: the HBM-bound part of the launch); "matrix" = all others
    (the MFMA-bound part)."""
    from precondition_amd import kernels as K
    items = []
    for pc, g, st in zip(self.pcs, self.grads, self.stats):
      items.extend(pc.statistics_update_items(st, g, st))  # in place
    if self.world > 1:
      items = [it for it, m in zip(items, self.mine) if m]
    if subset is not None:
      kdim = lambda it: it[0].numel() // it[0].shape[it[1]]
      items = [it for it in items if (kdim(it) > 1) == (subset == "matrix")]
    K.stats_update_grouped(items, 0.999, 1.0 - 0.999)
    return items

  def step(self):
    from precondition_amd import comm
    self.stats_step()
    flat = [s for st in self.stats for s in st]
    # owner-only statistics: the ownership must not move between steps, so the hint steers the
    # per-block accuracy policy only (hint_in_ownership=False)
    _, self.metrics = comm.sharded_inverse_pth_roots(
        flat, self.exps, group=self.group, ownership="lpt", pi_first=True,
        iters_hint=self.hint, hint_in_ownership=False)

  def refresh_hint(self):
    if self.metrics is not None:
      self.hint = self.metrics[:, 1].detach().cpu().numpy().astype(np.float32).tolist()

  def flops(self, executed=False):
    m = self.metrics.cpu().numpy()
    flat = [s for st in self.stats for s in st]
    f = 0.0
    for i, s in enumerate(flat):
      n = int(s.shape[0])
      f += (m[i, 5] * c_of_p(self.exps[i]) * 2.0 * float(n) ** 3 *
            (executed_fraction(n, self.exps[i], m[i, 5], m[i, 7]) if executed else 1.0))
    return f  # roots of ALL ranks (metrics are gathered), statistics not included


def vit_b_rank_share(vw, dev, worlds=(2, 4, 8), reps=3):
  """Stand-in for the multi-GPU curve this builder cannot run (one GPU per lease): for a world of
  W ranks, the share of the ViT-B recompute that the MOST LOADED rank would execute -- the Gram
  updates of the statistics it owns + their roots, no gather -- timed on this one GPU, with the
  ownership the multi-rank run would use (LPT on comm.block_costs with last recompute's iteration
  counts).  `gather_ms_projected` prices the all-gather of DS:2876 at 7 xGMI links x 153 GB/s per
  GPU (direct algorithm: every rank receives (W - 1) / W of the roots); `projected_step_ms` is
  their sum (no overlap assumed), `projected_speedup` = the measured 1-rank step / that."""
  from precondition_amd import comm
  from precondition_amd import kernels as K
  flat = [s_ for st_ in vw.stats for s_ in st_]
  sizes = [int(s_.shape[0]) for s_ in flat]
  hint = vw.hint
  items_all = []
  for pc, g, st in zip(vw.pcs, vw.grads, vw.stats):
    items_all.extend(pc.statistics_update_items(st, g, st))
  cost = comm.block_costs(sizes, vw.exps, hint)
  out = {"ownership": "lpt on iterations x c(p) x tiles (comm.block_costs)", "worlds": {}}
  root_bytes = float(sum(4 * n * n for n in sizes))

  def run(idx):
    its = [items_all[i] for i in idx]
    mats = [flat[i] for i in idx]
    opts = {"iters_hint": np.asarray([hint[i] for i in idx], np.float32)} if hint is not None else None
    ms = []
    for _ in range(reps):
      _sync()
      t0 = time.perf_counter()
      K.stats_update_grouped(its, 0.999, 1.0 - 0.999)
      _, m = K.matrix_inverse_pth_root_batched(mats, [vw.exps[i] for i in idx],
                                               padding_starts=[sizes[i] for i in idx], options=opts)
      _sync()
      ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), m

  one_ms, _ = run(list(range(len(flat))))
  out["one_rank_ms"] = round(one_ms, 2)
  for w in worlds:
    owner = comm.ownership_table(sizes, vw.exps, w, "lpt", hint)
    load = [sum(c for c, o in zip(cost, owner) if o == r) for r in range(w)]
    crit = int(np.argmax(load))
    idx = [i for i, o in enumerate(owner) if o == crit]
    ms, m = run(idx)
    mm = m.cpu().numpy()
    fl = sum(mm[k, 5] * c_of_p(vw.exps[i]) * 2.0 * float(sizes[i]) ** 3 for k, i in enumerate(idx))
    fl_ex = sum(mm[k, 5] * c_of_p(vw.exps[i]) * 2.0 * float(sizes[i]) ** 3 *
                executed_fraction(sizes[i], vw.exps[i], mm[k, 5], mm[k, 7]) for k, i in enumerate(idx))
    # tiles of the largest product stage of this share on the 512 resident workgroup slots
    tiles = sum(((n + 127) // 128) * ((n + 127) // 128 + 1) // 2 for n in (sizes[i] for i in idx))
    gather_ms = root_bytes * (w - 1) / w / (7 * 153e9) * 1e3
    out["worlds"][str(w)] = {
        "statistics_of_critical_rank": len(idx), "load_imbalance_max_over_mean": round(max(load) / (sum(load) / w), 4),
        "share_ms": round(ms, 2), "roots_executed_frac_of_f32_mfma_peak": round(fl_ex / (ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4),
        "roots_algorithmic_tflops": round(fl / (ms * 1e-3) / 1e12, 1),
        "tile_rounds_per_stage_launch": round(tiles / 512.0, 2),
        "gather_ms_projected": round(gather_ms, 3),
        "projected_step_ms": round(ms + gather_ms, 2),
        "projected_speedup": round(one_ms / (ms + gather_ms), 2)}
  return out


def fd_cfg5(dev, factors=8, d=4096, rank=64, updates=3):
  """BASELINE.json configs[4]: Frequent-Directions sketch updates (rank 64) of
  4096-dim factors: Gram of a [4096, 4096] gradient block + _fd_update_root, three
  consecutive updates from a zero sketch.  Arithmetic of the large products (Gram, the
  Chebyshev filter's C @ Y): PS_FD_FILTER = bf16x3 (default: bf16 MFMA on hi/lo pairs),
  bf16 (plain bf16 operands first) or f32 (exact-f32 MFMA); Rayleigh-Ritz always float32."""
  from precondition_amd import low_rank, subspace
  if not SELFTEST:
    # what the optimizer's init_fn does for its compressed factors (kernel loading + allocator
    # pool: low_rank.prepare_fd); outside the timed updates, reported beside them
    _sync(); t_prep = time.perf_counter()
    low_rank.prepare_fd(d, rank, factors, dev)
    t_prep = time.perf_counter() - t_prep
  else:
    t_prep = 0.0
  gen = torch.Generator(device=dev).manual_seed(64)
  prevs = [torch.zeros((d, rank + 2), dtype=torch.float32, device=dev) for _ in range(factors)]
  times = []
  for u in range(updates):
    grads = [torch.randn((d, d), generator=gen, device=dev, dtype=torch.float32)
             for _ in range(factors)]
    _sync()
    t0 = time.perf_counter()
    calls = [dict(new_grad=low_rank.gram_of_block(grads[f], 0), p=4, rank=rank,
                  ridge_epsilon=1e-6, decay=0.999, padding_start=d, prev=prevs[f],
                  new_grad_is_gram=True) for f in range(factors)]
    prevs = [r[0] for r in low_rank._fd_update_root_batched(calls)]
    _sync()
    times.append((time.perf_counter() - t0) / factors)
    del grads
  tails = [float(p[1, -1]) for p in prevs]
  roof = None
  if subspace._filter_precision(d) != "f32" and not SELFTEST:
    # the dominant kernel: one step of the Chebyshev filter for all factors in ONE launch
    # (ps_fd_cy_step_f32: z = C y on bf16 hi/lo operands, the recurrence, the next bf16 operand).
    # HBM-bound: the covariance is read once as a hi/lo pair = 4 bytes per element, for b = 96
    # columns; y, y_prev, y_next (float32) and the iterate planes in and out are 20 bytes per
    # element of the [d, b] block
    from precondition_amd import kernels as K
    b = 96
    c16 = []
    for _ in range(factors):
      c = torch.randn((d, d), generator=gen, device=dev)
      c16.append(K.to_bf16(c, split=True, tiled="frag"))
      del c
    y = torch.randn((factors, d, b), generator=gen, device=dev)
    y_prev = torch.randn((factors, d, b), generator=gen, device=dev)
    z = torch.randn((factors, d, b), generator=gen, device=dev)
    y1, out = torch.empty_like(y), torch.empty_like(y)
    params = torch.tensor([[0.4, 0.5, 0.3, 12.0]] * factors, device=dev)
    yt = K.fd_filter_step(z, y, None, y1, params, 1, frag=True)
    nt = (torch.empty_like(yt[0]), torch.empty_like(yt[1]))
    for _ in range(3):
      K.fd_cy_step(c16, yt, y, y_prev, out, nt, params, 3)
    _sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
      K.fd_cy_step(c16, yt, y, y_prev, out, nt, params, 3)
    e1.record(); _sync()
    ms = e0.elapsed_time(e1) / 10
    nbytes = factors * (4.0 * d * d + 20.0 * d * b)
    roof = {"kernel": "fd_cy_step_kernel: one filter step (z = C y on hi/lo bf16 operands + recurrence "
                      "+ next operand) for all factors in one launch",
            "bound": "hbm", "peak": 8000, "unit": "GB/s",
            "achieved": round(nbytes / (ms * 1e-3) / 1e9, 1),
            "frac": round(nbytes / (ms * 1e-3) / 1e9 / 8000, 4),
            "ms_per_step_all_factors": round(ms, 4),
            "equiv_bf16x3_tflops": round(factors * 3 * 2.0 * d * d * b / (ms * 1e-3) / 1e12, 1)}
    del c16, y, y_prev, z, y1, out, yt, nt
  return {"workload": f"{factors} factors of dim {d}, rank {rank}, {updates} FD updates from a "
                      "zero sketch, grad blocks ~N(0,1) [4096x4096], fp32",
          "products": subspace._filter_precision(d),
          "ms_per_factor_update": [round(t * 1e3, 1) for t in times],
          "init_prepare_ms": round(t_prep * 1e3, 1),
          "tail_after_updates": round(float(np.mean(tails)), 1),
          "roofline": roof,
          "note": "Gram + leading rank+1 eigenpairs of the 4096x4096 covariance update by "
                  "Chebyshev-filtered subspace iteration (all factors batched): large products on "
                  "the bf16 MFMA (hi/lo split operands, fp32 accumulation) or the fp32 MFMA, "
                  "b x b problems in the LDS-resident eigensolver, fp32 Rayleigh-Ritz"}


def fd_parity_literal(dev, d=4096, rank=64, updates=2, p=4):
  """BASELINE configs[4] on its LITERAL input (grad blocks ~N(0,1), no spiked rows): the HIP
  Frequent-Directions update against oracle.fd_update_root (DS:1123-1290: LAPACK SVD of
  [sqrt(decay) W | R]) for `updates` chained updates of one factor, each chain on its own
  previous state.  The leading 64 singular values of a square Gaussian block sit in the edge
  cluster of the spectrum, so individual eigenvectors are not comparable; what the optimizer
  uses is: rho / tail, const = tail^(-1/p), the deflated and inverted eigenvalues, and the
  operator P = const (I - U U^T) + U diag(inverted) U^T (DS:1690-1705)."""
  from oracle import shampoo_oracle as orc
  from precondition_amd import low_rank
  gen = torch.Generator(device=dev).manual_seed(64)
  prev_g = torch.zeros((d, rank + 2), dtype=torch.float32, device=dev)
  prev_r = np.zeros((d, rank + 2), np.float32)
  rows = []
  for u in range(updates):
    g = torch.randn((d, d), generator=gen, device=dev, dtype=torch.float32)
    new, _ = low_rank._fd_update_root(
        low_rank.gram_of_block(g, 0), p, rank=rank, ridge_epsilon=1e-6, error_tolerance=0.0,
        relative_matrix_epsilon=True, decay=0.999, padding_start=d, prev=prev_g,
        new_grad_is_gram=True)
    _sync()
    ref = orc.fd_update_root(g.cpu().numpy(), p, rank, ridge_epsilon=1e-6, error_tolerance=0.0,
                             relative_matrix_epsilon=True, decay=0.999, padding_start=d, prev=prev_r)
    got = new.cpu().numpy().astype(np.float64)
    rf = ref.astype(np.float64)
    r = rank
    def op(pc):
      c = pc[0, -1]
      return c * np.eye(d) + (pc[:, :r] * (pc[:r, -2] - c)) @ pc[:, :r].T
    def low(pc):
      return (pc[:, :r] * pc[-r:, -1]) @ pc[:, :r].T
    pg, pr = op(got), op(rf)
    lg, lr = low(got), low(rf)
    rho = float(rf[1, -1])
    rows.append({
        "update": u + 1,
        "tail": float(got[1, -1]), "tail_ref": rho,
        "tail_rel": abs(float(got[1, -1]) - rho) / rho,
        "const_rel": abs(float(got[0, -1]) - float(rf[0, -1])) / float(rf[0, -1]),
        "deflated_max_abs_over_tail": float(np.abs(got[-r:, -1] - rf[-r:, -1]).max() / rho),
        "inverted_max_rel": float((np.abs(got[:r, -2] - rf[:r, -2]) / np.abs(rf[:r, -2])).max()),
        "operator_rel_fro": float(np.linalg.norm(pg - pr) / np.linalg.norm(pr)),
        "lowrank_part_rel_fro": float(np.linalg.norm(lg - lr) / max(np.linalg.norm(lr), 1e-300)),
        "has_zeros_equal": bool(got[-1, -2] == rf[-1, -2]),
    })
    prev_g, prev_r = new, ref
    del g, pg, pr, lg, lr
  return {"input": f"one factor of dim {d}, rank {rank}, grad blocks ~N(0,1) (the literal BASELINE input), "
                   f"{updates} chained updates, p={p}",
          "oracle": "oracle.fd_update_root (float32 LAPACK sgesdd of [sqrt(decay) W | R], scipy.linalg.lapack)",
          "updates": rows,
          "operator_rel_fro_max": max(x["operator_rel_fro"] for x in rows),
          "tail_rel_max": max(x["tail_rel"] for x in rows)}


def quant_f3(dev):
  """int16 quantize / dequantize of the ViT-B statistics (395 matrices,
  282.8 M elements, diagonal extracted) and int8 of its rank > 1 momentum buffers; HBM
  roofline (algorithmic bytes: 4 B read + 2 or 1 B written per element, and the reverse)."""
  from precondition_amd import kernels as K
  from precondition_amd.blocking import Preconditioner
  gen = torch.Generator(device=dev).manual_seed(3)
  stats, moms = [], []
  for shape in VIT_B_SHAPES:
    p = torch.empty(shape, device=dev)
    if len(shape) > 1:
      moms.append(torch.randn(shape, generator=gen, device=dev))
    for s in Preconditioner(p, 1024, 4096, True).shapes_for_preconditioners():
      g = torch.randn((s[0], 64), generator=gen, device=dev)
      stats.append(g @ g.T)

  def t(fn, reps=20):
    # sub-millisecond launches: keep the (untimed) warm-up going for 0.3 s, or the timed repetitions
    # run at ramping clocks (measured: every kernel of this leg then looks like 2.5 TB/s)
    out = fn(); _sync()
    t_warm = time.perf_counter()
    while not SELFTEST and time.perf_counter() - t_warm < 0.3:
      out = fn()
    _sync()
    t0 = time.perf_counter()
    for _ in range(reps):
      out = fn()
    _sync()
    return (time.perf_counter() - t0) / reps, out

  ne = sum(x.numel() for x in stats)
  nm = sum(x.numel() for x in moms)
  tq, tr = t(lambda: K.quantize_grouped(stats, torch.int16, True))
  td, _ = t(lambda: K.dequantize_grouped(tr))
  mq, mr = t(lambda: K.quantize_grouped(moms, torch.int8, False))
  md, _ = t(lambda: K.dequantize_grouped(mr))
  # the same calls into preallocated outputs (what the optimizer's recompute does: out= views of the
  # gather buffer): no 3 x 395 output views to create, the wall clock is the two kernel passes
  tq2, _ = t(lambda: K.quantize_grouped(stats, torch.int16, True, out=tr))
  fl = [torch.empty_like(x) for x in stats]
  td2, _ = t(lambda: K.dequantize_grouped(tr, out=fl))
  # descriptors resident (kernels.QuantizePlan: table + workspace built once; what a state updated
  # in place needs per step): one C-ABI call per launch
  plan = K.QuantizePlan(stats, torch.int16, True, tr)
  tq3, _ = t(lambda: plan.quantize())
  plan_f = K.QuantizePlan(fl, torch.int16, True, tr)
  td3, _ = t(lambda: plan_f.dequantize())
  mplan = K.QuantizePlan(moms, torch.int8, False, mr)
  mq3, _ = t(lambda: mplan.quantize())
  return {"workload": f"ViT-B state: {len(stats)} statistics ({ne / 1e6:.1f} M elements) as int16 + "
                      f"diagonal, {len(moms)} momentum buffers ({nm / 1e6:.1f} M elements) as int8; "
                      "wall clock of the grouped calls incl. host descriptor building",
          "bound": "hbm", "peak_GBps": 8000,
          "int16_quantize_ms": round(tq * 1e3, 3), "int16_quantize_GBps": round(ne * 6 / tq / 1e9, 1),
          "int16_dequantize_ms": round(td * 1e3, 3), "int16_dequantize_GBps": round(ne * 6 / td / 1e9, 1),
          "int16_quantize_preallocated_ms": round(tq2 * 1e3, 3),
          "int16_quantize_preallocated_GBps": round(ne * 6 / tq2 / 1e9, 1),
          "int16_dequantize_preallocated_ms": round(td2 * 1e3, 3),
          "int16_dequantize_preallocated_GBps": round(ne * 6 / td2 / 1e9, 1),
          "int16_quantize_plan_ms": round(tq3 * 1e3, 3),
          "int16_quantize_plan_GBps": round(ne * 6 / tq3 / 1e9, 1),
          "int16_quantize_plan_frac_of_hbm_peak": round(ne * 6 / tq3 / 8e12, 4),
          "int16_dequantize_plan_ms": round(td3 * 1e3, 3),
          "int16_dequantize_plan_GBps": round(ne * 6 / td3 / 1e9, 1),
          "int16_dequantize_plan_frac_of_hbm_peak": round(ne * 6 / td3 / 8e12, 4),
          "int8_quantize_plan_ms": round(mq3 * 1e3, 3), "int8_quantize_plan_GBps": round(nm * 5 / mq3 / 1e9, 1),
          "int8_quantize_ms": round(mq * 1e3, 3), "int8_quantize_GBps": round(nm * 5 / mq / 1e9, 1),
          "int8_dequantize_ms": round(md * 1e3, 3), "int8_dequantize_GBps": round(nm * 5 / md / 1e9, 1)}


DUMP_ROOTS_BUDGET = 48 << 20   # bytes of root blocks in a --dump-outputs directory (all files < 64 MB)


def dump_outputs(work, out_dir):
  """--dump-outputs: what the timed path returned in its last step, for output-for-output comparison
  of two builds on the same (seeded) inputs.
    roots.npy              float32 [k, n, n]: root blocks; all of them when they fit in DUMP_ROOTS_BUDGET,
                           else a fixed sample drawn with default_rng(0) (the same blocks in every run)
    roots_block_index.npy  float64 [k]: which blocks roots.npy holds (index into the list below)
    metrics.npy            float32 [blocks, 8]: the per-block metrics table of this rank (PS_M_*)
  The block list is this rank's roots at N = 1 and the gathered buffer (every rank's roots, laid out
  [part][rank][block]) at N > 1."""
  os.makedirs(out_dir, exist_ok=True)
  roots = work.gathered.view(-1, work.n, work.n) if work.gathered is not None else work.roots
  total = int(roots.shape[0])
  count = min(total, max(1, DUMP_ROOTS_BUDGET // (work.n * work.n * 4)))
  idx = np.arange(total)
  if count < total:
    idx = np.sort(np.random.default_rng(0).choice(total, size=count, replace=False))
  sample = roots[torch.from_numpy(idx).to(roots.device)]
  np.save(os.path.join(out_dir, "roots.npy"), sample.cpu().numpy().astype(np.float32))
  np.save(os.path.join(out_dir, "roots_block_index.npy"), idx.astype(np.float64))
  np.save(os.path.join(out_dir, "metrics.npy"), work.metrics.cpu().numpy().astype(np.float32))


def timed(work, steps, warmup, multi):
  import torch.distributed as dist
  t_warm = time.perf_counter()
  for _ in range(warmup):
    work.step()
    work.refresh_hint()
  # A timed region may follow seconds of host-only work (the oracle of a parity sample), after which
  # the GPU sits in a low power state and the first ~0.1 s of launches run at ramping clocks
  # (measured: 27 instead of 11 ms per step): keep the (untimed) warm-up going for 0.3 s.
  while (not SELFTEST and not multi and warmup > 0 and time.perf_counter() - t_warm < 0.3):
    work.step()
  _sync()
  if multi:
    dist.barrier()
  _sync()
  t0 = time.perf_counter()
  for _ in range(steps):
    work.step()
  _sync()
  if multi:
    dist.barrier()
  dt = time.perf_counter() - t0
  fl = work.flops()
  if multi:
    rdev = "cpu" if dist.get_backend() == "gloo" else "cuda"
    t = torch.tensor([dt], dtype=torch.float64, device=rdev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = t.item()
    f = torch.tensor([fl], dtype=torch.float64, device=rdev)
    dist.all_reduce(f, op=dist.ReduceOp.SUM)
    fl = f.item()
  return dt / steps, fl


def profile_stage_kernel(work):
  """One extra step with the library's HIP-event timing on (event pairs recorded inside the
  library on the launch stream): milliseconds and launch count of the product kernel
  (the persistent dataflow kernel: ONE launch per call), of the power iteration and of
  everything else the call enqueues."""
  from precondition_amd import _lib
  L = _lib.lib()
  # untimed calls first: the pass may follow seconds of host-only work (the oracle of the parity
  # sample), after which the GPU is in a low power state and the first launches run at ramping
  # clocks (one run read 0.485 ms per launch where the timed loop and rocprofv3 say 0.44)
  t_end = time.perf_counter() + 0.3
  while time.perf_counter() < t_end:
    work.compute()
    _sync()
  reps = 3
  L.ps_profile_reset()
  L.ps_profile_enable(1)
  try:
    for _ in range(reps):   # rank-local: no collective, so only rank 0 needs to run it
      work.compute()
    _sync()
  finally:
    L.ps_profile_enable(0)
  stage_ms, pi_ms, other_ms = C.c_double(), C.c_double(), C.c_double()
  launches = C.c_int64()
  L.ps_profile_get(C.addressof(stage_ms), C.addressof(launches), C.addressof(pi_ms),
                   C.addressof(other_ms))
  return stage_ms.value / reps, launches.value // reps, pi_ms.value / reps, other_ms.value / reps


def _pmc_traffic_bytes(kernel_substr, fname="r06_cfg2_pmc_by_kernel.json"):
  """HBM bytes per launch of the named kernel from the committed rocprofv3 --pmc summary (None if absent)."""
  path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", fname)
  try:
    with open(path) as f:
      table = json.load(f)
    for name, row in table.items():
      if kernel_substr in name and "hbm_MB_per_launch_corrected" in row:
        return round(float(row["hbm_MB_per_launch_corrected"]) * 1e6)
  except (OSError, ValueError):
    pass
  return None


def executed_fraction(n, p=4, iters=8.0, avg_steps=None):
  """Share of the algorithmic c(p) * 2n^3 flops per Newton step that the product kernel
  issues on the MFMA pipe.  Symmetric mode (the default): every product runs only the
  tiles with tm <= tn of its T x T tile grid ((T+1)/(2T) of the work) except the M update
  of the first `ps_newton_averaged_steps()` steps, which is computed in full (and averaged
  with its transpose, csrc/newton.hip TileFlags).  The H update of step 0 (H0 = h0 I times
  Mi) is not a product at all: newton_init2_tile writes fl(h0 * mi).  `iters` = Newton
  steps per block (one try assumed)."""
  it = max(float(iters), 1.0)
  c = c_of_p(p)
  if os.environ.get("PS_NEWTON_SYMMETRIC", "1") == "0":
    return (c * it - 1.0) / (c * it)
  from precondition_amd import _lib
  # steps whose M update ran in full: column PS_M_AVG_STEPS of the metrics table when the caller
  # has it (the rule is data dependent: newton_avg_next), else the cap
  navg = float(avg_steps) if avg_steps is not None else float(_lib.lib().ps_newton_averaged_steps())
  navg = min(navg, float(iters))
  t = (n + 127) // 128
  half = (t + 1) / (2.0 * t)
  per_step = (c - 1) * half + (navg / it) * 1.0 + (1 - navg / it) * half
  return (per_step * it - half) / (c * it)


def live_clock(warm_ms=1500.0):
  """Shader clock held under fp32-MFMA load and the fp32 MFMA rate of that loop, measured in
  THIS run by the library's diagnostic kernel (ps_diag_mfma_clock: delta s_memtime / delta
  s_memrealtime around an MFMA loop on non-trivial operands, after `warm_ms` of back-to-back
  launches).  The 157.3 TFLOP/s peak assumes 2.4 GHz; `peak_at_clock` = 256 CUs x 4 SIMDs x 64
  flop/clk x the measured clock is what this box can deliver to any fp32-MFMA kernel."""
  from precondition_amd import _lib
  ghz, tf = C.c_double(), C.c_double()
  rc = _lib.lib().ps_diag_mfma_clock(torch.cuda.current_stream().cuda_stream, float(warm_ms),
                                     C.addressof(ghz), C.addressof(tf))
  if rc != 0:
    return {"error": f"ps_diag_mfma_clock rc={rc}"}
  cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
  return {"clock_GHz_under_mfma_load": round(ghz.value, 3),
          "mfma_f32_loop_tflops": round(tf.value, 1),
          "peak_at_clock_tflops": round(cus * 4 * 64 * ghz.value * 1e9 / 1e12, 1),
          "nominal_peak_tflops": PEAK_F32_MFMA_TFLOPS,
          "source": "live: ps_diag_mfma_clock (csrc/diag.hip), %d ms warm-up" % int(warm_ms)}


def _rel_fro(got, ref):
  return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def parity_sample(work, count=8):
  """rel-Fro error of the GPU roots against the oracle (the checker, SURVEY 8d
  'Accuracy') on the first `count` blocks of the workload, same inputs; also iteration
  counts.  north_star bar: 1e-4."""
  from oracle import shampoo_oracle as orc
  errs, iters_equal = [], True
  m = work.metrics.cpu().numpy()
  for i in range(min(count, work.nb)):
    a = work.stats[i].cpu().numpy()
    h, mm = orc.matrix_inverse_pth_root(a, work.p, padding_start=work.n)
    got = work.roots[i].cpu().numpy()
    errs.append(_rel_fro(got, h))
    iters_equal &= bool(m[i, 1] == mm["inverse_pth_root_iters"] and m[i, 4] == mm["total_retries"])
  return {"blocks": len(errs), "rel_fro_max": max(errs), "rel_fro_median": float(np.median(errs)),
          "iteration_and_retry_counts_equal": iters_equal, "bar": 1e-4}


def parity_sample_eigh(work, count=2):
  """The eigh leg against the oracle's eigh root (DS:943-1030 restated over TRUE float32 LAPACK, ssyevd:
  what the reference's JAX CPU path runs) on the first `count` blocks; eigenvectors are not unique, so the
  comparison is on the root.  Beside it: both roots' distance from the float64 closed form of the same
  float32 matrix, and the reference's error metric (DS:1017-1021) of the build next to ssyevd's."""
  from oracle import shampoo_oracle as orc
  errs, e_build, e_ref, metric_ratio = [], [], [], []
  met = work.metrics.cpu().numpy() if getattr(work, "metrics", None) is not None else None
  for i in range(min(count, work.nb)):
    a = work.stats[i].cpu().numpy()
    h, m = orc.matrix_inverse_pth_root_eigh(a, work.p, padding_start=work.n)
    got = work.roots[i].cpu().numpy()
    errs.append(_rel_fro(got, h))
    truth = orc.eigh_root_float64(a, work.p, padding_start=work.n)
    e_build.append(_rel_fro(got, truth))
    e_ref.append(_rel_fro(h, truth))
    if met is not None and m["inverse_pth_root_errors"] > 0:
      metric_ratio.append(float(met[i, 0] / m["inverse_pth_root_errors"]))
  out = {"blocks": len(errs), "rel_fro_max": max(errs), "rel_fro_median": float(np.median(errs)),
         "bar": 1e-4, "oracle": "oracle.matrix_inverse_pth_root_eigh (scipy.linalg.lapack.ssyevd, float32)",
         "root_error_vs_float64_build_max": max(e_build), "root_error_vs_float64_ssyevd_max": max(e_ref)}
  if metric_ratio:
    out["error_metric_over_ssyevds_max"] = max(metric_ratio)
  return out


def parity_sample_vit_b(vw, roots, metrics, per_class=1):
  """ViT-B tree: one block per (size, exponent) class against the oracle, plus -- because the
  oracle's own float32 evaluation is 1.2e-4 from the float64 root on the cond ~7e3, p = 4
  blocks of this tree -- both errors against the float64 closed form."""
  from oracle import shampoo_oracle as orc
  flat = [s for st in vw.stats for s in st]
  m = metrics.cpu().numpy()
  seen, rows, iters_equal = {}, [], True
  for i, (s, p) in enumerate(zip(flat, vw.exps)):
    key = (int(s.shape[0]), int(p))
    if seen.get(key, 0) >= per_class:
      continue
    seen[key] = seen.get(key, 0) + 1
    a = s.cpu().numpy()
    h_ref, mm = orc.matrix_inverse_pth_root(a, p)
    got = roots[i].cpu().numpy()
    ridge = 1e-6 * max(float(m[i, 3]), 1e-25) * 10.0 ** (m[i, 4] - 1)
    w, v = np.linalg.eigh(a.astype(np.float64))
    h64 = (v * (np.maximum(w, 0) + ridge) ** (-1.0 / p)) @ v.T
    eq = bool(m[i, 1] == mm["inverse_pth_root_iters"] and m[i, 4] == mm["total_retries"])
    iters_equal &= eq
    row = {"n": key[0], "p": key[1], "iters": float(m[i, 1]),
           "rel_fro_vs_oracle": _rel_fro(got, h_ref),
           "build_vs_f64": _rel_fro(got, h64), "oracle_vs_f64": _rel_fro(h_ref, h64)}
    # the criterion, per class: where the oracle's own float32 evaluation is within the bar of the
    # float64 root, the build must be within the bar of the ORACLE; where it is not (two float32
    # evaluations of an ill-conditioned root differ by more than the bar), the build must be at
    # least as close to float64 as the oracle is
    row["passes"] = bool(row["rel_fro_vs_oracle"] <= 1e-4 if row["oracle_vs_f64"] <= 1e-4
                         else row["build_vs_f64"] <= row["oracle_vs_f64"])
    rows.append(row)
  return {"classes": rows, "passes": all(r["passes"] for r in rows),
          "criterion": "per class: rel_fro_vs_oracle <= 1e-4 where oracle_vs_f64 <= 1e-4, "
                       "else build_vs_f64 <= oracle_vs_f64",
          "rel_fro_max": max(r["rel_fro_vs_oracle"] for r in rows),
          "rel_fro_median": float(np.median([r["rel_fro_vs_oracle"] for r in rows])),
          "max_build_over_oracle_error_vs_f64": max(r["build_vs_f64"] / r["oracle_vs_f64"] for r in rows),
          "iteration_and_retry_counts_equal": iters_equal, "bar": 1e-4,
          "note": "north_star's 1e-4 is met vs the oracle wherever the oracle itself is within "
                  "1e-4 of float64; on the cond ~7e3 p=4 blocks two float32 evaluations differ by "
                  "more (tests/test_gpu_round2.py::test_vit_b_tree_recompute: build <= 1.5 x oracle)"}


def newton_bf16x6_leg(dev, clock):
  """Opt-in product arithmetic of the Newton root, reported separately (never in `value`):
  PS_NEWTON_PRODUCTS=bf16x6 = three-way bf16 split of both operands, six partial products per
  product on v_mfma_f32_32x32x16_bf16 with float32 accumulation (~2^-22 relative), exact float32
  products for the last steps of a block (max|M - I| < 1e-3).  Same workloads, same timing."""
  out = {"mode": "ps_options.products = bf16x6 / bf16x3 (what the factory's precision=HIGH / DEFAULT "
                 "select; csrc/newton.hip gemm_tile_bf16x_sym); the default exact-float32 numbers "
                 "are the top-level ones"}
  for name in ("cfg2_256x512_p4", "headline_64x1024_p4"):
    w = Workload(name, 0, 1, dev)
    row = {}
    for mode in ("f32", "bf16x6", "bf16x3"):   # one process, three modes: they are arguments
      w.options = {"products": mode}
      sec, fl = timed(w, 3, 1, False)
      row[mode] = {"ms_per_step": round(sec * 1e3, 3),
                   "algorithmic_gflops": round(fl / sec / 1e9, 1),
                   "newton_iters": {"min": float(w.metrics[:, 1].min()), "max": float(w.metrics[:, 1].max())}}
      if mode != "f32":
        row[mode]["parity_vs_oracle"] = parity_sample(w, count=4)
    out[name] = {"ms_per_step": row["bf16x6"]["ms_per_step"],
                 "ms_per_step_f32_products": row["f32"]["ms_per_step"],
                 "ms_per_step_bf16x3": row["bf16x3"]["ms_per_step"], "by_mode": row}
    del w
    torch.cuda.empty_cache()
  return out


def cpu_baseline(name, budget_s=12.0):
  """The oracle executing the reference's op sequence (its 6 products per step
  at p=4) on the host cores, on a bounded sample of the same workload."""
  from oracle import shampoo_oracle as orc
  nb, n, k, p, seed = WORKLOADS[name]
  rng = np.random.default_rng(seed)
  threads = None
  try:
    from threadpoolctl import threadpool_info
    info = [i for i in threadpool_info() if i.get("user_api") == "blas"]
    if info:
      threads = int(info[0]["num_threads"])
  except Exception:  # pylint: disable=broad-except
    pass
  done, flops, t_total = 0, 0.0, 0.0
  while done < nb and (t_total < budget_s or done < 2):
    g = rng.standard_normal((n, k), dtype=np.float32)
    a = g @ g.T
    t0 = time.perf_counter()
    _, m = orc.newton_root_reference_opcount(a, p, padding_start=n)
    t_total += time.perf_counter() - t0
    flops += m["inverse_pth_root_iters"] * c_of_p(p) * 2.0 * float(n) ** 3
    done += 1
  return dict(value=round(flops / t_total / 1e9, 2), unit="GFLOP/s",
              cores=threads or (os.cpu_count() or 1), kind="port",
              sample=f"first {done} of {nb} blocks of {name} (numpy/OpenBLAS float32, "
                     f"reference op sequence incl. its redundant products), "
                     f"{t_total:.1f} s, {t_total / done * 1e3:.1f} ms/block",
              host_cpus=os.cpu_count())


def _spawn_ranks(n):
  """`python bench.py --gpus N` without a launcher: run `python -m torch.distributed.run
  --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 <this script> <same arguments>` as a
  CHILD process (never exec: see the pool's rule about replacing a process), pass its output
  through and return its exit status.  Nothing here initialises the GPU: device_count() only
  counts."""
  import socket
  import subprocess
  if not SELFTEST and not os.environ.get("PS_BENCH_ONE_DEVICE"):
    have = torch.cuda.device_count()
    if n > have:
      print(f"bench.py: --gpus {n} but this node has {have} GPU(s): refusing to print a line for "
            "ranks that cannot run", file=sys.stderr)
      return 2
  with socket.socket() as s:
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
  env = dict(os.environ)
  env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
  env.setdefault("OMP_NUM_THREADS", "8")
  cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
         "--master-addr", "127.0.0.1", "--master-port", str(port),
         os.path.abspath(sys.argv[0])] + sys.argv[1:]
  return subprocess.run(cmd, env=env, check=False).returncode


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--gpus", type=int, default=1)
  ap.add_argument("--steps", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--workload", default="cfg2_256x512_p4", choices=sorted(WORKLOADS))
  ap.add_argument("--no-headline", action="store_true")
  ap.add_argument("--profile-hinted-only", action="store_true",
                  help="profiling mode (rocprofv3 around it): the iteration-count hint of the workload is "
                       "set BEFORE the first call (8 steps per block for the Wishart workloads, asserted "
                       "afterwards) and the un-hinted pass, parity samples, side legs and the CPU baseline "
                       "are skipped, so that every product launch of the trace is a hinted one and the "
                       "kernel-stats csv reproduces roofline.avg_launch_ms")
  ap.add_argument("--no-cpu-baseline", action="store_true")
  ap.add_argument("--no-extras", action="store_true",
                  help="skip the ViT-B (cfg4) and eigh (cfg3) side measurements")
  ap.add_argument("--full", action="store_true",
                  help="after the timed steps, also run everything beyond the headline figure: the un-hinted pass, "
                       "parity samples, kernel profile / rooflines / clock probe, the multi-GPU self-diagnosis, "
                       "the side legs and the CPU baseline (--no-headline / --no-extras / --no-cpu-baseline trim it)")
  ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                  help="write what the timed path returned in its last step to DIR/*.npy (dump_outputs); "
                       "bench_outputs/ is ignored by git")
  args = ap.parse_args()

  if args.gpus < 1:
    raise SystemExit("--gpus must be >= 1")
  if args.steps < 1 or args.warmup < 0:
    raise SystemExit("--steps must be >= 1 and --warmup >= 0")
  if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
    # launched plainly (`python bench.py --gpus N`): start the N ranks ourselves, one process per
    # GPU, BEFORE anything in this process touches the GPU, relay rank 0's line and exit with the
    # launcher's status (DS:2836, 2869-2879: the exchange step only exists with N > 1 ranks)
    raise SystemExit(_spawn_ranks(args.gpus))
  world = int(os.environ.get("WORLD_SIZE", "1"))
  # dev only: PS_BENCH_FORCE_DIST=1 under `torch.distributed.run --nproc-per-node 1` takes the
  # N > 1 code path (RCCL init, async all-gathers, barriers) with a one-rank group
  multi = world > 1 or bool(os.environ.get("PS_BENCH_FORCE_DIST"))
  rank = int(os.environ.get("RANK", "0"))
  local = int(os.environ.get("LOCAL_RANK", "0"))
  if os.environ.get("PS_BENCH_ONE_DEVICE"):  # dev only: several ranks on one GPU
    local = 0
  if world != args.gpus:
    raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: the line would report a "
                     "rank count that did not run (launch with matching --nproc-per-node, or "
                     "plainly and let bench.py start the ranks)")
  if SELFTEST:
    dev = torch.device("cpu")
  else:
    if not torch.cuda.is_available():
      raise SystemExit("bench.py needs an MI355X (no CPU path)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
  if multi:
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if SELFTEST or os.environ.get("PS_BENCH_ONE_DEVICE"):
      # tests / dev only: RCCL refuses two ranks on one GPU; gloo exercises the same control flow
      dist.init_process_group(backend="gloo")
    else:
      # RCCL (ROCm 7) prints a five-line version banner to STDOUT when the communicator is created; the line
      # contract of this script is ONE JSON line on rank 0's stdout, so file descriptor 1 points at stderr while
      # the group is created and warmed up (one barrier: the communicator is built lazily at the latest there)
      sys.stdout.flush()
      saved = os.dup(1)
      os.dup2(2, 1)
      try:
        dist.init_process_group(backend="nccl", device_id=dev)
        dist.barrier()
        torch.cuda.synchronize()
      finally:
        sys.stdout.flush()
        os.dup2(saved, 1)
        os.close(saved)

  work = Workload(args.workload, rank, world, dev, multi)
  if args.profile_hinted_only:
    args.no_headline = args.no_extras = args.no_cpu_baseline = True
    if not args.workload.startswith("eigh"):
      work.hint = np.full(work.nb, 8.0, np.float32)   # what a previous recompute reports (asserted below)
  sec, flops = timed(work, args.steps, args.warmup, multi)
  if args.profile_hinted_only and not args.workload.startswith("eigh"):
    assert bool((work.metrics[:, 1] == 8).all()), "the preset hint is not this workload's iteration count"
  if args.dump_outputs and rank == 0:
    dump_outputs(work, args.dump_outputs)
  # The same step WITHOUT last recompute's iteration counts (ps_options.iters_hint): the first
  # recompute of a run, or a caller that keeps no metrics.  Every block then takes the careful
  # path (averaged M updates); reported beside the hinted number, never instead of it.
  sec_no_hint = None
  if args.full and not args.workload.startswith("eigh") and not args.profile_hinted_only:
    kept, work.hint = work.hint, None
    _refresh, work.refresh_hint = work.refresh_hint, (lambda: None)
    sec_no_hint, _ = timed(work, max(2, args.steps // 2), 1, multi)
    work.refresh_hint = _refresh
    work.hint = kept
    work.step(); work.refresh_hint()   # metrics / hint of the state the later legs expect
  nb, n, _, p, _ = WORKLOADS[args.workload]
  iters = work.metrics[:, 1].cpu().numpy()
  errs = work.metrics[:, 0].cpu().numpy()

  line = {
      "metric": "preconditioner-recompute throughput, batched n x n inverse p-th root "
                "(algorithmic GFLOP/s; step time in ms_per_step)",
      "value": round(flops / sec / 1e9, 1),
      "unit": "GFLOP/s",
      "n_gpus": world,
      "steps": args.steps,
      "warmup": args.warmup,
      "ms_per_step": round(sec * 1e3, 3),
      "higher_is_better": True,
      "scaling": "weak",
      "vs_baseline": None,
      "dtype": "f32",
      "data": "selftest-cpu" if SELFTEST else "synthetic",
      "config": {
          "workload": f"{args.workload}: {nb} blocks/GPU of {n}x{n} fp32, p={p}, "
                      f"A=GG^T with G~N(0,1) [{n}x{WORKLOADS[args.workload][2]}], "
                      "ridge 1e-6 relative, Newton",
          "blocks_per_gpu": nb, "n": n, "p": p,
          "ms_per_step_no_hint": (round(sec_no_hint * 1e3, 3) if sec_no_hint else None),
          "parallelism": f"blocks partitioned over {world} GPU(s)" +
                         (", %s all-gather of roots in the timed region" % (
                             "RCCL" if (multi and not SELFTEST and
                                        not os.environ.get("PS_BENCH_ONE_DEVICE")) else "gloo (dev)")
                          if multi else ""),
          "newton_iters_per_block": {"min": float(iters.min()), "max": float(iters.max())},
          "max_newton_error": float(np.nanmax(errs)),
          # whole step (power iteration, init, control, copy-out included), EXECUTED flops
          "executed_frac_of_f32_mfma_peak": round(
              flops * executed_fraction(n, p, float(iters.mean()), float(work.metrics[:, 7].mean())) / sec / 1e12 /
              (PEAK_F32_MFMA_TFLOPS * world), 4),
      },
  }
  if not args.full:
    _emit(line, rank, multi)
    return

  if rank == 0 and world == 1 and not args.no_cpu_baseline and not args.workload.startswith("eigh"):
    line["parity_vs_oracle"] = parity_sample(work)
  if rank == 0:
    # (before the 1.5 s clock probe: the kernel is timed in the thermal state of the timed steps)
    stage_ms, launches, pi_ms, other_ms = profile_stage_kernel(work)
  clock = live_clock() if (rank == 0 and not SELFTEST) else {}
  if rank == 0:
    line["clock"] = clock
    fl1 = work.flops()
    ex = executed_fraction(n, p, float(iters.mean()), float(work.metrics[:, 7].mean()))
    alg = fl1 / (stage_ms * 1e-3) / 1e12 if stage_ms > 0 else 0.0
    ach = alg * ex
    # (the library reads PS_* only under PS_DEV_ENV=1: label the execution that actually ran)
    dev_env = os.environ.get("PS_DEV_ENV", "0") not in ("", "0")
    persistent = dev_env and os.environ.get("PS_NEWTON_PERSISTENT", "0") != "0"
    line["roofline"] = {
        "kernel": "newton_persistent_kernel" if persistent else "newton_stage_kernel",
        "bound": "mfma",
        # `achieved` = flops the MFMA pipe EXECUTES per launch / launch duration: the kernel
        # computes the upper tile triangle of every symmetric product ((T+1)/(2T) of the
        # algorithmic 2n^3) and mirrors it.  frac = achieved / peak.
        "achieved": round(ach, 2), "peak": PEAK_F32_MFMA_TFLOPS,
        "unit": "TFLOP/s", "frac": round(ach / PEAK_F32_MFMA_TFLOPS, 4),
        "executed_fraction_of_algorithmic_flops": round(ex, 4),
        # the SURVEY.md 8d convention (c(p) * 2n^3 per step) priced on the same time: a
        # rate of USEFUL work, not a fraction of hardware peak (it can exceed the peak)
        "algorithmic_equiv_tflops": round(alg, 2),
        # HBM bytes per launch come from separate rocprofv3 --pmc passes (2 x FETCH_SIZE + WRITE_SIZE
        # per the gfx950 rule) and cannot be collected inside this run: the figure is read from the
        # committed summary of the same workload (null if that file is not there)
        "traffic": _pmc_traffic_bytes("newton_stage_kernel"),
        "traffic_source": "profiles/r06_cfg2_pmc_by_kernel.json, hbm_MB_per_launch_corrected x 1e6 "
                          "(rocprofv3 --pmc, separate passes; tools/prof_pmc.sh): a committed measurement "
                          "of this workload, not a live one",
        "clock": clock,
        "frac_of_peak_at_measured_clock": (round(ach / clock["peak_at_clock_tflops"], 4)
                                           if "peak_at_clock_tflops" in clock else None),
        "launches": int(launches),
        "avg_launch_ms": round(stage_ms / max(launches, 1), 4),
        "executed_gflop_per_launch": round(fl1 * ex / max(launches, 1) / 1e9, 3),
        "algorithmic_gflop_per_launch": round(fl1 / max(launches, 1) / 1e9, 3),
        "note": ("one launch = the whole Newton iteration of the batch (init, every product "
                 "of every step, loop control, retries, copy-out) as a persistent dataflow "
                 "kernel") if persistent else "one launch = one product stage of the batch",
        "step_breakdown_ms": {"product_kernel": round(stage_ms, 3),
                              "power_iteration": round(pi_ms, 3),
                              "setup_seed_epilogue": round(other_ms, 3)},
        # the power iteration (reported separately): 100 matrix-vector passes.
        # Streaming execution (PS_PI_RESIDENT=0): HBM-bound, every pass re-reads the upper block
        # triangle ((T+1)/(2T) of the matrix).  Resident execution (default): the tiles stay in
        # registers for all passes, HBM is read once; a pass is bound by the tile mat-vecs on
        # the VALU and two hand-off latencies, so the bandwidth figures are "equivalent" ones.
        "power_iteration": {
            "execution": "streaming" if (dev_env and os.environ.get("PS_PI_RESIDENT", "1") == "0")
                         else "resident (matrices in registers, one launch per co-resident pass)",
            "ms": round(pi_ms, 3),
            "us_per_step": round(pi_ms * 10.0, 2),
            "bound": "hbm" if (dev_env and os.environ.get("PS_PI_RESIDENT", "1") == "0") else "valu+latency",
            "hbm_peak_GBps": 8000,
            "algorithmic_equiv_GBps": round(nb * n * n * 4 * 100 / max(pi_ms, 1e-9) / 1e6, 1),
            "upper_triangle_equiv_GBps": round(nb * n * n * 4 * 100 * ex / max(pi_ms, 1e-9) / 1e6,
                                               1)},
    }
  if multi:
    import torch.distributed as dist
    # self-diagnosis of a multi-GPU run: how many ranks answered, and one extra step split
    # into this rank's root computation and the all-gather tail that is NOT hidden under it
    rdev = "cpu" if dist.get_backend() == "gloo" else "cuda"
    ones = torch.ones(1, dtype=torch.int32, device=rdev)
    dist.all_reduce(ones, op=dist.ReduceOp.SUM)
    dist.barrier(); _sync()
    t0 = time.perf_counter(); work.compute(); _sync()
    t_compute = time.perf_counter() - t0
    dist.barrier(); _sync()
    t0 = time.perf_counter(); work.step(); _sync()
    t_step = time.perf_counter() - t0
    tt = torch.tensor([t_compute, t_step], dtype=torch.float64, device=rdev)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    line["config"]["rccl_ranks_seen"] = int(ones.item())   # the driver record keeps `config`
    line["multi_gpu"] = {
        "backend": "rccl" if dist.get_backend() == "nccl" else dist.get_backend(),
        "rccl_ranks_seen": int(ones.item()), "world_size": world,
        "roots_only_ms_max_over_ranks": round(tt[0].item() * 1e3, 3),
        "roots_plus_gather_ms_max_over_ranks": round(tt[1].item() * 1e3, 3),
        "gathered_bytes_per_rank": int(work.roots.numel() * 4),
        "gathered_list_matches_rank_order": bool(work.check_gathered_order(rank)),
    }
    dist.barrier()

  if not args.no_headline and args.workload != "headline_64x1024_p4":
    del work
    torch.cuda.empty_cache()
    hw = Workload("headline_64x1024_p4", rank, world, dev, multi)
    hsec, hflops = timed(hw, max(2, args.steps // 2), 1, multi)
    kept, hw.hint = hw.hint, None
    _refresh, hw.refresh_hint = hw.refresh_hint, (lambda: None)
    hsec_no_hint, _ = timed(hw, 2, 1, multi)
    hw.refresh_hint = _refresh
    hw.hint = kept
    hw.step(); hw.refresh_hint()
    hex_ = executed_fraction(1024, 4, float(hw.metrics[:, 5].double().mean().item()),
                             float(hw.metrics[:, 7].double().mean().item()))
    head = {"workload": "64 blocks/GPU of 1024x1024 fp32, p=4",
            "value": round(hflops / hsec / 1e9, 1), "unit": "GFLOP/s (algorithmic, SURVEY 8d)",
            "ms_per_step": round(hsec * 1e3, 3),
            "ms_per_step_no_hint": round(hsec_no_hint * 1e3, 3),
            "executed_fraction_of_algorithmic_flops": round(hex_, 4),
            # north_star bar: >= 40 % MFMA peak on this set; whole step, EXECUTED flops
            "executed_frac_of_f32_mfma_peak": round(
                hflops * hex_ / hsec / 1e12 / (PEAK_F32_MFMA_TFLOPS * world), 4)}
    if rank == 0:
      sm, ln, pm, om = profile_stage_kernel(hw)
      f1 = hw.flops()
      head["roofline"] = {
          "kernel": "newton_persistent_kernel" if (os.environ.get("PS_DEV_ENV", "0") not in ("", "0") and
                                                   os.environ.get("PS_NEWTON_PERSISTENT", "0") != "0")
                    else "newton_stage_kernel",
          "bound": "mfma", "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
          "achieved": round(f1 * hex_ / (sm * 1e-3) / 1e12, 2) if sm > 0 else None,
          "frac": round(f1 * hex_ / (sm * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4) if sm > 0 else None,
          "algorithmic_equiv_tflops": round(f1 / (sm * 1e-3) / 1e12, 2) if sm > 0 else None,
          "launches": int(ln), "avg_launch_ms": round(sm / max(ln, 1), 4),
          "frac_of_peak_at_measured_clock": (
              round(f1 * hex_ / (sm * 1e-3) / 1e12 / clock["peak_at_clock_tflops"], 4)
              if sm > 0 and "peak_at_clock_tflops" in clock else None)}
      if world == 1 and not args.no_cpu_baseline:
        head["parity_vs_oracle"] = parity_sample(hw, count=4)
      head["step_breakdown_ms"] = {"product_kernel": round(sm, 3),
                                   "power_iteration": round(pm, 3),
                                   "setup_seed_epilogue": round(om, 3)}
    if multi:
      import torch.distributed as dist
      dist.barrier()
    line["headline_1024"] = head
    # north_star's bar (>= 40 % of the fp32 MFMA peak on batched 1024^2, <= 1e-4 vs reference)
    # where the driver's record keeps it: the top-level `config`
    # FLAT scalars: the driver's record keeps the scalars of `config` and drops nested objects
    line["config"]["headline_1024_ms"] = head["ms_per_step"]
    line["config"]["headline_1024_ms_no_hint"] = head["ms_per_step_no_hint"]
    line["config"]["headline_1024_kernel_frac"] = (head.get("roofline") or {}).get("frac")
    line["config"]["headline_1024_step_executed_frac"] = head["executed_frac_of_f32_mfma_peak"]
    line["config"]["headline_1024_rel_fro"] = (head.get("parity_vs_oracle") or {}).get("rel_fro_max")
    del hw

  if not args.no_extras:
    torch.cuda.empty_cache()
    group = None
    if multi:
      import torch.distributed as dist
      group = dist.group.WORLD
    vw = VitBWorkload(rank, world, dev, group)
    vsteps = 2
    for _ in range(1):
      vw.step()
      vw.refresh_hint()
    _sync()
    if multi:
      dist.barrier()
    t0 = time.perf_counter()
    for _ in range(vsteps):
      vw.step()
    _sync()
    if multi:
      dist.barrier()
    vdt = (time.perf_counter() - t0) / vsteps
    if multi:
      t = torch.tensor([vdt], dtype=torch.float64,
                       device="cpu" if dist.get_backend() == "gloo" else "cuda")
      dist.all_reduce(t, op=dist.ReduceOp.MAX)
      vdt = t.item()
    vm = vw.metrics.cpu().numpy()
    vfl = vw.flops()
    vfl_ex = vw.flops(executed=True)
    # statistics kernel alone (HIP events on the launch stream = torch's current stream)
    vw.stats_step(); _sync()
    if SELFTEST:
      t0 = time.perf_counter(); vw.stats_step(); st_ms = (time.perf_counter() - t0) * 1e3
    else:
      # The host needs ~1 ms of Python to describe the 395 statistics; a few milliseconds of
      # unrelated GPU work queued in front of the first event keep the stream busy meanwhile, so
      # that the event pair brackets the descriptor upload + the kernel and not the host.
      filler = torch.randn((4096, 4096), device=dev)
      st_ms = 0.0
      for _ in range(5):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _f in range(4):
          torch.mm(filler, filler)
        ev0.record()
        vw.stats_step()
        ev1.record(); _sync()
        st_ms += ev0.elapsed_time(ev1) / 5
      # the two halves of the launch by themselves: matrix-shaped blocks (MFMA-bound) and the
      # d x d outer products of the vector blocks (HBM-bound: 8 d^2 bytes each)
      st_part = {}
      for sub in ("matrix", "vector"):
        vw.stats_step(sub); _sync()
        ms = 0.0
        for _ in range(5):
          ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
          for _f in range(4):
            torch.mm(filler, filler)
          ev0.record()
          its = vw.stats_step(sub)
          ev1.record(); _sync()
          ms += ev0.elapsed_time(ev1) / 5
        fl = by = 0.0
        for g_, axis_, _o, _n in its:
          d_ = g_.shape[axis_]; t_ = (d_ + 127) // 128
          fl += 2.0 * d_ * g_.numel() * (t_ + 1) / (2.0 * t_)
          by += 8.0 * d_ * d_
        st_part[sub] = (ms, fl, by, len(its))
      del filler
    st_fl = vw.stats_flops / (world if world > 1 else 1)  # owner-only statistics when sharded
    st_ex = vw.stats_executed_flops() / (world if world > 1 else 1)
    line["vit_b_cfg4"] = {
        "workload": "ViT-B/16 tree (200 leaves, 395 statistics, block_size 1024): statistics "
                    "update + all roots" + (" + all-gather" if multi else "") +
                    ", strong scaling (LPT ownership)",
        "ms_per_step": round(vdt * 1e3, 3),
        "roots_algorithmic_gflops": round(vfl / vdt / 1e9, 1),
        "roots_executed_gflops": round(vfl_ex / vdt / 1e9, 1),
        "roots_executed_frac_of_f32_mfma_peak": round(
            vfl_ex / vdt / 1e12 / (PEAK_F32_MFMA_TFLOPS * world), 4),
        "stats_gflop_per_step": round(vw.stats_flops / 1e9, 1),
        "stats_roofline": {
            "kernel": "stats_grouped_kernel (one launch per tree: both operand layouts + the "
                      "streaming tiles of the 149 vector statistics)",
            "bound": "mfma", "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
            # executed = upper tile triangle of each Gram matrix (mirrored in the epilogue)
            "achieved": round(st_ex / (st_ms * 1e-3) / 1e12, 2),
            "frac": round(st_ex / (st_ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4),
            "algorithmic_equiv_tflops": round(st_fl / (st_ms * 1e-3) / 1e12, 2),
            "ms_per_tree": round(st_ms, 3),
            "timing": "HIP events around the grouped call on the launch stream (descriptor "
                      "upload + kernel; the stream is kept busy while the host builds the "
                      "descriptors)",
            **({} if SELFTEST else {
                "matrix_blocks": {
                    "statistics": st_part["matrix"][3], "ms": round(st_part["matrix"][0], 3),
                    "bound": "mfma", "achieved_tflops": round(
                        st_part["matrix"][1] / (st_part["matrix"][0] * 1e-3) / 1e12, 2),
                    "frac": round(st_part["matrix"][1] / (st_part["matrix"][0] * 1e-3) / 1e12 /
                                  PEAK_F32_MFMA_TFLOPS, 4)},
                "vector_blocks": {
                    "statistics": st_part["vector"][3], "ms": round(st_part["vector"][0], 3),
                    "bound": "hbm", "peak_GBps": 8000,
                    "achieved_GBps": round(st_part["vector"][2] / (st_part["vector"][0] * 1e-3) / 1e9, 1),
                    "frac": round(st_part["vector"][2] / (st_part["vector"][0] * 1e-3) / 8e12, 4),
                    "note": "w1 S + w2 g g^T of a vector block reads and writes its d x d "
                            "statistic once: 8 d^2 bytes, no MFMA work; launched alone"}})},
        "newton_iters": {"min": float(vm[:, 1].min()), "max": float(vm[:, 1].max()),
                         "mean": round(float(vm[:, 1].mean()), 2)},
        "retries_max": float(vm[:, 4].max()),
        "failed_blocks": int((~(vm[:, 0] < 0.1)).sum()),
    }
    if world == 1 and rank == 0 and not args.no_cpu_baseline and not SELFTEST:
      from precondition_amd import comm as _comm   # roots of the statistics as they are NOW
      _flat = [s_ for st_ in vw.stats for s_ in st_]
      _roots, _met = _comm.sharded_inverse_pth_roots(_flat, vw.exps, group=None, ownership="lpt",
                                                     pi_first=True, iters_hint=vw.hint,
                                                     hint_in_ownership=False)
      _sync()
      line["vit_b_cfg4"]["parity_vs_oracle"] = parity_sample_vit_b(vw, _roots, _met)
      del _roots, _met, _flat
    if multi and not SELFTEST:
      # BASELINE configs[4] over the ranks of this run: 8 factors of dim 4096 dealt to the ranks (one
      # per GPU at N = 8), no exchange step inside an FD update -- measured on every rank, max over
      # ranks reported, to be read against fd_cfg5_rank_share of the N = 1 line
      import torch.distributed as dist
      try:
        fr = fd_cfg5(dev, factors=max(1, 8 // world))
        t = torch.tensor([float(np.median(fr["ms_per_factor_update"]))], dtype=torch.float64, device="cuda")
      except Exception as e:  # pylint: disable=broad-except
        fr, t = {"error": f"{type(e).__name__}: {e}"[:300]}, torch.tensor([float("nan")], dtype=torch.float64, device="cuda")
      dist.all_reduce(t, op=dist.ReduceOp.MAX)
      if rank == 0:
        line["fd_cfg5_sharded"] = {"factors_per_rank": max(1, 8 // world), "world": world,
                                   "ms_per_factor_update_max_over_ranks": round(t.item(), 3),
                                   "rank0": fr}
        line["config"]["fd_cfg5_sharded_ms_per_factor"] = round(t.item(), 3)
    if world == 1 and rank == 0 and not SELFTEST:
      try:
        line["vit_b_cfg4_rank_share"] = vit_b_rank_share(vw, dev)
      except Exception as e:  # pylint: disable=broad-except
        line["vit_b_cfg4_rank_share"] = {"error": f"{type(e).__name__}: {e}"[:300]}
    del vw
    if world == 1 and rank == 0:
      # single-GPU side measurements: a failure in one of them must not cost the line
      def eigh_cfg3():
        ew = Workload("eigh_cfg3_64x2048_p2", rank, 1, dev)
        ew.step(); _sync()
        samples = []
        for _ in range(3):
          t0 = time.perf_counter(); ew.step(); _sync()
          samples.append(time.perf_counter() - t0)
        edt = float(np.median(samples))
        conv = (6 + 2.0 / 3 + 4) * 2048.0 ** 3 * 64
        if not args.no_cpu_baseline:
          deferred.append(("eigh_cfg3", lambda: parity_sample_eigh(ew)))
        return {
            "workload": "64 blocks of 2048x2048 fp32, p=2, eigh path (Householder tridiagonalisation + "
                        "float64 divide and conquer + compact-WY back-transformation, "
                        "csrc/eigh_td.hip.h; eigh_solver auto: every block keeps that result -- at or "
                        "below a true float32 ssyevd's root error, profiles/r06_eigh_keep_rule.json)",
            "ms_per_step": round(edt * 1e3, 1),
            "ms_per_step_samples": [round(x * 1e3, 1) for x in samples],
            "jacobi_sweeps": float(ew.metrics[:, 5].max()),
            "error_metric_max": float(ew.metrics[:, 0].max()),
            "parity_vs_oracle": None,   # filled by the deferred pass below (after every timed leg)
            "conventional_gflops": round(conv / edt / 1e9, 1),
            "roofline": {"bound": "mfma", "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                         "achieved": round(conv / edt / 1e12, 2),
                         "frac": round(conv / edt / 1e12 / PEAK_F32_MFMA_TFLOPS, 4),
                         "convention": "SURVEY.md 8d: (6 2/3 + 4) n^3 per block incl. the error "
                                       "metric; the reduction's symmetric mat-vec is HBM-bound "
                                       "(n^3 / 6 * 4 bytes per block: kernel split in "
                                       "profiles/r05_eigh_*)"},
        }

      def fd_f32():
        old = {k: os.environ.get(k) for k in ("PS_FD_FILTER", "PS_FD_GRAM")}
        os.environ["PS_FD_FILTER"] = "f32"
        os.environ["PS_FD_GRAM"] = "f32"
        try:
          return fd_cfg5(dev)
        finally:
          for k, v in old.items():
            if v is None:
              os.environ.pop(k, None)
            else:
              os.environ[k] = v

      def fd_one():   # per-rank share of configs[4] on 8 GPUs: one factor per GPU
        r = fd_cfg5(dev, factors=1)
        return {"workload": r["workload"], "ms_per_factor_update": r["ms_per_factor_update"],
                "note": "BASELINE configs[4] over 8 GPUs = one 4096-dim factor per rank; no exchange "
                        "step inside an FD update"}

      def fd_main():
        r = fd_cfg5(dev)
        if not args.no_cpu_baseline:
          deferred.append(("fd_cfg5", lambda: fd_parity_literal(dev)))
        return r

      # Oracle work (float32 LAPACK through SciPy: sgesdd of 4096 x 8192, ssyevd of 2048^2 on all host cores)
      # runs AFTER every timed leg: the legs that are bound by the host's launch rate (eigh: ~25 000
      # launches per step, FD with one factor: ~360) measured 217 / 11.0 ms behind it against 172 / 9.3
      # standalone -- the BLAS worker threads of the checker disturb the enqueueing thread for a while.
      deferred = []
      for key, fn in (("newton_bf16x6", lambda: newton_bf16x6_leg(dev, clock)),
                      ("fd_cfg5", fd_main), ("fd_cfg5_f32_products", fd_f32),
                      ("fd_cfg5_rank_share", fd_one),
                      ("quant_f3", lambda: quant_f3(dev)), ("eigh_cfg3", eigh_cfg3)):
        torch.cuda.empty_cache()
        try:
          line[key] = fn()
        except Exception as e:  # pylint: disable=broad-except
          line[key] = {"error": f"{type(e).__name__}: {e}"[:300]}
      for key, fn in deferred:
        try:
          line[key]["parity_vs_oracle"] = fn()
        except Exception as e:  # pylint: disable=broad-except
          line[key]["parity_vs_oracle"] = {"error": f"{type(e).__name__}: {e}"[:300]}

  if rank == 0:
    cfg = line["config"]   # flat scalars only (the driver's record drops lists and objects)
    if isinstance(line.get("eigh_cfg3"), dict) and "ms_per_step" in line["eigh_cfg3"]:
      cfg["eigh_cfg3_ms"] = line["eigh_cfg3"]["ms_per_step"]
      cfg["eigh_cfg3_rel_fro"] = (line["eigh_cfg3"].get("parity_vs_oracle") or {}).get("rel_fro_max")
      cfg["eigh_cfg3_frac_of_f32_mfma_peak"] = (line["eigh_cfg3"].get("roofline") or {}).get("frac")
    if isinstance(line.get("fd_cfg5"), dict) and "ms_per_factor_update" in line["fd_cfg5"]:
      cfg["fd_cfg5_ms_per_factor"] = float(np.median(line["fd_cfg5"]["ms_per_factor_update"]))
      par = line["fd_cfg5"].get("parity_vs_oracle") or {}
      cfg["fd_cfg5_operator_rel_fro"] = par.get("operator_rel_fro_max")
      cfg["fd_cfg5_tail_rel"] = par.get("tail_rel_max")
    if isinstance(line.get("fd_cfg5_rank_share"), dict) and "ms_per_factor_update" in line["fd_cfg5_rank_share"]:
      cfg["fd_cfg5_one_factor_per_gpu_ms"] = float(np.median(line["fd_cfg5_rank_share"]["ms_per_factor_update"]))
    if isinstance(line.get("quant_f3"), dict) and "int16_quantize_plan_ms" in line["quant_f3"]:
      q3 = line["quant_f3"]
      cfg["quant_f3_int16_quantize_ms"] = q3.get("int16_quantize_plan_ms")
      cfg["quant_f3_int16_quantize_frac_of_hbm_peak"] = q3.get("int16_quantize_plan_frac_of_hbm_peak")
      cfg["quant_f3_int16_dequantize_ms"] = q3.get("int16_dequantize_plan_ms")
      cfg["quant_f3_int16_dequantize_frac_of_hbm_peak"] = q3.get("int16_dequantize_plan_frac_of_hbm_peak")
      cfg["quant_f3_int8_quantize_ms"] = q3.get("int8_quantize_plan_ms")
    rs8 = ((line.get("vit_b_cfg4_rank_share") or {}).get("worlds") or {}).get("8") or {}
    if "share_ms" in rs8:
      cfg["vit_b_cfg4_rank_share_world8_ms"] = rs8.get("share_ms")
      cfg["vit_b_cfg4_rank_share_world8_projected_speedup"] = rs8.get("projected_speedup")
    if isinstance(line.get("vit_b_cfg4"), dict):
      cfg["vit_b_cfg4_ms"] = line["vit_b_cfg4"].get("ms_per_step")
      vpar = line["vit_b_cfg4"].get("parity_vs_oracle") or {}
      if vpar:
        cfg["vit_b_cfg4_parity_passes"] = vpar.get("passes")
  if rank == 0 and world == 1 and not args.no_cpu_baseline:
    line["cpu_baseline"] = cpu_baseline(args.workload)
  _emit(line, rank, multi)


def _emit(line, rank, multi):
  """Rank 0 prints the line; every rank leaves the process group."""
  if rank == 0:
    def _plain(o):
      if isinstance(o, (np.floating, np.integer)):
        return o.item()
      raise TypeError(type(o))
    print(json.dumps(line, default=_plain), flush=True)
  if multi:
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
  main()
