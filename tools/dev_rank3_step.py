"""Every-step cost of update() on a tree with merged rank-3 parameters (dev only).

  python3 tools/dev_rank3_step.py [--tree resnet50|vitb] [--donate] [--bf16] [--block N]
                                  [--package-root DIR] [--dump DIR] [--launches]
  python3 tools/dev_rank3_step.py --stages

The default tree is ResNet-50 with its conv kernels in HWIO layout ([3,3,512,512] merges to
[9,512,512]: the three 3x3 kernels of the last stage keep rank 3) plus the dense layer and the
batch-norm vectors; steps without a root recompute are timed: GPU time per step from events around
20 back-to-back steps, host enqueue time into an empty queue, optionally the kernel launches of one
step (--launches: torch.profiler).  --package-root imports the package from another checkout (a
build of the parent commit, which has only the per-block path for this tree); --dump writes the
updates of the last step as .npy for a byte-for-byte comparison of two runs.

--stages times the grouped launches of one application stage on a uniform batch of blocks and
prints the fraction of the fp32 MFMA peak each reaches: rank-3 stage 1 (segmented operand A) and
stage 3 (segmented result) at m_seg = 128 and 64 against unsegmented products of the same m, n, k
(what the rank-2 stages A / B issue)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--package-root" in sys.argv:
  ROOT = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1])
sys.path.insert(0, ROOT)
import numpy as np, torch
import precondition_amd as pa

FP32_MFMA_PEAK_TFLOPS = 157.3
dev = torch.device("cuda:0")


def arg(name, default=None):
  return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def resnet50_shapes():
  shapes = [(7, 7, 3, 64), (64,), (64,)]
  cin = 64
  for width, blocks in ((64, 3), (128, 4), (256, 6), (512, 3)):
    for b in range(blocks):
      shapes += [(1, 1, cin, width), (width,), (width,), (3, 3, width, width), (width,), (width,),
                 (1, 1, width, 4 * width), (4 * width,), (4 * width,)]
      if b == 0:
        shapes += [(1, 1, cin, 4 * width), (4 * width,), (4 * width,)]
      cin = 4 * width
  return shapes + [(2048, 1000), (1000,)]


def median_range(xs):
  xs = sorted(xs)
  return f"{xs[len(xs) // 2]:.3f} ({xs[0]:.3f}-{xs[-1]:.3f})"


def step_timing():
  tree = arg("--tree", "resnet50")
  if tree == "vitb":
    import bench
    shapes, block = bench.VIT_B_SHAPES, 1024
  else:
    shapes, block = resnet50_shapes(), 128
  block = int(arg("--block", block))
  rng = np.random.default_rng(0)
  mk = lambda: [torch.from_numpy((rng.standard_normal(s) * 0.02).astype(np.float32)).to(dev) for s in shapes]
  params, grads = mk(), mk()
  if "--bf16" in sys.argv:
    params, grads = [p.to(torch.bfloat16) for p in params], [g.to(torch.bfloat16) for g in grads]
  kw = dict(donate_state=True) if "--donate" in sys.argv else {}
  opt = pa.distributed_shampoo(0.1, block, preconditioning_compute_steps=1000, start_preconditioning_step=1,
                               graft_type=pa.GraftingType.RMSPROP_NORMALIZED, **kw)
  st = opt.init(params)
  from precondition_amd import plan as P
  used = []
  orig = P.TreePlan.apply_preconditioners
  def spy(self, *a, **k):
    used.append(len(getattr(self, "r1_tbl", ())))
    return orig(self, *a, **k)
  P.TreePlan.apply_preconditioners = spy
  for _ in range(3):          # step 0 recomputes the roots
    upd, st = opt.update(grads, st, params)
  torch.cuda.synchronize()
  print(f"tree {tree}: {len(shapes)} parameters, block_size {block}, "
        f"{sum(int(np.prod(s)) for s in shapes) / 1e6:.1f} M elements; "
        f"tree plan applied the preconditioners: {bool(used)} (rank-3 blocks on it: {used[-1] if used else 0})")
  gpu, host = [], []
  for rep in range(5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(20):
      upd, st = opt.update(grads, st, params)
    e1.record()
    torch.cuda.synchronize()
    gpu.append(e0.elapsed_time(e1) / 20)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(2):
      upd, st = opt.update(grads, st, params)
    host.append((time.perf_counter() - t0) / 2 * 1e3)
    torch.cuda.synchronize()
  print(f"ms per step over 20 back-to-back steps, median (range) of 5: {median_range(gpu)}")
  print(f"host enqueue ms per step into an empty queue, median (range) of 5: {median_range(host)}")
  if "--launches" in sys.argv:
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
      upd, st = opt.update(grads, st, params)
      torch.cuda.synchronize()
    n = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
    print(f"kernel launches and copies of one step: {n}")
  if arg("--dump"):
    os.makedirs(arg("--dump"), exist_ok=True)
    for i, u in enumerate(upd):
      np.save(os.path.join(arg("--dump"), f"update_{i:03d}.npy"), u.float().cpu().numpy())


def stage_rates():
  import ctypes as C
  from precondition_amd import _lib, kernels as K
  lib = _lib.lib()
  nblk, reps = 96, 7
  def run(tbl):
    seg = tbl.dtype == K._GSEGDESC_DT
    descs = C.cast(tbl.ctypes.data, C.POINTER(_lib.GemmSegDesc if seg else _lib.GemmDesc))
    nbytes = (lib.ps_gemm_grouped_seg_workspace_bytes if seg else lib.ps_gemm_grouped_workspace_bytes)(descs, len(tbl))
    ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
    fn = lib.ps_gemm_grouped_seg_typed if seg else lib.ps_gemm_grouped_typed
    ts = []
    for r in range(reps + 2):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      rc = fn(torch.cuda.current_stream().cuda_stream, descs, len(tbl), 0, 0, ws.data_ptr(), ws.numel())
      e1.record()
      torch.cuda.synchronize()
      assert rc == 0, rc
      if r >= 2:
        ts.append(e0.elapsed_time(e1))
    flops = 2.0 * float(np.sum(tbl["m"].astype(np.float64) * tbl["n"] * tbl["k"]))
    ts.sort()
    med = ts[len(ts) // 2]
    return med, flops / (med * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS, ts[0], ts[-1]
  print(f"{nblk} blocks per launch; event time incl. the upload of the task tables; median of {reps}")
  for a, m_seg in ((128, 128), (128, 64), (9, 128)):
    # blocks [a, nseg, m_seg] of parents [a, 2 nseg, 2 m_seg]: stage 1 reads them segmented; blocks
    # [a, m_seg, c] of parents [a, 2 m_seg, c]: stage 3 writes them segmented
    nseg = 16
    m = nseg * m_seg
    parent = torch.randn((nblk, a, 2 * nseg, 2 * m_seg), device=dev)
    pa_ = torch.randn((a, a), device=dev)
    x1 = torch.empty((nblk, m, a), device=dev)
    dense = torch.randn((nblk, a, m), device=dev)
    s1 = np.zeros(nblk, K._GSEGDESC_DT)
    pl = np.zeros(nblk, K._GDESC_DT)
    for t, src, lda in ((s1, parent, 4 * nseg * m_seg), (pl, dense, m)):
      t["a"] = [src[i].data_ptr() for i in range(nblk)]
      t["b"] = pa_.data_ptr()
      t["c"] = [x1[i].data_ptr() for i in range(nblk)]
      t["m"], t["n"], t["k"], t["lda"], t["ldb"], t["ldc"], t["transa"] = m, a, a, lda, a, a, 1
    s1["m_seg"], s1["a_seg_stride"], s1["c_seg_stride"] = m_seg, 2 * m_seg, m_seg * a
    for name, t in (("stage 1, segmented A", s1), ("same products, unsegmented", pl)):
      med, frac, lo, hi = run(t)
      print(f"a={a:4d} m={m:6d} m_seg={m_seg:4d}  {name:28s} {med:.3f} ms ({lo:.3f}-{hi:.3f})  {frac:.3f} of the fp32 MFMA peak")
    # stage 3: X2 [c, (a b)] -> result rows (a', b') segmented; here c = m_seg columns, b = m_seg rows
    c = 128
    mm = a * m_seg
    x2 = torch.randn((nblk, c, mm), device=dev)
    pc = torch.randn((c, c), device=dev)
    outp = torch.empty((nblk, a, 2 * m_seg, c), device=dev)
    outd = torch.empty((nblk, mm, c), device=dev)
    s3 = np.zeros(nblk, K._GSEGDESC_DT)
    p3 = np.zeros(nblk, K._GDESC_DT)
    for t, dst in ((s3, outp), (p3, outd)):
      t["a"] = [x2[i].data_ptr() for i in range(nblk)]
      t["b"] = pc.data_ptr()
      t["c"] = [dst[i].data_ptr() for i in range(nblk)]
      t["m"], t["n"], t["k"], t["lda"], t["ldb"], t["ldc"], t["transa"] = mm, c, c, mm, c, c, 1
    s3["m_seg"], s3["a_seg_stride"], s3["c_seg_stride"] = m_seg, m_seg, 2 * m_seg * c
    for name, t in (("stage 3, segmented C", s3), ("same products, unsegmented", p3)):
      med, frac, lo, hi = run(t)
      print(f"a={a:4d} m={mm:6d} m_seg={m_seg:4d}  {name:28s} {med:.3f} ms ({lo:.3f}-{hi:.3f})  {frac:.3f} of the fp32 MFMA peak")


if __name__ == "__main__":
  if "--stages" in sys.argv:
    stage_rates()
  else:
    step_timing()
