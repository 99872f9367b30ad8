"""Leading eigenpairs of symmetric PSD matrices by Chebyshev-filtered subspace iteration.

Used by the Frequent-Directions branch (config 5, DS:1123-1290), which needs only the
top rank+1 singular values / rank singular vectors of the d x d covariance update but
gets them in the reference from a full SVD of a d x (rank+d) factor (DS:1193).  Here the
heavy work is d x d @ d x b products (b = k + oversampling columns) on the fp32 MFMA GEMM
(`ps_gemm_grouped_f32`, all matrices of a call in one launch), the small b x b Gram /
Rayleigh-Ritz problems go to the batched Jacobi eigensolver (`ps_eigh_batched_f32`), and
the O(d b) recurrences run in fused kernels over the stacked iterates (csrc/fd.hip).

Algorithm (Zhou & Saad's scaled Chebyshev filter inside subspace iteration):
  X <- orth(random d x b);  Rayleigh-Ritz -> theta_1 >= ... >= theta_b, X <- Ritz vectors
  repeat: X <- p(C) X with p the degree-m Chebyshev polynomial that damps [0, theta_b]
          and is scaled to 1 at theta_1;  X <- orth(X) (CholeskyQR of the Gram matrix, or its
          eigendecomposition for wide blocks, + one Newton-Schulz polish);  Rayleigh-Ritz;
          stop when the residuals ||C x_i - theta_i x_i|| of the k wanted pairs are below
          tol * theta_1.
The caller falls back to the full eigendecomposition if this does not converge.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

import torch


def _K():
  from . import kernels
  return kernels


def _gemm(items):
  _K().gemm_grouped(items)


def _small_eigh_desc(mats: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
  """Batched eigh of [B, b, b] symmetric matrices, eigenvalues DESCENDING."""
  sym = 0.5 * (mats + mats.transpose(1, 2))
  es, us = _K().eigh_batched(list(sym.unbind(0)))
  e = torch.stack(es, 0).flip(1)
  u = torch.stack(us, 0).flip(2)
  return e, u


def _use_cholqr(b: int) -> bool:
  """CholeskyQR where the library's ps_chol_rinv kernel takes the block width (b <= 96), else the
  eigen-based form of _Planned.orthonormalize."""
  from . import _lib
  return b <= _lib.lib().ps_chol_rinv_max_n()


class _Planned:
  """Orthonormalisation and Rayleigh-Ritz of one top_eigenpairs_batched call on persistent buffers,
  every product a kernels.GemmPlan: the eight products of an outer round are built once per call
  and launched ~6 times."""

  def __init__(self, c, x, z, tmp, c16x6=None):
    K = _K()
    bsz, n, b = x.shape
    dev = x.device
    self.c, self.x, self.z, self.tmp = c, x, z, tmp
    self._rd = None
    self.c16x6 = c16x6      # three-plane fragment-major covariances: C x of Rayleigh-Ritz by fd_cx6
    self.x6_scratch = None
    if c16x6 is not None:
      self.x6_scratch = [torch.empty((bsz * n * b,), dtype=torch.bfloat16, device=dev) for _ in range(3)]
    mk = lambda: torch.empty((bsz, b, b), dtype=torch.float32, device=dev)
    self.gram, self.m, self.polish, self.t, self.y = mk(), mk(), mk(), mk(), mk()
    self.eye = torch.eye(b, dtype=torch.float32, device=dev)
    R = range(bsz)
    self.p_gram_x = K.GemmPlan([(x[j], x[j], self.gram[j], True, False) for j in R])
    self.p_xm = K.GemmPlan([(x[j], self.m[j], tmp[j], False, False) for j in R])
    self.p_gram_t = K.GemmPlan([(tmp[j], tmp[j], self.gram[j], True, False) for j in R])
    self.p_pol = K.GemmPlan([(tmp[j], self.polish[j], x[j], False, False) for j in R])
    self.p_cx = K.GemmPlan([(c[j], x[j], z[j], False, False) for j in R])
    self.p_xtz = K.GemmPlan([(x[j], z[j], self.t[j], True, False) for j in R])
    self.p_xy = K.GemmPlan([(x[j], self.y[j], tmp[j], False, False) for j in R])
    self.p_zy = K.GemmPlan([(z[j], self.y[j], tmp[j], False, False) for j in R])

  def round_call(self, k, tol, degree, orthonormalize=True):
    """orthonormalize (optional) + Rayleigh-Ritz + the per-round control in ONE library call
    (ps_fd_round_f32: the ~35 launches of these steps issued from C++ instead of one by one from
    Python -- the host was the limit of a round with few factors).  Returns (theta, res, params,
    converged, summary) as persistent device tensors, or None where the call does not apply."""
    from . import _lib
    L = _lib.lib()
    bsz, n, b = (int(v) for v in self.x.shape)
    if b < 32 or not _use_cholqr(b) or b > L.ps_eigh_sorted_max_n():
      return None
    if self._rd is None:
      dev = self.x.device
      d = _lib.FdRoundDesc()
      f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
      keep = dict(sym=f32(bsz, b, b), evals=f32(bsz, b), evecs=f32(bsz, b, b), theta=f32(bsz, b), res=f32(bsz, b),
                  params=f32(bsz, 4), converged=torch.empty((bsz,), dtype=torch.int32, device=dev),
                  summary=torch.empty((4,), dtype=torch.int32, device=dev))
      nn = (C.c_int32 * bsz)(*([b] * bsz))
      keep["ews"] = torch.empty((max(int(L.ps_eigh_root_workspace_bytes(bsz, nn)), 256),), dtype=torch.uint8, device=dev)
      for name, plan in (("gram_x", self.p_gram_x), ("xm", self.p_xm), ("gram_t", self.p_gram_t), ("pol", self.p_pol),
                         ("cx", self.p_cx), ("xtz", self.p_xtz), ("xy", self.p_xy), ("zy", self.p_zy)):
        setattr(d, name, plan._h.value)
      if self.c16x6 is not None:
        ptrs = [(C.c_void_p * bsz)() for _ in range(3)]
        for j, a in enumerate(self.c16x6):
          ptrs[0][j], ptrs[1][j], ptrs[2][j] = a.hi.data_ptr(), a.lo.data_ptr(), a.lo2.data_ptr()
        keep["ptrs"] = ptrs
        d.c0, d.c1, d.c2 = (C.cast(p, C.c_void_p).value for p in ptrs)
        d.xt0, d.xt1, d.xt2 = (t.data_ptr() for t in self.x6_scratch)
      for name, t in (("x", self.x), ("z", self.z), ("tmp", self.tmp), ("gram", self.gram), ("m", self.m),
                      ("polish", self.polish), ("t", self.t), ("y", self.y)):
        setattr(d, name, t.data_ptr())
      for name in ("sym", "evals", "evecs", "theta", "res", "params", "converged", "summary"):
        setattr(d, name, keep[name].data_ptr())
      d.eigh_workspace, d.eigh_workspace_bytes = keep["ews"].data_ptr(), keep["ews"].numel()
      d.batch, d.n, d.b = bsz, n, b
      self._rd, self._rd_keep = d, keep
    d, keep = self._rd, self._rd_keep
    d.k, d.degree, d.tol, d.orthonormalize = int(k), int(degree), float(tol), 1 if orthonormalize else 0
    with torch.cuda.device(self.x.device):
      _lib.check(L.ps_fd_round_f32(torch.cuda.current_stream().cuda_stream, C.byref(d)), "ps_fd_round_f32")
    return keep["theta"], keep["res"], keep["params"], keep["converged"], keep["summary"]

  def orthonormalize(self):
    """Columns of every x[j] ([B, n, b]) made orthonormal: x <- x M with M = R^-1 of the Gram matrix
    G = R^T R (CholeskyQR, float64 on the device) or, for wider blocks, M = U L^{-1/2} of its
    eigendecomposition; then one Newton-Schulz step x <- x (1.5 I - 0.5 x^T x).  Directions below
    1e-10 of the largest Gram eigenvalue / diagonal entry (a rank-deficient C) are dropped (zero
    columns, Ritz value 0; their zero row / column in the Gram matrix leaves 1.5 I harmless)."""
    b = self.x.shape[2]
    self.p_gram_x.launch()
    if _use_cholqr(b):
      _K().chol_rinv_batched(self.gram, 1e-10, out=self.m)
    else:
      lam, u = _small_eigh_desc(self.gram)
      keep = lam > 1e-10 * lam[:, :1].clamp_min(1e-30)
      scale = torch.where(keep, lam.clamp_min(1e-30).rsqrt(), torch.zeros_like(lam))
      self.m.copy_(u * scale[:, None, :])
    self.p_xm.launch()
    self.p_gram_t.launch()
    torch.add(self.eye * 1.5, self.gram, alpha=-0.5, out=self.polish)
    self.p_pol.launch()
    return self.x

  def rayleigh_ritz(self):
    """x orthonormal.  Returns (theta desc [B, b], residual norms [B, b]); x holds the Ritz vectors
    and z = C x afterwards."""
    if self.c16x6 is not None:   # z = C x on the bf16 MFMA, three planes per operand: float32 accuracy
      _K().fd_cx6(self.c16x6, self.x, self.z, self.x6_scratch)
    else:
      self.p_cx.launch()
    self.p_xtz.launch()
    theta, y = _small_eigh_desc(self.t)
    self.y.copy_(y)
    self.p_xy.launch()
    self.x.copy_(self.tmp)
    self.p_zy.launch()
    self.z.copy_(self.tmp)
    res = torch.linalg.vector_norm(self.z - self.x * theta[:, None, :], dim=1)
    return theta, res


def _filter_precision(n: int) -> str:
  """Arithmetic of the Chebyshev filter's C @ Y products (the bulk of the work; the
  Rayleigh-Ritz products and residuals are always float32 MFMA):
    "f32"    exact-f32 MFMA (v_mfma_f32_32x32x2_f32);
    "bf16x3" bf16 MFMA on hi/lo pairs of C and Y (hi*hi + lo*hi + hi*lo, float32
             accumulation): ~2^-17 operand precision at the byte traffic of float32, i.e.
             HBM-bound instead of MFMA-bound;
    "bf16"   plain bf16 operands while the residuals are above the bf16 floor, then bf16x3
             (BASELINE configs[4] names bf16 MFMA for this branch).
  Default bf16x3 where the bf16 kernel's alignment rules hold (n % 32 == 0);
  PS_FD_FILTER overrides.  This and low_rank._gram_precision's PS_FD_GRAM are the only
  environment reads of the Python host: bench.py's --full fd_f32 leg sets both."""
  import os
  mode = os.environ.get("PS_FD_FILTER", "bf16x3")
  if mode not in ("f32", "bf16x3", "bf16"):
    raise ValueError(f"PS_FD_FILTER must be f32, bf16x3 or bf16, got {mode!r}")
  return mode if n % 32 == 0 else "f32"


def top_eigenpairs_batched(mats: Sequence[torch.Tensor], k: int, tol: float = 1e-5,
                           degree: int = 12, max_outer: int = 14, oversample: int = 31,
                           seed: int = 1729):
  """Leading k eigenpairs of each symmetric PSD matrix in `mats` (all n x n with the same
  n, float32, on the GPU).  Returns (evals [B, k] descending, evecs [B, n, k], converged
  [B] bool, info dict).  Deterministic (fixed-seed start block)."""
  bsz = len(mats)
  n = int(mats[0].shape[0])
  dev = mats[0].device
  b = min(n, ((k + oversample + 31) // 32) * 32)
  c = [m if m.is_contiguous() else m.contiguous() for m in mats]
  mode = _filter_precision(n)
  c16 = None
  # fragment-major with a third plane (the kilobyte one MFMA consumes is contiguous): every filter step after
  # the first is ONE launch (ps_fd_cy_step_f32), and the float32-accurate C x of Rayleigh-Ritz runs on the bf16
  # MFMA as well; else tile-blocked (128 x 32 tiles contiguous: the product streams whole DRAM pages of C)
  frag3 = mode == "bf16x3" and _K().fd_frag_supported(bsz, n, b)
  if mode != "f32":  # the covariance is converted ONCE per call (hi/lo pair)
    c16 = [_K().to_bf16(m, split=True, tiled="frag3" if frag3 else True) for m in c]

  gen = torch.Generator(device=dev).manual_seed(seed)
  x = torch.randn((bsz, n, b), generator=gen, device=dev, dtype=torch.float32)
  z = torch.empty_like(x)
  tmp = torch.empty_like(x)
  planned = _Planned(c, x, z, tmp, c16x6=c16 if frag3 else None)
  # orthonormalisation + Rayleigh-Ritz + the control of the next round in one library call where it applies
  rc = planned.round_call(k, tol, degree)
  lib_round = rc is not None
  if lib_round:
    theta, res, params, conv_i, summ = rc
  else:
    planned.orthonormalize()
    theta, res = planned.rayleigh_ritz()
  gemms = 1
  converged = torch.zeros((bsz,), dtype=torch.bool, device=dev)
  outer = 0
  scratch = None   # two more [B, n, b] iterates of the filter, allocated once per call
  for outer in range(1, max_outer + 1):
    # convergence test + filter interval + per-factor degree in ONE small launch and one host read
    # (csrc/fd.hip fd_round_control_kernel), or from the round call
    if not lib_round:
      params, conv_i, summ = _K().fd_round_control(theta, res, k, n, tol, degree)
    all_conv, max_deg, _, plain_ok = summ.tolist()
    converged = conv_i.bool()
    if all_conv:
      break
    # z = C x is current from the Rayleigh-Ritz step
    if c16 is not None:
      # The whole filter in ONE library call (ps_fd_filter_round_f32): the product's task tables are
      # uploaded once and the host does nothing between the ~3 launches of a step.
      if scratch is None:
        scratch = (torch.empty_like(x), torch.empty_like(x))
      y_b = _K().fd_filter_round(c16, z, [x, scratch[0], scratch[1]], params, max_deg,
                                 plain=mode == "bf16" and bool(plain_ok))
      gemms += max(max_deg - 1, 0)
    else:
      # float32 products between fused recurrence steps (csrc/fd.hip), every factor in one launch
      y_prev_b, y_b, y_next_b = x, torch.empty_like(x), torch.empty_like(x)   # rotate
      _K().fd_filter_step(z, y_prev_b, None, y_b, params, 1, want_bf16=False)
      for step in range(2, max_deg + 1):
        _gemm([(c[j], y_b[j], z[j], False, False) for j in range(bsz)])
        gemms += 1
        _K().fd_filter_step(z, y_b, y_prev_b, y_next_b, params, step, want_bf16=False)
        y_prev_b, y_b, y_next_b = y_b, y_next_b, y_prev_b
    if y_b is not x:
      x.copy_(y_b)
    if lib_round:
      theta, res, params, conv_i, summ = planned.round_call(k, tol, degree)
    else:
      planned.orthonormalize()
      theta, res = planned.rayleigh_ritz()
    gemms += 1
  else:
    top = theta[:, :1].clamp_min(1e-30)
    wanted = theta[:, :k] > n * 2.4e-7 * top
    converged = ((res[:, :k] <= tol * top) | ~wanted).all(dim=1)
  info = {"outer_iterations": outer, "big_gemms": gemms, "block": b, "filter_precision": mode,
          "max_residual_rel": float((res[:, :k] / theta[:, :1].clamp_min(1e-30)).max())}
  return theta[:, :k].contiguous(), x[:, :, :k].contiguous(), converged, info
