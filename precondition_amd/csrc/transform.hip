// transform.hip — fused, multi-tensor form of _transform_grad (reference DS:3496-3625):
// grafting (SGD / Adagrad / RMSProp (+normalised, +clip) / sqrt-n / none), norm
// matching of the preconditioned gradient, coupled or decoupled weight decay,
// momentum / Nesterov, for EVERY parameter of the tree in three launches.
//
// HBM-bound elementwise work with two to three per-parameter norms.  The norms
// are deterministic: each 4096-element chunk writes partial sums to a slab and
// every consumer workgroup re-reduces its parameter's partials in a fixed order
// (no float atomics).  Algorithmic bytes per element: pass A reads grad + pgrad
// (8 B), pass B reads grad + diag (8 B, only for Adagrad/RMSProp grafting), pass C
// reads up to 6 and writes up to 4 arrays (<= 40 B).  Int8 momenta (ps_transform_grads_q8) are decoded and
// encoded in registers: pass C then runs twice, C1 for the column maxima of the new momenta (14-18 B read) and C2
// for codes, update and diagonal statistics (14-18 B read, 10 B written); see the section below.
#include <math.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "gemm_core.hip.h"
#include "quant_math.h"

namespace psk {

constexpr int TCHUNK = 4096;
constexpr float T_EPS = 1e-25f;  // DS:41

enum Graft { G_NONE = 0, G_SGD = 1, G_ADAGRAD = 2, G_RMSPROP = 3, G_RMSPROP_N = 4,
             G_SQRT_N = 5, G_ADAGRAD_N = 6 };

struct TParam {
  const float* grad;
  const float* pgrad;   // preconditioned gradient; null => parameter skipped (DS:3557-3561)
  const float* param;   // may be null when weight_decay == 0
  const float* diag_in; // null unless Adagrad/RMSProp grafting
  float* diag_out;
  const float* mom_in;
  float* mom_out;
  const float* dmom_in;
  float* dmom_out;
  float* upd_out;
  int64_t numel;
  int chunk0, nchunks;
};

struct TChunk { int param; int idx; };

// chunk -> (parameter, chunk within it) from the per-parameter prefix chunk0: a binary
// search per workgroup instead of a host-built table of one entry per 4096 elements
// (21k entries for a ViT-B tree, rebuilt and uploaded every step).  Parameters without
// elements add no chunks; equal keys resolve to the last one, which owns the chunk.
__device__ inline TChunk find_chunk(const TParam* params, int count, int chunk) {
  int lo = 0, hi = count - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (params[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1;
  }
  return {lo, chunk - params[lo].chunk0};
}

__device__ inline bool has_diag(int g) {
  return g == G_ADAGRAD || g == G_RMSPROP || g == G_RMSPROP_N || g == G_ADAGRAD_N;
}
__device__ inline bool normalized(int g) { return g == G_RMSPROP_N || g == G_ADAGRAD_N; }

__device__ inline float block_sum(float v, float* red) {
  v = wave_sum_f32(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// fixed-order sum of one slab column over a parameter's chunks
__device__ inline float param_sum(const float* slab, int col, const TParam& p, float* red) {
  float s = 0.f;
  for (int c = threadIdx.x; c < p.nchunks; c += 256) s += slab[(int64_t)(p.chunk0 + c) * 4 + col];
  return block_sum(s, red);
}

// Storage of grad / upd_out (GH) and of param (PH): float32, or bf16 behind the same pointer
// fields (ps_transform_grads_typed).  A bf16 element widens exactly; the update is rounded to
// nearest even from the float32 value the float32 kernel stores.  Loads: gload1t (gemm_core.hip.h).
template <bool H>
__device__ __forceinline__ void tstore(float* p, int64_t i, float v) {
  if constexpr (H) {
    const __bf16 h = (__bf16)v;
    *(uint16_t PS_GLOBAL*)((uint16_t*)p + i) = __builtin_bit_cast(uint16_t, h);
  } else {
    gstore1(p + i, v);
  }
}

// pass A: slab[.][0] = sum (graft base)^2 ; slab[.][1] = sum pgrad^2
template <bool GH>
__global__ __launch_bounds__(256) void transform_pass_a(const TParam* params, int count,
                                                        float* slab, ps_transform_config cfg) {
  __shared__ float red[4];
  const TChunk ch = find_chunk(params, count, blockIdx.x);
  const TParam p = params[ch.param];
  const int64_t lo = (int64_t)ch.idx * TCHUNK;
  const int64_t hi = lo + TCHUNK < p.numel ? lo + TCHUNK : p.numel;
  float s0 = 0.f, s1 = 0.f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const float g = gload1t<GH>(p.grad, i);
    float base = g;
    if (cfg.graft_type == G_SQRT_N) base = g > 0.f ? 1.f : (g < 0.f ? -1.f : 0.f);
    s0 += base * base;
    if (p.pgrad) { const float q = gload1(p.pgrad + i); s1 += q * q; }
  }
  s0 = block_sum(s0, red);
  s1 = block_sum(s1, red);
  if (threadIdx.x == 0) {
    slab[(int64_t)(p.chunk0 + ch.idx) * 4 + 0] = s0;
    slab[(int64_t)(p.chunk0 + ch.idx) * 4 + 1] = s1;
  }
}

// Diagonal grafting update before lr / clipping (DS:3502-3528).
__device__ inline float diag_graft(float g, float gden, float diag, int graft, float w1,
                                   float w2, float eps, float& new_diag) {
  const float scaled = normalized(graft) ? g / gden : g;  // grad / (||grad|| + 1e-25)
  if (graft == G_ADAGRAD || graft == G_ADAGRAD_N) new_diag = diag + scaled * scaled;
  else new_diag = w1 * diag + w2 * (scaled * scaled);
  return scaled / (sqrtf(new_diag) + eps);
}

// pass B (Adagrad/RMSProp only): slab[.][2] = sum u^2 of the unclipped update
template <bool GH>
__global__ __launch_bounds__(256) void transform_pass_b(const TParam* params, int count,
                                                        float* slab, ps_transform_config cfg) {
  __shared__ float red[4];
  const TChunk ch = find_chunk(params, count, blockIdx.x);
  const TParam p = params[ch.param];
  float gscale = 1.f;
  if (normalized(cfg.graft_type)) gscale = sqrtf(param_sum(slab, 0, p, red)) + T_EPS;
  const int64_t lo = (int64_t)ch.idx * TCHUNK;
  const int64_t hi = lo + TCHUNK < p.numel ? lo + TCHUNK : p.numel;
  float s = 0.f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    float nd;
    const float u = diag_graft(gload1t<GH>(p.grad, i), gscale, gload1(p.diag_in + i), cfg.graft_type,
                               cfg.beta2_w1, cfg.beta2_w2, cfg.diagonal_epsilon, nd);
    s += u * u;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) slab[(int64_t)(p.chunk0 + ch.idx) * 4 + 2] = s;
}

// Per-parameter scalars of pass C: the norms re-reduced from the slab in a fixed order, and what
// the configuration fixes for every element.
struct TScalars {
  float gscale, clip_div, pm, mult, w, run, wd_lr, mm;
  bool coupled_wd, dec_wd;
};

__device__ __forceinline__ TScalars transform_scalars(const float* slab, const TParam& p,
                                                      const ps_transform_config& cfg, float* red) {
  TScalars s;
  const int graft = cfg.graft_type;
  const float r0 = param_sum(slab, 0, p, red);
  const float r1 = param_sum(slab, 1, p, red);
  float gnorm;
  s.gscale = 1.f; s.clip_div = 1.f;
  s.pm = cfg.decoupled_learning_rate ? 1.f : cfg.lr;  // DS:3549
  if (has_diag(graft)) {
    if (normalized(graft)) s.gscale = sqrtf(r0) + T_EPS;
    const float unorm = sqrtf(param_sum(slab, 2, p, red));
    if ((graft == G_RMSPROP || graft == G_RMSPROP_N) && cfg.clip_by_scaled_gradient_norm > 0.f) {
      const float scaled_norm = unorm / sqrtf((float)p.numel);  // DS:3531-3535
      s.clip_div = fmaxf(1.f, scaled_norm / cfg.clip_by_scaled_gradient_norm);
    }
    gnorm = unorm / s.clip_div * s.pm;
  } else {
    gnorm = sqrtf(r0) * s.pm;  // ||grad|| or sqrt(#nonzero) for sqrt-n
  }
  const float pnorm = p.pgrad ? sqrtf(r1) : gnorm;  // skipped: precond_grad = grafting_update
  s.mult = graft != G_NONE ? gnorm / (pnorm + T_EPS) : 1.f;  // DS:3566-3569
  s.w = cfg.moving_average_for_momentum ? 1.f - cfg.beta1 : 1.f;
  s.run = cfg.run_shampoo ? 1.f : 0.f;
  s.coupled_wd = cfg.weight_decay != 0.f && !cfg.decoupled_weight_decay;
  s.dec_wd = cfg.weight_decay != 0.f && cfg.decoupled_weight_decay;
  s.wd_lr = cfg.decoupled_learning_rate ? 1.f : cfg.lr;
  s.mm = cfg.decoupled_learning_rate ? cfg.lr : 1.f;  // DS:3610
  return s;
}

// What pass C makes of element i: the new diagonal statistic (diagonal grafting only), both new
// momenta and the update (float32, before its storage rounding).
struct TElem { float nd, smom, gmom, upd; };

// What pass C reads of element i besides the momenta (operands a configuration does not use are not loaded).
struct TIn { float g, diag, pg, prm; };

template <bool GH, bool PH>
__device__ __forceinline__ TIn transform_load(const TParam& p, const TScalars& s,
                                              const ps_transform_config& cfg, int64_t i) {
  TIn in;
  in.g = gload1t<GH>(p.grad, i);
  in.diag = has_diag(cfg.graft_type) ? gload1(p.diag_in + i) : 0.f;
  in.pg = p.pgrad ? gload1(p.pgrad + i) : 0.f;
  in.prm = (s.coupled_wd || s.dec_wd) ? gload1t<PH>(p.param, i) : 0.f;
  return in;
}

// Pass C's per-element arithmetic, from the element's operands and its two momenta as float32: the
// float32 kernel loads the momenta, the int8 kernels decode them.  Stores are the caller's.
__device__ __forceinline__ TElem transform_compute(const TParam& p, const TScalars& s,
                                                   const ps_transform_config& cfg, const TIn& in,
                                                   float mom, float dmom) {
  TElem e;
  const int graft = cfg.graft_type;
  const float g = in.g;
  float gu;
  e.nd = 0.f;
  if (has_diag(graft)) {
    gu = diag_graft(g, s.gscale, in.diag, graft, cfg.beta2_w1, cfg.beta2_w2, cfg.diagonal_epsilon, e.nd);
    gu = gu / s.clip_div;
  } else if (graft == G_SQRT_N) {
    gu = g > 0.f ? 1.f : (g < 0.f ? -1.f : 0.f);
  } else {
    gu = g;
  }
  gu = gu * s.pm;
  const float pg = p.pgrad ? in.pg : gu;
  float su = pg * s.mult;  // shampoo_update
  float sw = su, gw = gu;
  const float prm = in.prm;
  if (s.coupled_wd) { sw = su + cfg.weight_decay * prm; gw = gu + cfg.weight_decay * prm; }
  e.smom = mom * cfg.beta1 + s.w * sw;    // DS:3581-3586
  e.gmom = dmom * cfg.beta1 + s.w * gw;
  const float mom_u = s.run * e.smom + (1.f - s.run) * e.gmom;
  const float wd_u = s.run * sw + (1.f - s.run) * gw;
  float nest = mom_u;
  if (cfg.nesterov) nest = s.w * wd_u + cfg.beta1 * mom_u;           // DS:3601-3602
  if (s.dec_wd) nest = nest + s.wd_lr * cfg.weight_decay * prm;
  e.upd = -1.f * s.mm * nest;
  return e;
}

template <bool GH, bool PH>
__device__ __forceinline__ TElem transform_element(const TParam& p, const TScalars& s,
                                                   const ps_transform_config& cfg, int64_t i,
                                                   float mom, float dmom) {
  return transform_compute(p, s, cfg, transform_load<GH, PH>(p, s, cfg, i), mom, dmom);
}

// pass C: everything else, elementwise.  <storage of grad / upd_out, storage of param>
template <bool GH, bool PH>
__global__ __launch_bounds__(256) void transform_pass_c(const TParam* params, int count,
                                                        const float* slab, ps_transform_config cfg) {
  __shared__ float red[4];
  const TChunk ch = find_chunk(params, count, blockIdx.x);
  const TParam p = params[ch.param];
  const TScalars s = transform_scalars(slab, p, cfg, red);
  const bool diag = has_diag(cfg.graft_type);
  const int64_t lo = (int64_t)ch.idx * TCHUNK;
  const int64_t hi = lo + TCHUNK < p.numel ? lo + TCHUNK : p.numel;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const TElem e = transform_element<GH, PH>(p, s, cfg, i, gload1(p.mom_in + i), gload1(p.dmom_in + i));
    if (diag) gstore1(p.diag_out + i, e.nd);
    tstore<GH>(p.upd_out, i, e.upd);
    gstore1(p.mom_out + i, e.smom);
    gstore1(p.dmom_out + i, e.gmom);
  }
}

// ---- int8 momentum (ps_transform_grads_q8) ---------------------------------------------------------
// A parameter with cols > 0 keeps both momenta as int8 codes [numel / cols, cols] with one float32 bucket
// size per column (quant.hip); the column of flat element i is i mod cols.  Per element: decode (QU:109),
// pass C's body, encode with the NEW bucket size of the column (QU:85-94) -- which needs the maximum of
// the new momentum over the whole column first.  So pass C runs twice over such parameters:
//   C1  recomputes both new momenta and merges |.| into per-column maxima in the workspace
//       (atomicMax on the bit patterns: exact and order independent);
//   C2  recomputes them again (same slab, same fixed-order re-reduction, same operations: the same
//       bits), encodes and stores codes, update and diagonal statistics -- the thread that read an
//       element is the only one that writes it, and nothing is written before this pass;
//   a last small launch turns the maxima into bucket_out, after every read of bucket_in.
// Parameters with cols == 0 (float32 momenta) take pass C's float32 body inside C2.
struct TQuant {
  const signed char* mc_in;  signed char* mc_out;     // momentum: codes, bucket sizes
  const float* mb_in;        float* mb_out;
  const signed char* dc_in;  signed char* dc_out;     // diagonal momentum
  const float* db_in;        float* db_out;
  unsigned* colmax;          // workspace: [cols] momentum, then [cols] diagonal momentum
  int64_t cols;
  int schunk0, nschunks;     // C1's chunks of QCHUNK consecutive elements
};

constexpr int QCHUNK = 32768;    // elements per C1 workgroup: column maxima merge in LDS first
constexpr int QLDS_COLS = 4096;  // columns per momentum kept in LDS (wider: global atomics directly)

__device__ inline TChunk find_schunk(const TQuant* q, int count, int chunk) {
  int lo = 0, hi = count - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (q[mid].schunk0 <= chunk) lo = mid; else hi = mid - 1;
  }
  return {lo, chunk - q[lo].schunk0};
}

__device__ __forceinline__ int gload1c(const signed char* p) {
  return (int)*(const signed char PS_GLOBAL*)(p);
}
__device__ __forceinline__ unsigned gload1u(const unsigned* p) { return *(const unsigned PS_GLOBAL*)(p); }

constexpr int QU = 4;   // elements per thread whose loads are in flight together

// Everything C1 / C2 read of element i of an int8 parameter (column `col`).
struct TQIn { TIn t; int mc, dc; float mb, db; int64_t col; };

template <bool GH, bool PH>
__device__ __forceinline__ TQIn q8_load(const TParam& p, const TQuant& q, const TScalars& s,
                                        const ps_transform_config& cfg, int64_t i, int64_t col) {
  TQIn in;
  in.t = transform_load<GH, PH>(p, s, cfg, i);
  in.mc = gload1c(q.mc_in + i); in.mb = gload1(q.mb_in + col);
  in.dc = gload1c(q.dc_in + i); in.db = gload1(q.db_in + col);
  in.col = col;
  return in;
}

template <bool GH, bool PH>
__global__ __launch_bounds__(256) void transform_q8_pass_c1(const TParam* params, const TQuant* quants,
                                                            int count, const float* slab,
                                                            ps_transform_config cfg) {
  __shared__ float red[4];
  __shared__ unsigned s_max[2][QLDS_COLS];
  const TChunk ch = find_schunk(quants, count, blockIdx.x);
  const TParam p = params[ch.param];
  const TQuant q = quants[ch.param];
  const TScalars s = transform_scalars(slab, p, cfg, red);
  const int64_t cols = q.cols;
  const bool in_lds = cols <= QLDS_COLS;
  if (in_lds) {
    for (int c = threadIdx.x; c < (int)cols; c += 256) { s_max[0][c] = 0u; s_max[1][c] = 0u; }
    __syncthreads();
  }
  const int64_t lo = (int64_t)ch.idx * QCHUNK;
  const int64_t hi = lo + QCHUNK < p.numel ? lo + QCHUNK : p.numel;
  int64_t col = (lo + threadIdx.x) % cols;
  const int64_t step = 256 % cols;
  const auto merge = [&](const TElem& e, int64_t c) {
    const unsigned bm = __float_as_uint(fabsf(e.smom)), bd = __float_as_uint(fabsf(e.gmom));
    if (in_lds) {
      if (bm) atomicMax(&s_max[0][c], bm);
      if (bd) atomicMax(&s_max[1][c], bd);
    } else {
      if (bm) atomicMax(q.colmax + c, bm);
      if (bd) atomicMax(q.colmax + cols + c, bd);
    }
  };
  int64_t i = lo + threadIdx.x;
  // whole batches of QU elements per thread: every load of a batch is issued before its first use (one
  // element at a time the loop waits out a memory latency per element)
  for (; i + 256 * (QU - 1) < hi; i += 256 * QU) {
    TQIn in[QU];
#pragma unroll
    for (int u = 0; u < QU; ++u) {
      in[u] = q8_load<GH, PH>(p, q, s, cfg, i + 256 * u, col);
      col += step;
      if (col >= cols) col -= cols;
    }
#pragma unroll
    for (int u = 0; u < QU; ++u)
      merge(transform_compute(p, s, cfg, in[u].t, decode1(in[u].mc, in[u].mb), decode1(in[u].dc, in[u].db)),
            in[u].col);
  }
  for (; i < hi; i += 256) {
    const TQIn in = q8_load<GH, PH>(p, q, s, cfg, i, col);
    merge(transform_compute(p, s, cfg, in.t, decode1(in.mc, in.mb), decode1(in.dc, in.db)), in.col);
    col += step;
    if (col >= cols) col -= cols;
  }
  if (in_lds) {
    __syncthreads();
    for (int c = threadIdx.x; c < (int)cols; c += 256) {
      const unsigned a = s_max[0][c], b = s_max[1][c];
      if (a) atomicMax(q.colmax + c, a);
      if (b) atomicMax(q.colmax + cols + c, b);
    }
  }
}

template <bool GH, bool PH>
__global__ __launch_bounds__(256) void transform_q8_pass_c2(const TParam* params, const TQuant* quants,
                                                            int count, const float* slab,
                                                            ps_transform_config cfg) {
  __shared__ float red[4];
  const TChunk ch = find_chunk(params, count, blockIdx.x);
  const TParam p = params[ch.param];
  const TQuant q = quants[ch.param];
  const TScalars s = transform_scalars(slab, p, cfg, red);
  const bool diag = has_diag(cfg.graft_type);
  const int64_t lo = (int64_t)ch.idx * TCHUNK;
  const int64_t hi = lo + TCHUNK < p.numel ? lo + TCHUNK : p.numel;
  if (q.cols == 0) {   // float32 momenta: pass C as it is
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
      const TElem e = transform_element<GH, PH>(p, s, cfg, i, gload1(p.mom_in + i), gload1(p.dmom_in + i));
      if (diag) gstore1(p.diag_out + i, e.nd);
      tstore<GH>(p.upd_out, i, e.upd);
      gstore1(p.mom_out + i, e.smom);
      gstore1(p.dmom_out + i, e.gmom);
    }
    return;
  }
  const int64_t cols = q.cols;
  int64_t col = (lo + threadIdx.x) % cols;
  const int64_t step = 256 % cols;
  // (the thread that read an element is the one that writes it: x_out may be x_in)
  const auto finish = [&](const TQIn& in, int64_t i, unsigned max_m, unsigned max_d) {
    const TElem e = transform_compute(p, s, cfg, in.t, decode1(in.mc, in.mb), decode1(in.dc, in.db));
    if (diag) gstore1(p.diag_out + i, e.nd);
    tstore<GH>(p.upd_out, i, e.upd);
    *(signed char PS_GLOBAL*)(q.mc_out + i) = (signed char)encode1(e.smom, bucket_nonzero(bucket_size(max_m, 127.f)));
    *(signed char PS_GLOBAL*)(q.dc_out + i) = (signed char)encode1(e.gmom, bucket_nonzero(bucket_size(max_d, 127.f)));
  };
  int64_t i = lo + threadIdx.x;
  for (; i + 256 * (QU - 1) < hi; i += 256 * QU) {
    TQIn in[QU];
    unsigned mm[QU], md[QU];
#pragma unroll
    for (int u = 0; u < QU; ++u) {
      in[u] = q8_load<GH, PH>(p, q, s, cfg, i + 256 * u, col);
      mm[u] = gload1u(q.colmax + col);
      md[u] = gload1u(q.colmax + cols + col);
      col += step;
      if (col >= cols) col -= cols;
    }
#pragma unroll
    for (int u = 0; u < QU; ++u) finish(in[u], i + 256 * u, mm[u], md[u]);
  }
  for (; i < hi; i += 256) {
    finish(q8_load<GH, PH>(p, q, s, cfg, i, col), i, gload1u(q.colmax + col), gload1u(q.colmax + cols + col));
    col += step;
    if (col >= cols) col -= cols;
  }
}

// bucket_out = column maximum / 127 (QU:86), once every read of bucket_in is behind a launch boundary
__global__ __launch_bounds__(256) void transform_q8_buckets(const TQuant* quants) {
  const TQuant q = quants[blockIdx.x];
  for (int64_t c = (int64_t)blockIdx.y * 256 + threadIdx.x; c < q.cols; c += 256 * (int64_t)gridDim.y) {
    gstore1(q.mb_out + c, bucket_size(q.colmax[c], 127.f));
    gstore1(q.db_out + c, bucket_size(q.colmax[q.cols + c], 127.f));
  }
}

}  // namespace psk

using namespace psk;

extern "C" size_t ps_transform_grads_workspace_bytes(const ps_transform_desc* desc, int count) {
  if (!desc || count <= 0) return 0;
  size_t chunks = 0;
  for (int i = 0; i < count; ++i) chunks += (size_t)((desc[i].numel + TCHUNK - 1) / TCHUNK);
  return psh::align_up(sizeof(TParam) * count, 256) +
         psh::align_up(sizeof(float) * 4 * chunks, 256) + 1024;
}

static int transform_grads(void* stream, const ps_transform_desc* desc, int count,
                           const ps_transform_config* cfg, bool gh, bool ph, void* workspace,
                           size_t workspace_bytes) {
  PS_DEVICE_CHECK();
  if (!desc || !cfg || count <= 0 || !workspace) return PS_EINVAL;
  if (workspace_bytes < ps_transform_grads_workspace_bytes(desc, count)) return PS_EWORKSPACE;
  if (cfg->graft_type < 0 || cfg->graft_type > 6) return PS_EINVAL;
  const bool diag = cfg->graft_type == G_ADAGRAD || cfg->graft_type == G_RMSPROP ||
                    cfg->graft_type == G_RMSPROP_N || cfg->graft_type == G_ADAGRAD_N;
  std::vector<TParam> hp(count);
  long long chunk0 = 0;
  for (int i = 0; i < count; ++i) {
    const ps_transform_desc& d = desc[i];
    // a parameter without elements has no chunk and none of its pointers is read: an empty
    // tensor's null data pointer is fine
    if (d.numel < 0 ||
        (d.numel > 0 &&
         (!d.grad || !d.mom_in || !d.mom_out || !d.dmom_in || !d.dmom_out || !d.upd_out ||
          (diag && (!d.diag_in || !d.diag_out)) || (cfg->weight_decay != 0.f && !d.param))))
      return PS_EINVAL;
    if (d.numel > 0 && ((gh && ((uintptr_t)d.grad % 2 != 0 || (uintptr_t)d.upd_out % 2 != 0)) ||
                        (ph && (uintptr_t)d.param % 2 != 0)))
      return PS_EINVAL;
    TParam& p = hp[i];
    p.grad = d.grad; p.pgrad = d.pgrad; p.param = d.param; p.diag_in = d.diag_in;
    p.diag_out = d.diag_out; p.mom_in = d.mom_in; p.mom_out = d.mom_out;
    p.dmom_in = d.dmom_in; p.dmom_out = d.dmom_out; p.upd_out = d.upd_out;
    p.numel = d.numel;
    p.chunk0 = (int)chunk0;
    p.nchunks = (int)((d.numel + TCHUNK - 1) / TCHUNK);
    chunk0 += p.nchunks;
    if (chunk0 > 0x7fffffffLL) return PS_EUNSUPPORTED;
  }
  if (chunk0 == 0) return PS_OK;
  hipStream_t st = (hipStream_t)stream;
  psh::Arena ar(workspace, workspace_bytes);
  TParam* dp = ar.take<TParam>(count);
  float* slab = ar.take<float>(4 * (size_t)chunk0);
  if (ar.overflow) return PS_EWORKSPACE;
  PS_RC(psh::upload_async(st, dp, hp.data(), sizeof(TParam) * count));
  const dim3 grid((unsigned)chunk0), blk(256);
  const auto pass_a = gh ? transform_pass_a<true> : transform_pass_a<false>;
  const auto pass_b = gh ? transform_pass_b<true> : transform_pass_b<false>;
  const auto pass_c = gh ? (ph ? transform_pass_c<true, true> : transform_pass_c<true, false>)
                         : (ph ? transform_pass_c<false, true> : transform_pass_c<false, false>);
  hipLaunchKernelGGL(pass_a, grid, blk, 0, st, dp, count, slab, *cfg);
  if (diag) hipLaunchKernelGGL(pass_b, grid, blk, 0, st, dp, count, slab, *cfg);
  hipLaunchKernelGGL(pass_c, grid, blk, 0, st, dp, count, slab, *cfg);
  PS_LAUNCH_CHECK();
  return PS_OK;
}

extern "C" int ps_transform_grads_f32(void* stream, const ps_transform_desc* desc, int count,
                                      const ps_transform_config* cfg, void* workspace,
                                      size_t workspace_bytes) {
  return transform_grads(stream, desc, count, cfg, false, false, workspace, workspace_bytes);
}

extern "C" int ps_transform_grads_typed(void* stream, const ps_transform_desc* desc, int count,
                                        const ps_transform_config* cfg, int grad_dtype,
                                        int param_dtype, void* workspace, size_t workspace_bytes) {
  if ((grad_dtype != PS_DTYPE_F32 && grad_dtype != PS_DTYPE_BF16) ||
      (param_dtype != PS_DTYPE_F32 && param_dtype != PS_DTYPE_BF16))
    return PS_EINVAL;
  return transform_grads(stream, desc, count, cfg, grad_dtype == PS_DTYPE_BF16,
                         param_dtype == PS_DTYPE_BF16, workspace, workspace_bytes);
}

// ---- int8 momentum ----------------------------------------------------------------------------------
static size_t q8_chunks(const ps_transform_q8_desc* desc, int count, size_t* total_cols) {
  size_t chunks = 0, cols = 0;
  for (int i = 0; i < count; ++i) {
    if (desc[i].numel <= 0) continue;
    chunks += (size_t)((desc[i].numel + TCHUNK - 1) / TCHUNK);
    if (desc[i].cols > 0) cols += (size_t)desc[i].cols;
  }
  *total_cols = cols;
  return chunks;
}

extern "C" size_t ps_transform_grads_q8_workspace_bytes(const ps_transform_q8_desc* desc, int count) {
  if (!desc || count <= 0) return 0;
  size_t cols = 0;
  const size_t chunks = q8_chunks(desc, count, &cols);
  return psh::align_up(sizeof(TParam) * count, 256) + psh::align_up(sizeof(TQuant) * count, 256) +
         psh::align_up(sizeof(float) * 4 * chunks, 256) +
         psh::align_up(sizeof(unsigned) * 2 * cols, 256) + 1024;
}

// Descriptor validation and the two device tables' host images; no device is touched.  Returns
// PS_OK with the chunk totals, or the error the entry point returns before it writes anything.
static int q8_build(const ps_transform_q8_desc* desc, int count, const ps_transform_config* cfg,
                    bool gh, bool ph, std::vector<TParam>& hp, std::vector<TQuant>& hq,
                    long long* chunks, long long* schunks, size_t* total_cols) {
  if (cfg->graft_type < 0 || cfg->graft_type > 6) return PS_EINVAL;
  const bool diag = cfg->graft_type == G_ADAGRAD || cfg->graft_type == G_RMSPROP ||
                    cfg->graft_type == G_RMSPROP_N || cfg->graft_type == G_ADAGRAD_N;
  hp.assign(count, TParam{});
  hq.assign(count, TQuant{});
  long long chunk0 = 0, schunk0 = 0;
  size_t col0 = 0;
  for (int i = 0; i < count; ++i) {
    const ps_transform_q8_desc& d = desc[i];
    if (d.numel < 0 || d.cols < 0) return PS_EINVAL;
    TParam& p = hp[i];
    TQuant& q = hq[i];
    p.chunk0 = (int)chunk0;
    q.schunk0 = (int)schunk0;
    if (d.numel == 0) continue;   // no chunk, and none of its pointers is read
    if (!d.grad || !d.upd_out || (diag && (!d.diag_in || !d.diag_out)) ||
        (cfg->weight_decay != 0.f && !d.param))
      return PS_EINVAL;
    if (d.cols == 0) {
      if (!d.mom_in || !d.mom_out || !d.dmom_in || !d.dmom_out) return PS_EINVAL;
    } else if (d.numel % d.cols != 0 || !d.mom_codes_in || !d.mom_codes_out || !d.mom_bucket_in ||
               !d.mom_bucket_out || !d.dmom_codes_in || !d.dmom_codes_out || !d.dmom_bucket_in ||
               !d.dmom_bucket_out) {
      return PS_EINVAL;
    }
    if ((gh && ((uintptr_t)d.grad % 2 != 0 || (uintptr_t)d.upd_out % 2 != 0)) ||
        (ph && (uintptr_t)d.param % 2 != 0))
      return PS_EINVAL;
    p.grad = d.grad; p.pgrad = d.pgrad; p.param = d.param; p.diag_in = d.diag_in;
    p.diag_out = d.diag_out; p.mom_in = d.mom_in; p.mom_out = d.mom_out;
    p.dmom_in = d.dmom_in; p.dmom_out = d.dmom_out; p.upd_out = d.upd_out;
    p.numel = d.numel;
    p.nchunks = (int)((d.numel + TCHUNK - 1) / TCHUNK);
    chunk0 += p.nchunks;
    if (d.cols > 0) {
      q.mc_in = d.mom_codes_in; q.mc_out = d.mom_codes_out;
      q.mb_in = d.mom_bucket_in; q.mb_out = d.mom_bucket_out;
      q.dc_in = d.dmom_codes_in; q.dc_out = d.dmom_codes_out;
      q.db_in = d.dmom_bucket_in; q.db_out = d.dmom_bucket_out;
      q.cols = d.cols;
      q.colmax = reinterpret_cast<unsigned*>(2 * col0 * sizeof(unsigned));   // offset; rebased on the workspace
      col0 += (size_t)d.cols;
      q.nschunks = (int)((d.numel + QCHUNK - 1) / QCHUNK);
      schunk0 += q.nschunks;
    }
    if (chunk0 > 0x7fffffffLL) return PS_EUNSUPPORTED;
  }
  *chunks = chunk0; *schunks = schunk0; *total_cols = col0;
  return PS_OK;
}

extern "C" int ps_transform_grads_q8(void* stream, const ps_transform_q8_desc* desc, int count,
                                     const ps_transform_config* cfg, int grad_dtype, int param_dtype,
                                     void* workspace, size_t workspace_bytes) {
  PS_DEVICE_CHECK();
  if (!desc || !cfg || count <= 0 || !workspace) return PS_EINVAL;
  if ((grad_dtype != PS_DTYPE_F32 && grad_dtype != PS_DTYPE_BF16) ||
      (param_dtype != PS_DTYPE_F32 && param_dtype != PS_DTYPE_BF16))
    return PS_EINVAL;
  const bool gh = grad_dtype == PS_DTYPE_BF16, ph = param_dtype == PS_DTYPE_BF16;
  std::vector<TParam> hp;
  std::vector<TQuant> hq;
  long long chunks = 0, schunks = 0;
  size_t cols = 0;
  PS_RC(q8_build(desc, count, cfg, gh, ph, hp, hq, &chunks, &schunks, &cols));
  if (workspace_bytes < ps_transform_grads_q8_workspace_bytes(desc, count)) return PS_EWORKSPACE;
  if (chunks == 0) return PS_OK;
  const bool diag = cfg->graft_type == G_ADAGRAD || cfg->graft_type == G_RMSPROP ||
                    cfg->graft_type == G_RMSPROP_N || cfg->graft_type == G_ADAGRAD_N;
  hipStream_t st = (hipStream_t)stream;
  psh::Arena ar(workspace, workspace_bytes);
  TParam* dp = ar.take<TParam>(count);
  TQuant* dq = ar.take<TQuant>(count);
  float* slab = ar.take<float>(4 * (size_t)chunks);
  unsigned* colmax = ar.take<unsigned>(2 * cols);
  if (ar.overflow) return PS_EWORKSPACE;
  for (TQuant& q : hq)
    if (q.cols > 0) q.colmax = reinterpret_cast<unsigned*>((char*)colmax + (uintptr_t)q.colmax);
  PS_RC(psh::upload_async(st, dp, hp.data(), sizeof(TParam) * count));
  PS_RC(psh::upload_async(st, dq, hq.data(), sizeof(TQuant) * count));
  // the maxima start from zero on every call: nothing is assumed about the workspace
  if (cols) PS_HIP(hipMemsetAsync(colmax, 0, sizeof(unsigned) * 2 * cols, st));
  const dim3 grid((unsigned)chunks), blk(256);
  const auto pass_a = gh ? transform_pass_a<true> : transform_pass_a<false>;
  const auto pass_b = gh ? transform_pass_b<true> : transform_pass_b<false>;
  const auto pass_c1 = gh ? (ph ? transform_q8_pass_c1<true, true> : transform_q8_pass_c1<true, false>)
                          : (ph ? transform_q8_pass_c1<false, true> : transform_q8_pass_c1<false, false>);
  const auto pass_c2 = gh ? (ph ? transform_q8_pass_c2<true, true> : transform_q8_pass_c2<true, false>)
                          : (ph ? transform_q8_pass_c2<false, true> : transform_q8_pass_c2<false, false>);
  hipLaunchKernelGGL(pass_a, grid, blk, 0, st, dp, count, slab, *cfg);
  if (diag) hipLaunchKernelGGL(pass_b, grid, blk, 0, st, dp, count, slab, *cfg);
  if (schunks)
    hipLaunchKernelGGL(pass_c1, dim3((unsigned)schunks), blk, 0, st, dp, dq, count, slab, *cfg);
  hipLaunchKernelGGL(pass_c2, grid, blk, 0, st, dp, dq, count, slab, *cfg);
  if (schunks) hipLaunchKernelGGL(transform_q8_buckets, dim3((unsigned)count, 32), blk, 0, st, dq);
  PS_LAUNCH_CHECK();
  return PS_OK;
}
