// options.h — every mode switch of the library, resolved once per call.
//
// psh::resolve(ps_options*) turns the caller's ps_options (include/ps_api.h; NULL = defaults)
// into the flat struct below.  The fields after `dev` have no public spelling: they are the A/B
// switches that a test, a tool or a profiling recipe still sets, and keep their defaults unless the
// process runs with PS_DEV_ENV=1, in which case ps_dev_env_overrides() -- the ONLY function of the
// library that reads the environment -- applies the PS_* variables on top.
#pragma once
#include "../../include/ps_api.h"

namespace psh {

struct Options {
  // ---- public (ps_options) --------------------------------------------------------------------
  int products = PS_PRODUCTS_F32;
  int accumulation = PS_ACCUM_SEGMENTED;
  int averaged_steps = 4;
  const float* iters_hint = nullptr;
  int iters_hint_stride = 1;
  int fast_max_iters = 8;
  float averaged_err_threshold = 0.f;
  int execution = PS_EXEC_STAGED;
  int power_iteration = PS_PI_AUTO;
  double pi_timeout_ms = 5000.0;
  float eigh_sweep_tol = 2e-6f;
  int eigh_streams = 0;            // stream groups of the one-sided sweeps: 0 = default (2), 1 | 2
  int eigh_cj = 1;                 // eigh_solver TWO_SIDED clears it: one-sided block Jacobi for more than 128 rows (PS_EIGH_CJ)
  int eigh_td = 1;                 // eigh_solver AUTO / TRIDIAGONAL: eigh_td.hip.h for 129 ... 4096 rows (PS_EIGH_TD)
  int eigh_td_force = 0;           // eigh_solver TRIDIAGONAL: every block keeps the fast path's result
  float eigh_td_max_cond = 1e3f;   // ps_options.eigh_keep_max_cond: the ACCURATE rule keeps a block's result if it is positive definite with lambda_max / lambda_min below
  int eigh_td_accurate = 0;        // eigh_solver ACCURATE: the rule above in root calls too (AUTO: root calls keep every block, plain eigh keeps the rule)
  // ---- dev (environment, PS_DEV_ENV=1 only) -----------------------------------------------------
  bool force_general = false;      // PS_NEWTON_SYMMETRIC=0: full products for every block
  int pipe = 1;                    // PS_NEWTON_PIPE
  int grid_cap = 0;                // PS_NEWTON_GRID
  int newton_groups = 0;           // PS_NEWTON_GROUPS: stream groups of the staged execution (0 = default 2; 1 = one stream)
  bool newton_prof = false;        // PS_NEWTON_PROF
  const char* newton_trace = nullptr;  // PS_NEWTON_TRACE=<file>
  int stagger = -1;                // PS_NEWTON_STAGGER: -1 = auto (25 us when every tile of a launch has K >= 1024), 0 = off, else (mode << 16) | microseconds (dev)
  bool eigh_trace = false;         // PS_EIGH_TRACE
  int eigh_cj_refine = 1;          // PS_EIGH_CJ_REFINE
  int eigh_refine = 1;             // PS_EIGH_REFINE
  int eigh_td_stage = 0;           // PS_EIGH_TD_STAGE: 1 = stop after the reduction (Z_T = I; tests of the stages)
  int eigh_td_streams = 4;         // PS_EIGH_TD_STREAMS: stream groups of the reduction
  int eigh_td_tail = 192;          // PS_EIGH_TD_TAIL: last columns of a block reduced inside LDS (0: off; <= 192)
  int fd_groups = 1;               // PS_FD_GROUPS: 2 = a Frequent-Directions update of >= 4 factors runs as two groups on two streams (dev A/B: measured +-0)
};

// PS_EINVAL-style validation is the caller's: resolve() clamps what it does not understand to the
// defaults and reports it through *bad (may be NULL).
Options resolve(const ps_options* user, bool* bad = nullptr);

}  // namespace psh
