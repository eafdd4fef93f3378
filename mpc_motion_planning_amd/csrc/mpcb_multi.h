// mpcb_multi.h — the two glue kernels of the multi-start solve (mpcb_solve_multi, include/mpcbatch_multi.h): K starts per instance, the best
// solution kept on the device.
//
//   mpcbm::expand (kernel mpcb_multi_expand)
//                       one wave per expanded instance e = b * K + k: writes the start row of candidate k of instance b and replicates
//                       x0, xs and the obstacle rows of b into the expanded batch that one ordinary solve of K * B instances reads.
//   mpcbm::select (kernel mpcb_multi_select)
//                       one wave per instance b: walks the K candidates in index order, keeps the winner, counts the eligible candidates
//                       and the distinct solutions, and copies the winner's rows out.
//
// Both are copies with a little wave-uniform control flow around them: every row is read and written lane-strided (coalesced), nothing
// goes through LDS.  Written against mpcb_wave.h like mpcb_eval.h, so tests/emu_multi steps exactly this code on the CPU.
#pragma once

#include "mpcb_plant.h"    // mpcbp::step_failed: the rule "neither solved nor acceptable" is stated there

#include <cstddef>

#ifndef MPCB_MULTI_MAX
#define MPCB_MULTI_MAX 8
#endif

// Every multi kernel takes ONE argument, a MpcbMultiArgs by value.  Expanded arrays (*_e, *_all) have K * B rows, row e = b * K + k.
struct MpcbMultiArgs {
  int32_t B, K, N, nx, nz, ng;
  int32_t obs_row;                         // doubles of one instance's obstacle rows: n_obs * 6 (static) or n_obs * (N + 1) * 6 (predicted); 0: none
  double controls[2 * MPCB_MULTI_MAX];     // (steer, accel) of candidate k at [2k], [2k + 1]
  double obj_margin, basin_tol;
  // expand: the caller's batch in, the expanded batch out
  const double *x0, *xs, *obs, *z0;        // z0: [B, nz] the caller's start of candidate 0, or NULL
  double *x0_e, *xs_e, *obs_e, *z0_e;
  // select: the K * B results in, the winner's out (lam_g, lam_x, kkt, iters: with their *_all twin, or both NULL)
  const double *z_all, *obj_all, *kkt_all, *lam_g_all, *lam_x_all;
  const int32_t *status_all, *iters_all;
  double *z, *obj, *kkt, *lam_g, *lam_x;
  int32_t *status, *iters, *which, *n_ok, *n_basins;
};

namespace mpcbm {

// dst[0..n) <- src[0..n), lane i takes elements i, i + 64, ...: consecutive lanes touch consecutive doubles
MPCB_DEV void copy_row(double* __restrict__ dst, const double* __restrict__ src, int n, int lane) {
  for (int i = lane; i < n; i += 64) dst[i] = src[i];
}

// a candidate takes part in the selection when its solve ended solved or acceptable and its objective is a finite number
MPCB_DEV bool eligible(int status, double obj) { return !mpcbp::step_failed(status) && obj - obj == 0.0; }

// does a later eligible candidate with objective `obj` replace the incumbent?  Only by more than the margin, relative above |obj| = 1.
MPCB_DEV bool replaces(double obj, double obj_inc, double obj_margin) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double scale = fabs(obj_inc) > 1.0 ? fabs(obj_inc) : 1.0;
  const double bar = obj_inc - obj_margin * scale;       // two roundings, as the rule reads in numpy
  return obj < bar;
}

// Start row of candidate k of instance b, layout z = [vec(U); vec(X)]: U[c, i] = controls[k][c] at every stage, X[:, j] = x0[b] at every
// node (with cfg.init_rollout the solve rolls X out itself; without it the start is finite and the dynamic model's vx is x0's).  With a
// caller start, candidate 0 is that row verbatim.
MPCB_DEVFN void expand(const MpcbMultiArgs& a_in, const int e) {
  const MpcbMultiArgs& a = *wv::late_args(a_in);
  const int K = a.K, b = e / K, k = e - b * K, lane = wv::lane();
  const int nx = a.nx, nz = a.nz, nu2 = 2 * a.N;
  double* zr = a.z0_e + (size_t)e * nz;
  if (k == 0 && a.z0) {
    copy_row(zr, a.z0 + (size_t)b * nz, nz, lane);
  } else {
    const double c0 = a.controls[2 * k], c1 = a.controls[2 * k + 1];
    const double* xb = a.x0 + (size_t)b * nx;
    for (int i = lane; i < nz; i += 64) {
      double v;
      if (i < nu2) v = (i & 1) ? c1 : c0;
      else v = xb[(i - nu2) % nx];
      zr[i] = v;
    }
  }
  copy_row(a.x0_e + (size_t)e * nx, a.x0 + (size_t)b * nx, nx, lane);
  copy_row(a.xs_e + (size_t)e * nx, a.xs + (size_t)b * nx, nx, lane);
  if (a.obs_row > 0) copy_row(a.obs_e + (size_t)e * a.obs_row, a.obs + (size_t)b * a.obs_row, a.obs_row, lane);
}

// The selection rule (every decision is wave-uniform: all lanes read the same status and objective words):
//   walk k = 0..K-1; the first eligible candidate is the incumbent; a later eligible one replaces it only if
//   obj_k < obj_inc - obj_margin * max(1, |obj_inc|).  No eligible candidate: the winner is candidate 0, with its failure status.
//   n_ok = eligible candidates.  n_basins = distinct solutions: an eligible candidate is a new representative when
//   max_i |z_k[i] - z_r[i]| > basin_tol for every earlier representative r.
MPCB_DEVFN void select(const MpcbMultiArgs& a_in, const int b) {
  const MpcbMultiArgs& a = *wv::late_args(a_in);
  const int K = a.K, nz = a.nz, ng = a.ng, lane = wv::lane();
  const size_t e0 = (size_t)b * K;
  const double margin = a.obj_margin, tol = a.basin_tol;
  int win = -1, n_ok = 0, n_basins = 0;
  unsigned reps = 0;                      // bit r: candidate r represents a solution of its own
  double obj_inc = 0.0;
  for (int k = 0; k < K; ++k) {
    const int st = a.status_all[e0 + k];
    const double f = a.obj_all[e0 + k];
    if (!eligible(st, f)) continue;
    ++n_ok;
    if (win < 0 || replaces(f, obj_inc, margin)) { win = k; obj_inc = f; }
    // a new solution, or one an earlier representative stands for already?  The walk ends at the first representative within basin_tol.
    const double* zk = a.z_all + (e0 + k) * nz;
    bool fresh = true;
    for (int r = 0; r < k; ++r) {
      if (!((reps >> r) & 1u)) continue;
      const double* zr = a.z_all + (e0 + r) * nz;
      double d = 0.0;
      for (int i = lane; i < nz; i += 64) d = fmax(d, fabs(zk[i] - zr[i]));
      d = wv::max(d);
      if (!(d > tol)) { fresh = false; break; }
    }
    if (fresh) { reps |= 1u << k; ++n_basins; }
  }
  const int w = win < 0 ? 0 : win;
  const size_t ew = e0 + w;
  copy_row(a.z + (size_t)b * nz, a.z_all + ew * nz, nz, lane);
  if (a.lam_g) copy_row(a.lam_g + (size_t)b * ng, a.lam_g_all + ew * ng, ng, lane);
  if (a.lam_x) copy_row(a.lam_x + (size_t)b * nz, a.lam_x_all + ew * nz, nz, lane);
  if (a.kkt) copy_row(a.kkt + (size_t)b * 4, a.kkt_all + ew * 4, 4, lane);
  if (lane == 0) {
    if (a.obj) a.obj[b] = a.obj_all[ew];
    if (a.status) a.status[b] = a.status_all[ew];
    if (a.iters) a.iters[b] = a.iters_all[ew];
    if (a.which) a.which[b] = w;
    if (a.n_ok) a.n_ok[b] = n_ok;
    if (a.n_basins) a.n_basins[b] = n_basins;
  }
}

}  // namespace mpcbm
