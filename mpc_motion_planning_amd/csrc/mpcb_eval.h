// mpcb_eval.h — evaluate the NLP at any point: objective, constraint vector, gradient of the Lagrangian and the KKT residuals.
//
// What it states: the NLP of CasaDi_MPC_Optimize_Multishoot/MPC_CBF_optimize_kin.py:136-255 (and _dyn.py) in the library's own row form
// and order, the one lam_g of mpcb_solve refers to (include/mpcbatch.h): g = [X_0 - x0; shooting rows X_{i+1} - F(X_i, U_i); rate rows
// U[c,i] - U[c,i-1]; obstacle rows], obstacle rows h on both models or gamma h_i(X_i) + h_i(X_{i+1}) - h_i(X_i).  Nothing of the solver's
// scaling, slacks or elimination enters: the point may come from anywhere (a solve, a held plan, a warm start, a learned policy).
//
// One wavefront per instance, lane k = node k (k = 0..N <= 63) as in the solve kernels, but with no serial sweep: lane k needs X_k, U_k,
// X_{k+1}, U_{k-1}, U_{k+1}, the multipliers of its own rows and of the rows of stage k-1 that read X_k.  The rows of z, lam_g and lam_x are
// read coalesced into LDS, the rows of g and grad_lag leave through LDS the same way.  The structure (n_obs, row mode, gamma,
// obs_terminal, rate_interleaved, which rate rows exist, integrator, du0_cost) is wave-uniform and read from the config at run time:
// there is one instantiation per model and per source of the config (the handle's, or row b of a parameter set), not one per structure.
//
// Written against mpcb_wave.h like the solve functions, so tests/emu_eval steps exactly this code on the CPU.
#pragma once

#include "mpcb_kernel_dyn.h"

// An argument struct of its own: MpcbKArgs keeps its layout.  Every eval kernel takes ONE argument, a MpcbEvalArgs by value (wv::late_args).
struct MpcbEvalArgs {
  mpcb_config cfg;            // the handle's config
  const mpcb_config* cfgs;    // [B] rows of a parameter set (PARAMS kernels), NULL elsewhere
  int32_t B, nz, ng, obs_kind;
  const double *x0, *xs, *xref, *obs, *z;    // xref: [B][N][4] per-stage reference of the tracking objective, NULL = xs
  const double *lam_g, *lam_x;               // both or neither
  double *obj, *g, *grad, *res;              // each may be NULL; grad only with multipliers
};

namespace mpcbk {

// LDS of one instance (doubles): the staged rows z, lam_x [nz], lam_g [ng] and the rows that leave, g [ng] and grad_lag [nz]
struct EvalLayout { int z, lx, lg, g, gl, total; };
MPCB_HD EvalLayout layout_eval(int nz, int ng) {
  EvalLayout L;
  int o = 0;
  L.z = o; o += nz;
  L.lx = o; o += nz;
  L.lg = o; o += ng;
  L.g = o; o += ng;
  L.gl = o; o += nz;
  L.total = o;
  return L;
}

// Running maximum / minimum that KEEP a NaN: fmax and fmin (v_max_f64, v_min_f64) return the operand that is a number, so a residual
// accumulated with them would read 0 at a point that holds a NaN, and such a point would pass every gate.  A certificate must fail
// there: once a NaN has been seen in a column, the column is NaN (numpy's maximum() and max() behave the same way).
MPCB_DEV double nanmax(double m, double x) { return (x > m || x != x) ? x : m; }
MPCB_DEV double nanmin(double m, double x) { return (x < m || x != x) ? x : m; }

// One entry of (lam, v, lo, hi) in the complementarity and the sign check of oracle/kkt_check.certificate's inner compl(): rows with
// lo == hi count nothing; lam > 0 is measured against the upper bound, everything else against the lower one; a distance to a
// non-finite bound counts nothing in cmax and the multiplier itself in smax.  A NaN multiplier or value makes both columns NaN, on
// equality rows too (kkt_check's nan_to_num would count it as zero: the one place where this differs from it, toward failing).
MPCB_DEV void kkt_item(double lam, double v, double lo, double hi, double& cmax, double& smax) {
  if (lam != lam || v != v) { cmax = lam + v; smax = lam + v; return; }
  if (lo == hi) return;
  const bool fhi = isfinite(hi), flo = isfinite(lo);
  double cc = lam > 0.0 ? (fhi ? lam * fmax(hi - v, 0.0) : 0.0) : (flo ? -lam * fmax(v - lo, 0.0) : 0.0);
  if (!isfinite(cc)) cc = 0.0;                        // (+inf: an infinite value against a finite bound; kkt_check: posinf = 0)
  cmax = nanmax(cmax, cc);
  double ws = 0.0;
  if (lam > 0.0 && !fhi) ws += lam;
  if (lam < 0.0 && !flo) ws += -lam;
  smax = nanmax(smax, ws);
}
MPCB_DEV double viol(double v, double lo, double hi) { return nanmax(0.0, nanmax(lo - v, v - hi)); }

}  // namespace mpcbk

// res columns: see MPCB_EVAL_COLS in include/mpcbatch.h
template <int NX, bool PARAMS>
MPCB_DEVFN void mpcb_eval(const MpcbEvalArgs& a_in, const int b, double* lds) {
  using namespace mpcbk;
  static_assert(NX == 4 || NX == 6, "kinematic (4 states) or dynamic (6 states) bicycle");
  constexpr bool DYN = NX == 6;
  const MpcbEvalArgs& a = *wv::late_args(a_in);
  const mpcb_config* cp_ = &a.cfg;
  if constexpr (PARAMS) cp_ = wv::late_row(a.cfgs, b);           // row b of the parameter set: uniform, constant address space
  const mpcb_config& c = *cp_;
  const int N = c.N, k = wv::lane(), nobs = c.n_obs, nz = a.nz, ng = a.ng;
  const bool mult = a.lam_g != nullptr && a.lam_x != nullptr;
  const bool isnode = k <= N, hasu = k < N;
  const double T = wv::uni(c.T);
  const EvalLayout L = layout_eval(nz, ng);
  double *zb = lds + L.z, *lxb = lds + L.lx, *lgb = lds + L.lg, *gb = lds + L.g, *glb = lds + L.gl;

  // ----- the rows of the instance (coalesced) -> LDS; lam_scale on the way ------------------------------------------------------
  double lmax = 1.0;
  for (int i = k; i < nz; i += 64) {
    zb[i] = a.z[(size_t)b * nz + i];
    const double l = mult ? a.lam_x[(size_t)b * nz + i] : 0.0;
    lxb[i] = l; lmax = nanmax(lmax, fabs(l)); glb[i] = 0.0;
  }
  for (int i = k; i < ng; i += 64) {
    const double l = mult ? a.lam_g[(size_t)b * ng + i] : 0.0;
    lgb[i] = l; lmax = nanmax(lmax, fabs(l)); gb[i] = 0.0;
  }
  wv::sync();

  // ----- row pattern (wave-uniform) ------------------------------------------------------------------------------------------------
  const bool rate0 = c.du_lo[0] > -1e300 || c.du_hi[0] < 1e300, rate1 = c.du_lo[1] > -1e300 || c.du_hi[1] < 1e300;   // mk_bnd's predicate
  const int nrate = (rate0 ? 1 : 0) + (rate1 ? 1 : 0);
  const bool inter = c.rate_interleaved != 0;
  const bool dcbf = c.obs_mode == MPCB_OBS_DCBF;
  const int obs_nodes = (c.obs_terminal && !dcbf) ? N + 1 : N;
  const int r_obs = NX * (N + 1) + nrate * (N - 1);
  // first shooting row of stage i; rate row of stage i (1..N-1) and rate slot ci
  auto shoot_row = [&](int i) { return NX + NX * i + (inter ? nrate * (i > 1 ? i - 1 : 0) : 0); };
  auto rate_row = [&](int i, int ci) { return inter ? shoot_row(i) + NX + ci : NX + NX * N + (i - 1) * nrate + ci; };

  // ----- this node ------------------------------------------------------------------------------------------------------------------
  double X[NX], Xn[NX], U[NU], Up[NU], Un[NU], gX[NX], gU[NU];
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    X[i] = isnode ? zb[NU * N + NX * k + i] : 0.0;
    Xn[i] = hasu ? zb[NU * N + NX * (k + 1) + i] : 0.0;
    gX[i] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    U[i] = hasu ? zb[NU * k + i] : 0.0;
    Up[i] = k == 0 ? c.u_last[i] : (k <= N ? zb[NU * (k - 1) + i] : 0.0);
    Un[i] = k + 1 < N ? zb[NU * (k + 1) + i] : 0.0;
    gU[i] = 0.0;
  }
  double feas_g = 0.0, feas_x = 0.0, cmax = 0.0, smax = 0.0, hmin = __builtin_inf(), f = 0.0;
  // one row of g: its value to LDS, its violation, complementarity and sign; returns its multiplier
  auto row = [&](int r, double v, double lo, double hi) -> double {
    if (r < 0 || r >= ng) return 0.0;
    gb[r] = v;
    feas_g = nanmax(feas_g, viol(v, lo, hi));
    const double l = lgb[r];
    if (mult) kkt_item(l, v, lo, hi, cmax, smax);
    return l;
  };

  // ----- objective and its gradient (kin.py:195-205; tracking: r_i in place of xs) --------------------------------------------------
  if (hasu) {
    const double* ref = a.xref ? a.xref + ((size_t)b * N + k) * NX : a.xs + (size_t)b * NX;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const double e = X[i] - ref[i];
      f += e * e * c.Q[i];
      gX[i] = 2.0 * c.Q[i] * e;
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      f += U[i] * U[i] * c.R[i];
      double gu = 2.0 * c.R[i] * U[i];
      if (k > 0 || c.du0_cost) { const double d = U[i] - Up[i]; f += d * d * c.DR[i]; gu += 2.0 * c.DR[i] * d; }
      if (k + 1 < N) gu -= 2.0 * c.DR[i] * (Un[i] - U[i]);
      gU[i] = gu;
    }
  }

  // ----- boxes on the variables: violation, complementarity, sign; lam_x into the gradient -----------------------------------------
  if (isnode) {
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const double lo = c.x_lo[i], hi = c.x_hi[i], l = lxb[NU * N + NX * k + i];
      feas_x = nanmax(feas_x, viol(X[i], lo, hi));
      if (mult) kkt_item(l, X[i], lo, hi, cmax, smax);
      gX[i] += l;
    }
  }
  if (hasu) {
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const double lo = c.u_lo[i], hi = c.u_hi[i], l = lxb[NU * k + i];
      feas_x = nanmax(feas_x, viol(U[i], lo, hi));
      if (mult) kkt_item(l, U[i], lo, hi, cmax, smax);
      gU[i] += l;
    }
  }

  // ----- X_0 rows ---------------------------------------------------------------------------------------------------------------------
  if (k == 0) {
#pragma unroll
    for (int i = 0; i < NX; ++i) gX[i] += row(i, X[i] - a.x0[(size_t)b * NX + i], 0.0, 0.0);
  }
  // ----- shooting rows of stage k: X_{k+1} - F(X_k, U_k); -A' mu_k and -B' mu_k here, + mu_{k-1} on X_k ---------------------------
  if (k >= 1 && isnode) {
    const int r = shoot_row(k - 1);
#pragma unroll
    for (int i = 0; i < NX; ++i) gX[i] += lgb[r + i];
  }
  if (hasu) {
    const int r = shoot_row(k);
    double F[NX], m[NX];
    if constexpr (DYN) {
      DynEval e; dyn_eval(c, X, U, e);
      dyn_F(c, T, X, U, e, F);
#pragma unroll
      for (int i = 0; i < NX; ++i) m[i] = row(r + i, Xn[i] - F[i], 0.0, 0.0);
      DynJac J; dyn_jac(c, T, X, e, J);
      gX[0] -= m[0];
      gX[1] -= m[1];
      gX[2] -= J.a02 * m[0] + J.a12 * m[1] + m[2];
      gX[3] -= J.a03 * m[0] + J.a13 * m[1] + m[3] + J.a43 * m[4] + J.a53 * m[5];
      gX[4] -= J.a04 * m[0] + J.a14 * m[1] + J.a34 * m[3] + J.a44 * m[4] + J.a54 * m[5];
      gX[5] -= T * m[2] + J.a35 * m[3] + J.a45 * m[4] + J.a55 * m[5];
      gU[0] -= J.b4 * m[4] + J.b5 * m[5];
      gU[1] -= T * m[3];
    } else {
      const double il = 1.0 / c.veh_l;
      double sp, cp, sd, cd;
      sincos_b(X[2], sp, cp); sincos_b(U[0], sd, cd);
      const double icd = wv::rcp(cd), td = sd * icd, sec2 = icd * icd;
      KinRkJac J{};
      const bool rk4 = c.integrator == MPCB_INT_RK4;
      if (rk4) {
        kin_rk4_step(X, U, T, il, sp, cp, td, F);
      } else {
        F[0] = X[0] + T * (X[3] * cp); F[1] = X[1] + T * (X[3] * sp); F[2] = X[2] + T * (X[3] * td * il); F[3] = X[3] + T * U[1];
      }
#pragma unroll
      for (int i = 0; i < NX; ++i) m[i] = row(r + i, Xn[i] - F[i], 0.0, 0.0);
      if (rk4) {
        KinRkHess H{}; kin_rk4_derivs(X, U, T, il, sp, cp, td, sec2, m, J, H);
      } else {
        J.a02 = -T * X[3] * sp; J.a03 = T * cp; J.a12 = T * X[3] * cp; J.a13 = T * sp; J.a23 = T * td * il;
        J.b00 = 0.0; J.b01 = 0.0; J.b10 = 0.0; J.b11 = 0.0; J.b20 = T * X[3] * sec2 * il; J.b21 = 0.0;
      }
      gX[0] -= m[0];
      gX[1] -= m[1];
      gX[2] -= J.a02 * m[0] + J.a12 * m[1] + m[2];
      gX[3] -= J.a03 * m[0] + J.a13 * m[1] + J.a23 * m[2] + m[3];
      gU[0] -= J.b00 * m[0] + J.b10 * m[1] + J.b20 * m[2];
      gU[1] -= J.b01 * m[0] + J.b11 * m[1] + J.b21 * m[2] + T * m[3];
    }
  }
  // ----- rate rows U[c,k] - U[c,k-1], k = 1..N-1: + rho_k - rho_{k+1} on U_k ------------------------------------------------------------
  {
    int ci = 0;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const bool on = i == 0 ? rate0 : rate1;
      if (on) {
        if (k >= 1 && k <= N - 1) gU[i] += row(rate_row(k, ci), U[i] - Up[i], c.du_lo[i], c.du_hi[i]);
        if (k + 1 <= N - 1) gU[i] -= lgb[rate_row(k + 1, ci)];
        ++ci;
      }
    }
  }
  // ----- obstacle rows; h_min over every node with that node's obstacle row, whatever the row mode -------------------------------
  if (nobs > 0 && isnode) {
    const double gam = c.gamma, hlo = dcbf ? c.obs_hmin * gam : c.obs_hmin;
    const bool pred = a.obs_kind == MPCB_OBSIN_PREDICTED;
    for (int j = 0; j < nobs; ++j) {
      const double* q = pred ? a.obs + (((size_t)b * nobs + j) * (N + 1) + k) * 6 : a.obs + ((size_t)b * nobs + j) * 6;
      const double sx = c.obs_sx_fixed > 0 ? c.obs_sx_fixed : c.ego_hl + q[4] / 2 + c.safe_disl;
      const double sy = c.obs_sy_fixed > 0 ? c.obs_sy_fixed : c.ego_hw + q[5] / 2 + c.safe_disw;
      const double ix2 = 1.0 / (sx * sx), iy2 = 1.0 / (sy * sy);
      const double dx = X[0] - q[0], dy = X[1] - q[1];
      const double hi = dx * dx * ix2 + dy * dy * iy2 - 1.0;
      hmin = nanmin(hmin, hi);
      if (k < obs_nodes) {
        const int r = r_obs + k * nobs + j;
        if (!dcbf) {
          const double nu = row(r, hi, hlo, __builtin_inf());
          gX[0] += nu * (2.0 * dx * ix2); gX[1] += nu * (2.0 * dy * iy2);
        } else {
          const double dxn = Xn[0] - q[0], dyn_ = Xn[1] - q[1];
          const double hn = dxn * dxn * ix2 + dyn_ * dyn_ * iy2 - 1.0;
          const double nu = row(r, gam * hi + (hn - hi), hlo, __builtin_inf());
          const double hx = 2.0 * dx * ix2, hy = 2.0 * dy * iy2;
          gX[0] += nu * (gam * hx - hx); gX[1] += nu * (gam * hy - hy);
        }
      }
      if (dcbf && k >= 1) {        // row k-1 reads h of ITS obstacle row at X_k
        const double* p = pred ? q - 6 : q;
        const double sxp = c.obs_sx_fixed > 0 ? c.obs_sx_fixed : c.ego_hl + p[4] / 2 + c.safe_disl;
        const double syp = c.obs_sy_fixed > 0 ? c.obs_sy_fixed : c.ego_hw + p[5] / 2 + c.safe_disw;
        const int r = r_obs + (k - 1) * nobs + j;
        const double nu = (r >= 0 && r < ng) ? lgb[r] : 0.0;
        gX[0] += nu * (2.0 * (X[0] - p[0]) / (sxp * sxp)); gX[1] += nu * (2.0 * (X[1] - p[1]) / (syp * syp));
      }
    }
  }

  // ----- gradient of the Lagrangian -> LDS; the reductions ----------------------------------------------------------------------------
  double stat = 0.0;
  if (isnode) {
#pragma unroll
    for (int i = 0; i < NX; ++i) { glb[NU * N + NX * k + i] = gX[i]; stat = nanmax(stat, fabs(gX[i])); }
  }
  if (hasu) {
#pragma unroll
    for (int i = 0; i < NU; ++i) { glb[NU * k + i] = gU[i]; stat = nanmax(stat, fabs(gU[i])); }
  }
  // the wave's maxima: wv::reduce combines with fmax, which drops a NaN, so every column travels as (value with NaN taken out, "saw a NaN")
  double s[1] = {f}, mx[14] = {feas_g, feas_x, -hmin, stat, cmax, smax, lmax, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 7; ++i) if (mx[i] != mx[i]) { mx[i] = 0.0; mx[7 + i] = 1.0; }
  wv::reduce<1, 14>(s, mx);
#pragma unroll
  for (int i = 0; i < 7; ++i) if (mx[7 + i] != 0.0) mx[i] = __builtin_nan("");
  wv::sync();
  if (a.g) for (int i = k; i < ng; i += 64) a.g[(size_t)b * ng + i] = gb[i];
  if (a.grad && mult) for (int i = k; i < nz; i += 64) a.grad[(size_t)b * nz + i] = glb[i];
  if (k == 0) {
    if (a.obj) a.obj[b] = s[0];
    if (a.res) {
      const double nan_ = __builtin_nan("");
      double* q = a.res + (size_t)b * MPCB_EVAL_COLS;
      q[0] = mx[0]; q[1] = mx[1]; q[2] = -mx[2];
      q[3] = mult ? mx[3] : nan_; q[4] = mult ? mx[4] : nan_; q[5] = mult ? mx[5] : nan_; q[6] = mult ? mx[6] : nan_;
    }
  }
}
