// mpcb_plant.h — what the closed loop does to ONE instance between two solves: which plan is executed (the hold rule), the shift of that
// plan into the next warm start, the plant step with the first control, the obstacle move.  Plain C++ behind MPCB_HD / MPCB_DEV, no wave
// primitives: one thread per instance on the device (mpcb_advance, mpcb_loop_commit, mpcb_loop_plant in mpcb_api.hip are index arithmetic
// around these functions), a plain loop over the instances on the host (tests/emu/wave_emu.cpp compiles this header unchanged).  The
// model expressions of the plant, the shift loops and the hold rule are stated here and nowhere else.
//   main_cbf_kin_c_sim.py:16-26 / main_cbf_dyn_c_sim.py:15-25 (shift_movement), main_cbf_kin_c_sim_pre.py:106 (obstacle advance)
//
// (The solve and evaluation kernels have model expressions of their own, mpcb_kernel*.h / mpcb_eval.h: other forms, with FMA and
// derivatives.)
#pragma once

#include "../../include/mpcbatch.h"
#include "mpcb_wave.h"     // MPCB_HD, MPCB_DEV

#include <cmath>
#include <type_traits>

// Every product and sum of this header is rounded on its own, as numpy / CasADi evaluate the reference's expressions: st = x0 + T*f and
// x += v*cos(theta)*dt are then bit-equal to the reference's helpers.  (The host compiler of tests/emu gets -ffp-contract=off.)
#ifdef __clang__
#define MPCB_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MPCB_NO_CONTRACT
#endif

namespace mpcbp {

// Run-time nx -> compile-time NX, in the style of mpcbd::visit: f(std::integral_constant<int, NX>{}), returns what f returns.
template <class F>
auto visit_nx(int nx, F&& f) { return nx == 6 ? f(std::integral_constant<int, 6>{}) : f(std::integral_constant<int, 4>{}); }

// f(x,u) of the model: the reference's `mpc_solver.f` (kin.py:153-159, dyn.py:156-177).  The model is fixed at compile time by NX
// (4: kinematic, 6: dynamic): with the model a run-time branch the compiler indexes xdot[] dynamically and parks it in scratch.
template <int NX>
MPCB_HD void model_rhs(const mpcb_config& c, const double* x, const double* u, double* xdot) {
  MPCB_NO_CONTRACT
  static_assert(NX == 4 || NX == 6, "NX is 4 (kinematic) or 6 (dynamic)");
  if constexpr (NX == 4) {                               // kin.py:153-156
    xdot[0] = x[3] * cos(x[2]);
    xdot[1] = x[3] * sin(x[2]);
    xdot[2] = x[3] * tan(u[0]) / c.veh_l;
    xdot[3] = u[1];
  } else {                                               // dyn.py:156-170
    const double phi = x[2], vx = x[3], vy = x[4], r = x[5], df = u[0], ax = u[1];
    const double af = df - (vy + c.veh_lf * r) / vx, ar = -(vy - c.veh_lr * r) / vx;
    const double Cf = c.Fymax_f * 2 * c.aopt_f / (c.aopt_f * c.aopt_f + af * af);
    const double Cr = c.Fymax_r * 2 * c.aopt_r / (c.aopt_r * c.aopt_r + ar * ar);
    const double Fcf = -Cf * af, Fcr = -Cr * ar;
    xdot[0] = vx * cos(phi) - vy * sin(phi);
    xdot[1] = vx * sin(phi) + vy * cos(phi);
    xdot[2] = r;
    xdot[3] = ax + r * vy;
    xdot[4] = -r * vx + 2.0 / c.veh_m * (Fcf * cos(df) + Fcr);
    xdot[5] = 2.0 / c.veh_Iz * (c.veh_lf * Fcf - c.veh_lr * Fcr);
  }
}

// x <- x + T * slope with the control held: st = x0 + T f(x0, u) (Euler), or the plant follows the NLP's integrator with a classical
// RK4 step (T times the weighted slope).  T is the length of the executed step (cfg.T, or T_0 of the time grid).
// NX is a template parameter so that x[] and the slopes live in registers: constant indices after unrolling.
template <int NX>
MPCB_DEV void plant_step(const mpcb_config& c, const double T, const double* u, double* x) {
  MPCB_NO_CONTRACT
  double f[NX];
  model_rhs<NX>(c, x, u, f);
  if (c.integrator == MPCB_INT_RK4) {
    double k2[NX], k3[NX], k4[NX], xt[NX];
#pragma unroll
    for (int q = 0; q < NX; ++q) xt[q] = x[q] + 0.5 * T * f[q];
    model_rhs<NX>(c, xt, u, k2);
#pragma unroll
    for (int q = 0; q < NX; ++q) xt[q] = x[q] + 0.5 * T * k2[q];
    model_rhs<NX>(c, xt, u, k3);
#pragma unroll
    for (int q = 0; q < NX; ++q) xt[q] = x[q] + T * k3[q];
    model_rhs<NX>(c, xt, u, k4);
#pragma unroll
    for (int q = 0; q < NX; ++q) f[q] = (f[q] + 2.0 * k2[q] + 2.0 * k3[q] + k4[q]) / 6.0;
  }
#pragma unroll
  for (int q = 0; q < NX; ++q) x[q] = x[q] + T * f[q];
}

// a step whose solve ended neither solved nor acceptable counts as failed
MPCB_HD bool step_failed(int status) { return status != MPCB_ST_SOLVED && status != MPCB_ST_ACCEPTABLE; }

// The plan a step executes: this step's solution z, or (hold) after a failed solve the previous plan.  The warm start w IS that plan,
// already moved one stage: hold-and-shift, prior art `reference code/MPC-D-CBF.py:341-353`.
MPCB_HD const double* executed_plan(int hold, int status, const double* z, const double* w) {
  const bool keep = hold && step_failed(status);
  return keep ? w : z;
}

// w <- the plan moved one stage: u <- [u[1:]; u[-1]], x <- [x[1:]; x[-1]] on [vec(U); vec(X)].  Ascending, so that it is right in
// place (plan == w, a held plan): every read is ahead of the writes.
template <int NX>
MPCB_DEV void shift_plan(int N, const double* plan, double* w) {
  for (int i = 0; i < N; ++i) { int s = (i + 1 < N) ? i + 1 : N - 1; const double a0 = plan[2 * s], a1 = plan[2 * s + 1]; w[2 * i] = a0; w[2 * i + 1] = a1; }
  for (int i = 0; i <= N; ++i) {
    int s = (i + 1 <= N) ? i + 1 : N;
    double t[NX];
#pragma unroll
    for (int q = 0; q < NX; ++q) t[q] = plan[2 * N + NX * s + q];
#pragma unroll
    for (int q = 0; q < NX; ++q) w[2 * N + NX * i + q] = t[q];
  }
}

// The controller's half of a step: u <- the first control of the executed plan, w <- that plan shifted.  Returns whether the step failed.
template <int NX>
MPCB_DEV bool commit(int N, int hold, int status, const double* z, double* w, double* u) {
  const double* plan = executed_plan(hold, status, z, w);
  u[0] = plan[0]; u[1] = plan[1];
  shift_plan<NX>(N, plan, w);
  return step_failed(status);
}

// obs [n_obs, 6] of one instance one step on with constant velocity and heading (Obs_prediction.py:27-30).
//   move_obs: 0 none, 1 every obstacle, 2 only the first one (what main_cbf_kin_c_sim_pre.py:106 does)
MPCB_DEV void move_obstacles(int n_obs, int move_obs, const double T, double* obs) {
  MPCB_NO_CONTRACT
  const int nmove = move_obs == 1 ? n_obs : move_obs == 2 ? (n_obs < 1 ? n_obs : 1) : 0;
  for (int j = 0; j < nmove; ++j) {
    double* o = obs + (size_t)j * 6;
    o[0] += o[3] * cos(o[2]) * T; o[1] += o[3] * sin(o[2]) * T;
  }
}

// The plant's half of a step: x [NX] <- the plant step with u, obs [n_obs, 6] <- the obstacle move (obs is not read when nothing moves).
template <int NX>
MPCB_DEV void plant(const mpcb_config& c, const double T, const double* u, int move_obs, double* x, double* obs) {
  const double ul[2] = {u[0], u[1]};
  double xl[NX];
#pragma unroll
  for (int q = 0; q < NX; ++q) xl[q] = x[q];
  plant_step<NX>(c, T, ul, xl);
#pragma unroll
  for (int q = 0; q < NX; ++q) x[q] = xl[q];
  move_obstacles(c.n_obs, move_obs, T, obs);
}

}  // namespace mpcbp
