// tests/emu_params/params_emu.cpp — TEST INFRASTRUCTURE ONLY.
//
// Steps the PARAMS = true instantiations of mpcb_solve_kin and mpcb_solve_dyn (mpc_motion_planning_amd/csrc, per-instance problem data:
// instance b reads its config from row b of a table) on the CPU the way tests/emu/wave_emu.cpp steps the others: every lane of the
// wavefront is a host thread, cross-lane primitives (mpcb_wave.h, MPCB_WAVE_EMU branch) go through a barrier, and the passes of a
// solve run in the order mpcb_api.hip launches them.  The handle's config (a.cfg) is the caller's `base`; the rows are NOT validated
// here (mpcb_params_check does that).  Never loaded by the mpc_motion_planning_amd package.
#define MPCB_WAVE_EMU 1
#include "../../mpc_motion_planning_amd/csrc/mpcb_kernel_dyn.h"

#include <thread>
#include <limits>
#include <cstdlib>
#include <vector>

namespace wv {
thread_local int t_lane = 0;
thread_local Emu* t_emu = nullptr;
}

template <int NOBS>
static void run_instance(const MpcbKArgs& a, int b) {
  using namespace mpcbk;
  const bool dyn = a.cfg.model == MPCB_MODEL_DYN;
  const bool rp = a.pass == MPCB_PASS_RESTO;
  const int total = dyn ? layout_dyn(a.cfg.N, rp, obs_in_lds(NOBS)).total : layout_kin(a.cfg.N, a.nz, rp, obs_in_lds(NOBS)).total;
  // LDS starts as garbage on the device: NaN here, so that a read of a never-written slot shows
  std::vector<double> lds(total + 64, std::numeric_limits<double>::quiet_NaN());
  std::barrier<> bar(64);
  wv::Emu emu; emu.bar = &bar;
  std::vector<std::thread> th;
  for (int l = 0; l < 64; ++l)
    th.emplace_back([&, l]() {
      wv::t_lane = l; wv::t_emu = &emu;
      if constexpr (NOBS > 0) {
        if (dyn && rp) { mpcb_solve_dyn<NOBS, true, true>(a, b, lds.data(), a.pass); return; }
        if (dyn) { mpcb_solve_dyn<NOBS, false, true>(a, b, lds.data(), a.pass); return; }
      }
      if (rp) mpcb_solve_kin<NOBS, false, true, false, false, true>(a, b, lds.data(), a.pass);
      else mpcb_solve_kin<NOBS, false, false, false, false, true>(a, b, lds.data(), a.pass);
    });
  for (auto& t : th) t.join();
}

extern "C" int mpcb_emu_params_solve(const mpcb_config* base, const mpcb_config* cfgs, int32_t B, const double* x0, const double* xs,
                                     const double* obs, int32_t obs_kind, const double* z0, double* z, double* obj, int32_t* status,
                                     int32_t* iters, double* kkt, double* lam_g, double* lam_x) {
  if (!base || !cfgs) return MPCB_E_INVALID;
  const mpcb_config* cfg = base;
  const bool gen = cfg->model == MPCB_MODEL_KIN && cfg->obs_mode == MPCB_OBS_DCBF && cfg->gamma < 1.0 - 1e-12 && cfg->n_obs > 0;
  if (gen || cfg->integrator != MPCB_INT_EULER || cfg->n_obs > 3) return MPCB_E_UNSUPPORTED;       // as mpcb_params_create
  const int nx = cfg->model == MPCB_MODEL_DYN ? 6 : 4;
  int nrate = 0;
  for (int i = 0; i < 2; ++i) if (cfg->du_lo[i] > -1e300 || cfg->du_hi[i] < 1e300) ++nrate;
  MpcbKArgs a{};
  a.st_stride = 1;
  a.cfg = *cfg; a.cfgs = cfgs; a.B = B; a.obs_kind = obs_kind; a.want_mult = (lam_g || lam_x) ? 1 : 0; a.trace_instance = -1;
  a.nz = 2 * cfg->N + nx * (cfg->N + 1);
  a.ng = nx * (cfg->N + 1) + nrate * (cfg->N - 1) + cfg->n_obs * (cfg->obs_terminal ? cfg->N + 1 : cfg->N);
  a.x0 = x0; a.xs = xs; a.obs = obs; a.z0 = z0; a.z = z; a.obj = obj; a.kkt = kkt; a.lam_g = lam_g; a.lam_x = lam_x;
  a.status = status; a.iters = iters; a.trace = nullptr; a.tgrid = nullptr; a.xref = nullptr;
  std::vector<double> work((size_t)B * mpcbk::WK_SIZE, 0.0);
  const bool second = cfg->second_start && cfg->init_rollout;
  a.work = (cfg->restoration || second) ? work.data() : nullptr;
  // launch order of mpcb_api.hip: first attempt, its restoration pass, second attempt, its restoration pass
  const int order[4] = {MPCB_PASS_FIRST, MPCB_PASS_RESTO, MPCB_PASS_SECOND, MPCB_PASS_RESTO};
  for (int q = 0; q < 4; ++q) {
    const int pass = order[q];
    if ((q >= 2 && !second) || (pass == MPCB_PASS_RESTO && !cfg->restoration)) continue;
    const int ss = cfg->second_start == 3 ? (z0 ? 2 : 1) : cfg->second_start;   // 3: by the kind of start, as mpcb_api.hip
    if (q == 1 && second && ss == 1) continue;      // second start instead of the first attempt's restoration
    a.pass = pass;
    for (int b = 0; b < B; ++b) {
      if (pass == MPCB_PASS_SECOND && (status[b] == MPCB_ST_SOLVED || status[b] == MPCB_ST_ACCEPTABLE || status[b] == MPCB_ST_INFEASIBLE_X0)) continue;
      if (pass == MPCB_PASS_RESTO && status[b] != MPCB_ST_NEEDS_RESTO) continue;
      if (cfg->n_obs == 0) run_instance<0>(a, b);
      else if (cfg->n_obs == 1) run_instance<1>(a, b);
      else run_instance<3>(a, b);
    }
  }
  return MPCB_OK;
}
