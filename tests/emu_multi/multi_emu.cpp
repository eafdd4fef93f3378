// tests/emu_multi/multi_emu.cpp — TEST INFRASTRUCTURE ONLY.
//
// Steps the device source mpc_motion_planning_amd/csrc/mpcb_multi.h on the CPU, as tests/emu_eval steps mpcb_eval.h: every lane of the
// wavefront is a host thread, the cross-lane primitives (mpcb_wave.h, MPCB_WAVE_EMU branch) go through a barrier.  The 64 lane threads
// are started once per call and walk the grid together, one "workgroup" after the other.  The kernels use no LDS, so there is none here.
// It is NOT part of libmpcbatch.so and is never loaded by the mpc_motion_planning_amd package.
#define MPCB_WAVE_EMU 1
#include "../../mpc_motion_planning_amd/csrc/mpcb_multi.h"

#include <thread>
#include <vector>

namespace wv {
thread_local int t_lane = 0;
thread_local Emu* t_emu = nullptr;
}

// f(a, block) for block = 0..grid-1 on 64 lanes
template <class F>
static void run_grid(const MpcbMultiArgs& a, int grid, F f) {
  std::barrier<> bar(64);
  wv::Emu emu; emu.bar = &bar;
  std::vector<std::thread> th;
  for (int l = 0; l < 64; ++l)
    th.emplace_back([&, l]() {
      wv::t_lane = l; wv::t_emu = &emu;
      for (int blk = 0; blk < grid; ++blk) { f(a, blk); wv::sync(); }
    });
  for (auto& t : th) t.join();
}

// The arguments of the two kernels as mpcb_api.hip fills them (MpcbMultiArgs), flat.  controls: [K, 2] or NULL (K = 1 with z0).
extern "C" int mpcb_emu_multi_expand(int32_t B, int32_t K, int32_t N, int32_t nx, int32_t nz, int32_t obs_row, const double* x0, const double* xs,
                                     const double* obs, const double* z0, const double* controls, double* x0_e, double* xs_e, double* obs_e,
                                     double* z0_e) {
  if (B < 0 || K < 1 || K > MPCB_MULTI_MAX || !x0 || !xs || !x0_e || !xs_e || !z0_e || (obs_row > 0 && (!obs || !obs_e))) return MPCB_E_INVALID;
  if (!controls && !(K == 1 && z0)) return MPCB_E_INVALID;
  MpcbMultiArgs a{};
  a.B = B; a.K = K; a.N = N; a.nx = nx; a.nz = nz; a.obs_row = obs_row;
  if (controls) for (int i = 0; i < 2 * K; ++i) a.controls[i] = controls[i];
  a.x0 = x0; a.xs = xs; a.obs = obs; a.z0 = z0; a.x0_e = x0_e; a.xs_e = xs_e; a.obs_e = obs_e; a.z0_e = z0_e;
  run_grid(a, B * K, [](const MpcbMultiArgs& q, int e) { mpcbm::expand(q, e); });
  return MPCB_OK;
}

extern "C" int mpcb_emu_multi_select(int32_t B, int32_t K, int32_t nz, int32_t ng, double obj_margin, double basin_tol, const double* z_all,
                                     const double* obj_all, const double* kkt_all, const double* lam_g_all, const double* lam_x_all,
                                     const int32_t* status_all, const int32_t* iters_all, double* z, double* obj, double* kkt, double* lam_g,
                                     double* lam_x, int32_t* status, int32_t* iters, int32_t* which, int32_t* n_ok, int32_t* n_basins) {
  if (B < 0 || K < 1 || K > MPCB_MULTI_MAX || !z_all || !obj_all || !status_all || !z) return MPCB_E_INVALID;
  if ((kkt && !kkt_all) || (lam_g && !lam_g_all) || (lam_x && !lam_x_all) || (iters && !iters_all)) return MPCB_E_INVALID;
  MpcbMultiArgs a{};
  a.B = B; a.K = K; a.nz = nz; a.ng = ng; a.obj_margin = obj_margin; a.basin_tol = basin_tol;
  a.z_all = z_all; a.obj_all = obj_all; a.kkt_all = kkt_all; a.lam_g_all = lam_g_all; a.lam_x_all = lam_x_all;
  a.status_all = status_all; a.iters_all = iters_all;
  a.z = z; a.obj = obj; a.kkt = kkt; a.lam_g = lam_g; a.lam_x = lam_x; a.status = status; a.iters = iters;
  a.which = which; a.n_ok = n_ok; a.n_basins = n_basins;
  run_grid(a, B, [](const MpcbMultiArgs& q, int b) { mpcbm::select(q, b); });
  return MPCB_OK;
}
