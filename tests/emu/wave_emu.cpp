// tests/emu/wave_emu.cpp — TEST INFRASTRUCTURE ONLY.
//
// Steps the device source mpc_motion_planning_amd/csrc/mpcb_kernel.h / mpcb_kernel_dyn.h on the CPU: every lane of the wavefront is a
// host thread, cross-lane primitives (mpcb_wave.h, MPCB_WAVE_EMU branch) go through a barrier.  Which instantiation is stepped, with
// how much LDS and in which order of passes is read from mpcb_dispatch.h, the header mpcb_api.hip launches by: plain, tracking (xref)
// and per-instance (cfgs) solves alike.  It exists so that the kernels' logic can be checked against the oracle in the `-m "not gpu"`
// suite and while developing without a GPU.  It is NOT part of libmpcbatch.so, is never loaded by the mpc_motion_planning_amd package
// and is far too slow to be a fallback (64 OS threads per instance).
#define MPCB_WAVE_EMU 1
#include "../../mpc_motion_planning_amd/csrc/mpcb_kernel_dyn.h"
#include "../../mpc_motion_planning_amd/csrc/mpcb_dispatch.h"
#include "../../mpc_motion_planning_amd/csrc/mpcb_plant.h"

#include <thread>
#include <limits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace wv {
thread_local int t_lane = 0;
thread_local Emu* t_emu = nullptr;
}

constexpr int MPCB_EMU_E_GUARD = -100;      // a word behind the LDS the library allocates at launch was written
constexpr int GUARD = 64;

// the solve function an instantiation tag (mpcbd::Inst) stands for
template <class T> static void solve_as(T, const MpcbKArgs& a, int b, double* lds, int pass) {
  if constexpr (T::model == MPCB_MODEL_DYN) mpcb_solve_dyn<T::nobs, T::resto, T::params>(a, b, lds, pass);
  else mpcb_solve_kin<T::nobs, T::gen, T::resto, T::rk4, T::track, T::params>(a, b, lds, pass);
}

// One workgroup of one launch: instance b from a.pass on; `fused`: the wrapper's loop of the instantiations that fuse (mpcb_api.hip) — an
// instance whose first attempt fails starts its second at once, in the same LDS.  The LDS is exactly the doubles the library passes at
// launch, and starts as garbage on the device: poisoned here (MPCB_EMU_LDS_FILL, default NaN), so that a read of a never-written slot
// shows.  Behind it a guard of NaNs that nothing may write.
static int run_instance(const mpcbd::Variant& v, bool fused, const MpcbKArgs& a, int b) {
  const bool resto = a.pass == MPCB_PASS_RESTO;
  const int total = mpcbd::lds_doubles(v, a.cfg.N, resto);
  const char* fill_env = std::getenv("MPCB_EMU_LDS_FILL");
  std::vector<double> lds(total + GUARD, std::numeric_limits<double>::quiet_NaN());
  if (fill_env) std::fill(lds.begin(), lds.begin() + total, std::atof(fill_env));
  std::barrier<> bar(64);
  wv::Emu emu; emu.bar = &bar;
  const int rc = mpcbd::visit(v, resto, [&](auto inst) {
    std::vector<std::thread> th;
    for (int l = 0; l < 64; ++l)
      th.emplace_back([&, l]() {
        wv::t_lane = l; wv::t_emu = &emu;
        int pass = a.pass;
        for (;;) {
          solve_as(inst, a, b, lds.data(), pass);
          if (!fused || pass != MPCB_PASS_FIRST || !mpcbd::second_kind1(a.cfg, a.z0 != nullptr)) break;
          wv::sync();                                             // the status lane 0 has just stored
          const int st = a.status[b];
          wv::sync();
          if (st == MPCB_ST_SOLVED || st == MPCB_ST_ACCEPTABLE || st == MPCB_ST_INFEASIBLE_X0) break;
          pass = MPCB_PASS_SECOND;
        }
      });
    for (auto& t : th) t.join();
    return MPCB_OK;
  });
  if (rc != MPCB_OK) return rc;
  for (int i = 0; i < GUARD; ++i)
    if (lds[total + i] == lds[total + i]) {
      std::fprintf(stderr, "mpcb_emu: write %d doubles behind the %d doubles of LDS (model %d, capacity %d, gen %d, rk4 %d, track %d, params %d, pass %d)\n",
                   i, total, v.model, v.nobs, v.gen, v.rk4, v.track, v.params, a.pass);
      return MPCB_EMU_E_GUARD;
    }
  return MPCB_OK;
}

// xref: [B, N, 4] per-stage reference, NULL = the set-point solve.  cfgs: [B] per-instance configs (instance b is solved under row b, cfg
// plays the handle's config; the rows are NOT validated here, mpcb_params_check does that), NULL = cfg for every instance.
extern "C" int mpcb_emu_solve(const mpcb_config* cfg, int32_t B, const double* x0, const double* xs, const double* obs,
                              int32_t obs_kind, const double* z0, double* z, double* obj, int32_t* status, int32_t* iters,
                              double* kkt, double* lam_g, double* lam_x, double* trace, int32_t trace_instance, const double* tgrid,
                              const double* xref, const mpcb_config* cfgs) {
  if (!cfg) return MPCB_E_INVALID;
  mpcbd::Variant v;
  { const mpcbd::Refusal r = mpcbd::variant_of(*cfg, xref != nullptr, cfgs != nullptr, &v); if (r.code != MPCB_OK) return r.code; }
  const bool fused = mpcbd::fuses(v);
  const mpcbd::Plan plan = mpcbd::pass_plan(*cfg, z0 != nullptr, fused);
  const int nx = cfg->model == MPCB_MODEL_DYN ? 6 : 4;
  int nrate = 0;
  for (int i = 0; i < 2; ++i) if (cfg->du_lo[i] > -1e300 || cfg->du_hi[i] < 1e300) ++nrate;
  MpcbKArgs a{};
  a.st_stride = 1;
  a.cfg = *cfg; a.cfgs = cfgs; a.B = B; a.obs_kind = obs_kind; a.want_mult = (lam_g || lam_x) ? 1 : 0; a.trace_instance = trace_instance;
  a.nz = 2 * cfg->N + nx * (cfg->N + 1);
  a.ng = nx * (cfg->N + 1) + nrate * (cfg->N - 1) + cfg->n_obs * (cfg->obs_terminal ? cfg->N + 1 : cfg->N);
  a.x0 = x0; a.xs = xs; a.obs = obs; a.z0 = z0; a.z = z; a.obj = obj; a.kkt = kkt; a.lam_g = lam_g; a.lam_x = lam_x;
  a.status = status; a.iters = iters; a.trace = trace; a.tgrid = tgrid; a.xref = xref;
  std::vector<double> work((size_t)B * mpcbk::WK_SIZE, 0.0);
  a.work = mpcbd::multi_pass(*cfg) ? work.data() : nullptr;
  for (int q = 0; q < plan.n; ++q) {
    a.pass = plan.pass[q];
    for (int b = 0; b < B; ++b) {      // (the workgroups that would return at once are not started)
      if (a.pass == MPCB_PASS_SECOND && (status[b] == MPCB_ST_SOLVED || status[b] == MPCB_ST_ACCEPTABLE || status[b] == MPCB_ST_INFEASIBLE_X0)) continue;
      if (a.pass == MPCB_PASS_RESTO && status[b] != MPCB_ST_NEEDS_RESTO) continue;
      const int rc = run_instance(v, fused, a, b);
      if (rc != MPCB_OK) return rc;
    }
  }
  return MPCB_OK;
}

// LDS bytes of one instance (= one workgroup) as the library sizes it at launch: `pass` 0 first pass, 1 restoration pass
extern "C" int64_t mpcb_emu_lds_bytes(const mpcb_config* cfg, int32_t pass) {
  mpcbd::Variant v;
  if (mpcbd::variant_of(*cfg, false, false, &v).code != MPCB_OK) return -1;
  return (int64_t)mpcbd::lds_bytes(v, cfg->N, pass == 1);
}

// The policy of mpcb_dispatch.h for one solve, for tests/test_dispatch_cpu.py.  fused: 0 / 1 plan as if the instantiation did not / did
// fuse, -1 as it does.  out[14]: model, capacity, gen, rk4, track, params, fuses, LDS bytes of the first and of the restoration pass,
// number of passes, the passes.  Returns variant_of's code; `why` (256 bytes) takes its message.
extern "C" int mpcb_emu_dispatch(const mpcb_config* cfg, int32_t track, int32_t params, int32_t start_given, int32_t fused, int64_t* out, char* why) {
  mpcbd::Variant v;
  const mpcbd::Refusal r = mpcbd::variant_of(*cfg, track != 0, params != 0, &v);
  std::snprintf(why, 256, r.fmt, cfg->n_obs);
  if (r.code != MPCB_OK) return r.code;
  const mpcbd::Plan plan = mpcbd::pass_plan(*cfg, start_given != 0, fused < 0 ? mpcbd::fuses(v) : fused != 0);
  const int64_t head[10] = {v.model, v.nobs, v.gen, v.rk4, v.track, v.params, mpcbd::fuses(v), (int64_t)mpcbd::lds_bytes(v, cfg->N, false),
                            (int64_t)mpcbd::lds_bytes(v, cfg->N, true), plan.n};
  for (int i = 0; i < 10; ++i) out[i] = head[i];
  for (int i = 0; i < 4; ++i) out[10 + i] = i < plan.n ? plan.pass[i] : -1;
  return MPCB_OK;
}

// closed-form dyn model derivatives of the kernel source (host-compiled) for comparison with the oracle's AD
extern "C" int mpcb_emu_dyn_model(const mpcb_config* cfg, const double* X, const double* U, const double* lam, double* F, double* jac16,
                                  double* hess13) {
  using namespace mpcbk;
  DynEval e; dyn_eval(*cfg, X, U, e);
  dyn_F(*cfg, cfg->T, X, U, e, F);
  DynJac J; dyn_jac(*cfg, cfg->T, X, e, J);
  const double j[16] = {J.a02, J.a03, J.a04, J.a12, J.a13, J.a14, J.a34, J.a35, J.a43, J.a44, J.a45, J.a53, J.a54, J.a55, J.b4, J.b5};
  for (int i = 0; i < 16; ++i) jac16[i] = j[i];
  DynHess H; dyn_hess(*cfg, cfg->T, X, e, lam, H);
  const double h[13] = {H.h22, H.h23, H.h24, H.h33, H.h34, H.h35, H.h44, H.h45, H.h55, H.h38, H.h48, H.h58, H.h88};
  for (int i = 0; i < 13; ++i) hess13[i] = h[i];
  return 0;
}

// One step of the closed loop between two solves on the host: the per-instance pieces of mpcb_plant.h composed as the kernel mpcb_advance
// composes them (its arguments, status being column `step` of the [B, steps] history), plus what mpcb_loop_commit adds: the executed
// control to u0 [B,2] and the counters.  x_hist, u_hist, u0 and the counters may be NULL; obs may be NULL when nothing moves.
extern "C" int mpcb_emu_advance(const mpcb_config* cfg, const mpcb_config* cfgs, int32_t B, const double* z, double* x0, double* z0, double* obs,
                                double* x_hist, double* u_hist, const int32_t* status, int32_t step, int32_t steps, int32_t move_obs,
                                int32_t hold, double T, double* u0, int32_t* n_steps, int32_t* n_failed) {
  if (!cfg || !z || !x0 || !z0 || !status) return MPCB_E_INVALID;
  return mpcbp::visit_nx(cfg->model == MPCB_MODEL_DYN ? 6 : 4, [&](auto nx) {
    constexpr int NX = decltype(nx)::value;
    const int nz = 2 * cfg->N + NX * (cfg->N + 1);
    for (int b = 0; b < B; ++b) {
      const mpcb_config& c = cfgs ? cfgs[b] : *cfg;
      double* xb = x0 + (size_t)b * NX;
      double u[2];
      const bool failed = mpcbp::commit<NX>(cfg->N, hold, status[(size_t)b * steps + step], z + (size_t)b * nz, z0 + (size_t)b * nz, u);
      mpcbp::plant<NX>(c, T, u, move_obs, xb, obs + (size_t)b * cfg->n_obs * 6);
      if (u_hist) { u_hist[((size_t)b * steps + step) * 2] = u[0]; u_hist[((size_t)b * steps + step) * 2 + 1] = u[1]; }
      if (x_hist) for (int q = 0; q < NX; ++q) x_hist[((size_t)b * (steps + 1) + step + 1) * NX + q] = xb[q];
      if (u0) { u0[(size_t)b * 2] = u[0]; u0[(size_t)b * 2 + 1] = u[1]; }
      if (n_steps) n_steps[b] += 1;
      if (n_failed && failed) n_failed[b] += 1;
    }
    return (int)MPCB_OK;
  });
}
