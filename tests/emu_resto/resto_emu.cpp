// tests/emu_resto/resto_emu.cpp — TEST INFRASTRUCTURE ONLY.
//
// The kernel source stepped on the CPU as tests/emu steps it (every lane a host thread, mpcb_wave.h's MPCB_WAVE_EMU branch), with the one
// thing tests/emu does not step: the restoration phase inside the lean launch (mpcbd::resto_in_launch, mpcb_dispatch.h).  The wrapper below
// is the wrapper of the __global__ functions of mpcb_api.hip: the attempt loop of the instantiations that fuse, then — where the launch was
// told to restore here — the restoration instantiation on the same LDS for an instance that has just ended with MPCB_ST_NEEDS_RESTO.
// Which launch is told so, and how much LDS it gets, is read from the header mpcb_api.hip launches by; the rule can be forced on or off.
// tests/emu itself is unchanged and steps every restoration phase as a pass of its own.
#define MPCB_WAVE_EMU 1
#include "../../mpc_motion_planning_amd/csrc/mpcb_kernel_dyn.h"
#include "../../mpc_motion_planning_amd/csrc/mpcb_dispatch.h"

#include <thread>
#include <limits>
#include <cstdio>
#include <cstdlib>
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

// One workgroup of one launch: instance b from a.pass on.  The LDS is exactly the doubles the library passes at launch — the restoration
// layout's where a.resto_here is set — poisoned with NaNs, and behind it a guard of NaNs that nothing may write.
static int run_instance(const mpcbd::Variant& v, bool fused, const MpcbKArgs& a, int b) {
  const bool resto = a.pass == MPCB_PASS_RESTO;
  const int total = mpcbd::lds_doubles(v, a.cfg.N, resto || a.resto_here);
  std::vector<double> lds(total + GUARD, std::numeric_limits<double>::quiet_NaN());
  std::barrier<> bar(64);
  wv::Emu emu; emu.bar = &bar;
  const int rc = mpcbd::visit(v, resto, [&](auto inst) {
    using I = decltype(inst);
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
        if constexpr (!I::resto) {
          if (a.resto_here && a.status) {
            wv::sync();                                           // the status lane 0 has just stored, with z and the hand-over record
            const int st = a.status[b];
            wv::sync();
            if (st == MPCB_ST_NEEDS_RESTO)
              solve_as(mpcbd::Inst<I::model, I::nobs, I::gen, I::rk4, I::track, I::params, true>{}, a, b, lds.data(), MPCB_PASS_RESTO);
          }
        }
      });
    for (auto& t : th) t.join();
    return MPCB_OK;
  });
  if (rc != MPCB_OK) return rc;
  for (int i = 0; i < GUARD; ++i)
    if (lds[total + i] == lds[total + i]) {
      std::fprintf(stderr, "mpcb_emu_resto: write %d doubles behind the %d doubles of LDS (model %d, capacity %d, track %d, params %d, pass %d, resto_here %d)\n",
                   i, total, v.model, v.nobs, v.track, v.params, a.pass, a.resto_here);
      return MPCB_EMU_E_GUARD;
    }
  return MPCB_OK;
}

// The arguments of tests/emu's mpcb_emu_solve, and resto_in_launch: the restoration phase inside the lean launch -1 by the rule, 0 never,
// 1 wherever the instantiation has it and a restoration pass follows, whatever the LDS.
extern "C" int mpcb_emu_resto_solve(const mpcb_config* cfg, int32_t B, const double* x0, const double* xs, const double* obs,
                                    int32_t obs_kind, const double* z0, double* z, double* obj, int32_t* status, int32_t* iters,
                                    double* kkt, double* lam_g, double* lam_x, const double* xref, const mpcb_config* cfgs, int32_t resto_in_launch) {
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
  a.cfg = *cfg; a.cfgs = cfgs; a.B = B; a.obs_kind = obs_kind; a.want_mult = (lam_g || lam_x) ? 1 : 0; a.trace_instance = -1;
  a.nz = 2 * cfg->N + nx * (cfg->N + 1);
  a.ng = nx * (cfg->N + 1) + nrate * (cfg->N - 1) + cfg->n_obs * (cfg->obs_terminal ? cfg->N + 1 : cfg->N);
  a.x0 = x0; a.xs = xs; a.obs = obs; a.z0 = z0; a.z = z; a.obj = obj; a.kkt = kkt; a.lam_g = lam_g; a.lam_x = lam_x;
  a.status = status; a.iters = iters; a.xref = xref;
  std::vector<double> work((size_t)B * mpcbk::WK_SIZE, 0.0);
  a.work = mpcbd::multi_pass(*cfg) ? work.data() : nullptr;
  for (int q = 0; q < plan.n; ++q) {
    a.pass = plan.pass[q];
    a.resto_here = mpcbd::resto_in_launch(v, cfg->N, plan, q, resto_in_launch) ? 1 : 0;
    for (int b = 0; b < B; ++b) {      // (the workgroups that would return at once are not started)
      if (a.pass == MPCB_PASS_SECOND && (status[b] == MPCB_ST_SOLVED || status[b] == MPCB_ST_ACCEPTABLE || status[b] == MPCB_ST_INFEASIBLE_X0)) continue;
      if (a.pass == MPCB_PASS_RESTO && status[b] != MPCB_ST_NEEDS_RESTO) continue;
      const int rc = run_instance(v, fused, a, b);
      if (rc != MPCB_OK) return rc;
    }
  }
  return MPCB_OK;
}

// The rule for the first launch of one solve.  fused: 0 / 1 plan as if the instantiation did not / did fuse, -1 as it does.  out[8]: whether
// the first launch runs the restoration phase of its instances itself, the LDS bytes it gets, number of passes, the passes (pass_plan's).
// Returns variant_of's code.
extern "C" int mpcb_emu_resto_dispatch(const mpcb_config* cfg, int32_t track, int32_t params, int32_t start_given, int32_t fused, int64_t* out) {
  mpcbd::Variant v;
  const mpcbd::Refusal r = mpcbd::variant_of(*cfg, track != 0, params != 0, &v);
  if (r.code != MPCB_OK) return r.code;
  const mpcbd::Plan plan = mpcbd::pass_plan(*cfg, start_given != 0, fused < 0 ? mpcbd::fuses(v) : fused != 0);
  out[0] = mpcbd::resto_in_launch(v, cfg->N, plan, 0) ? 1 : 0;
  out[1] = (int64_t)mpcbd::lds_bytes(v, cfg->N, out[0] != 0);
  out[2] = plan.n;
  for (int i = 0; i < 4; ++i) out[3 + i] = i < plan.n ? plan.pass[i] : -1;
  return MPCB_OK;
}
