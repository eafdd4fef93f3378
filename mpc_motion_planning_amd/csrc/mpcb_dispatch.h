// mpcb_dispatch.h — which solve instantiation serves a config, how much LDS it gets, whether it fuses its second attempt, in which
// order the passes of a solve run, which lean launch runs the restoration phase of its instances itself, and which pass is therefore
// not launched.  Host only, plain C++17;
// included behind the kernel headers by mpcb_api.hip (which launches what this header selects) and by tests/emu/wave_emu.cpp and
// tests/emu_resto/resto_emu.cpp (which step the same selection on the CPU).  The policy is stated here and nowhere else.
#pragma once

#include <cstddef>
#include <utility>

namespace mpcbd {

// ---- the variant of a solve: the template arguments of its instantiation, RESTO apart (that one belongs to the pass) -----------------
struct Variant {
  int model, nobs;                  // MPCB_MODEL_*, obstacle-row capacity (not the config's n_obs)
  bool gen, rk4, track, params;     // general-gamma CBF rows, Runge-Kutta shooting rows, per-stage reference, per-instance configs
};
constexpr bool operator==(const Variant& a, const Variant& b) {
  return a.model == b.model && a.nobs == b.nobs && a.gen == b.gen && a.rk4 == b.rk4 && a.track == b.track && a.params == b.params;
}

// The instantiations libmpcbatch.so ships, each as a first-pass and a restoration-pass kernel: kin<0|1|3|5|8>, kin<1|3|8, GEN>,
// kin<0|1|3, RK4> plain and tracking, dyn<1|3|5|8>, and the per-instance kin<0|1|3>, dyn<1|3>.  Every instantiation costs build time
// (the library is one translation unit): visit() below instantiates these and no others.
constexpr bool shipped(const Variant& v) {
  const int n = v.nobs;
  if (v.track && v.params) return false;
  if (v.model == MPCB_MODEL_DYN) return !v.gen && !v.rk4 && !v.track && (n == 1 || n == 3 || (!v.params && (n == 5 || n == 8)));
  if (v.model != MPCB_MODEL_KIN || (v.gen && v.rk4)) return false;
  if (v.params) return !v.gen && !v.rk4 && (n == 0 || n == 1 || n == 3);
  if (v.gen) return n == 1 || n == 3 || n == 8;
  if (v.rk4) return n == 0 || n == 1 || n == 3;
  return n == 0 || n == 1 || n == 3 || n == 5 || n == 8;
}

inline bool is_gen(const mpcb_config& c) { return c.model == MPCB_MODEL_KIN && c.obs_mode == MPCB_OBS_DCBF && c.gamma < 1.0 - 1e-12 && c.n_obs > 0; }
inline bool is_rk4(const mpcb_config& c) { return c.model == MPCB_MODEL_KIN && c.integrator == MPCB_INT_RK4; }

// why a solve has no instantiation: an MPCB_E_* code and a printf format that takes the config's n_obs
struct Refusal { int code; const char* fmt; };

// The variant that serves a config check_cfg has accepted, or the reason why the library ships none for it.
inline Refusal variant_of(const mpcb_config& c, bool track, bool params, Variant* out) {
  const bool dyn = c.model == MPCB_MODEL_DYN, gen = is_gen(c), rk4 = is_rk4(c);
  if (params && track) return {MPCB_E_UNSUPPORTED, "a parameter set together with a per-stage reference"};
  if (track && dyn) return {MPCB_E_UNSUPPORTED, "per-stage reference tracking is built for the kinematic model only"};
  if (params) {
    if (gen) return {MPCB_E_UNSUPPORTED, "parameter sets: general-gamma discrete-CBF rows have no per-instance kernel (keep-out or gamma = 1 rows only)"};
    if (c.integrator == MPCB_INT_RK4) return {MPCB_E_UNSUPPORTED, "parameter sets: MPCB_INT_RK4 has no per-instance kernel (MPCB_INT_EULER only)"};
    if (c.n_obs > 3) return {MPCB_E_UNSUPPORTED, "parameter sets: n_obs = %d, the per-instance kernels are built for up to 3 obstacles"};
  }
  const Variant v{c.model, dyn ? mpcbk::obs_capacity_dyn(c.n_obs) : mpcbk::obs_capacity_kin(c.n_obs, gen), gen, rk4, track, params};
  if (!shipped(v)) return {MPCB_E_UNSUPPORTED, "no kernel instantiation serves this config (n_obs = %d)"};     // (a config check_cfg rejects)
  *out = v;
  return {MPCB_OK, ""};
}

// ---- LDS of one workgroup: the one host-side caller of layout_kin / layout_dyn ---------------------------------------------------------
constexpr size_t LDS_MAX_BYTES = 160 * 1024;          // one CU's LDS on gfx950
inline int lds_doubles(const Variant& v, int N, bool resto) {
  const int in_lds = mpcbk::obs_in_lds(v.nobs);
  if (v.model == MPCB_MODEL_DYN) return mpcbk::layout_dyn(N, resto, in_lds).total;
  return mpcbk::layout_kin(N, 2 * N + 4 * (N + 1), resto, in_lds, v.gen || v.rk4 /* four more rows in the entry table */, v.track).total;
}
inline size_t lds_bytes(const Variant& v, int N, bool resto) { return (size_t)lds_doubles(v, N, resto) * sizeof(double); }

// ---- the second attempt inside the first launch ------------------------------------------------------------------------------------
// Second start of kind 1 (the cold-start batches): the wave whose first attempt failed starts over from z = 0 at once instead of in a
// second launch that can only begin when the slowest first attempt of the batch has finished.  Only the instantiations with registers
// to spare do this (kin<0>, kin<1>: +17 AGPRs; measured C2 +2.5 % with six lanes, +11 % with one launch at a time): the loop around the
// inlined solve keeps loop-invariant per-lane values alive across both attempts, which costs kin<3> 200 -> 256 AGPRs + 124 B of scratch
// (C3 -9 %) and dyn<3> 236 -> 256 + 452 B (C4 -7 %).  The instantiations that do not fuse run the second attempt as a pass of its own
// (pass_plan).  -DMPCB_NO_FUSED_SECOND: no instantiation fuses (A/B builds).
// The kernels' `if constexpr` (mpcb_kin_fuses / mpcb_dyn_fuses in mpcb_api.hip) and the host's pass plan both read this function.
#ifdef MPCB_NO_FUSED_SECOND
constexpr int FUSE_NOBS_MAX = -1;
#else
constexpr int FUSE_NOBS_MAX = 3;
#endif
constexpr bool fuses(int nobs, bool gen, bool rk4) { return nobs <= FUSE_NOBS_MAX && !gen && !rk4; }
constexpr bool fuses(const Variant& v) { return fuses(v.nobs, v.gen, v.rk4); }

// ---- the passes of a solve ---------------------------------------------------------------------------------------------------------
// A second start exists only after a roll-out start.  cfg.second_start = 3: by the kind of start — a cold start (no start vector)
// behaves as 1, a solve with a start vector (a warm start, every step of a closed loop) as 2.
inline bool second_pass(const mpcb_config& c) { return c.second_start != 0 && c.init_rollout != 0; }
inline bool multi_pass(const mpcb_config& c) { return c.restoration != 0 || second_pass(c); }       // the passes hand over through work records and statuses
inline bool second_kind1(const mpcb_config& c, bool start_given) {
  return second_pass(c) && (c.second_start == 3 ? !start_given : c.second_start == 1);
}

// First attempt from the caller's start, its restoration pass; with a second start the lean kernel once more over the same grid, where
// only the instances whose first attempt did not succeed run from z = 0, and the restoration pass of that attempt.  Kind 1 skips the
// first attempt's restoration pass (its instances go straight to the second start), and on an instantiation that fuses, its second
// attempt has already run inside the first launch.
struct Plan { int n; int pass[4]; };
inline Plan pass_plan(const mpcb_config& c, bool start_given, bool fused) {
  Plan p{0, {0, 0, 0, 0}};
  const bool kind1 = second_kind1(c, start_given);
  p.pass[p.n++] = MPCB_PASS_FIRST;
  if (c.restoration && !kind1) p.pass[p.n++] = MPCB_PASS_RESTO;
  if (second_pass(c)) {
    if (!(kind1 && fused)) p.pass[p.n++] = MPCB_PASS_SECOND;
    if (c.restoration) p.pass[p.n++] = MPCB_PASS_RESTO;
  }
  return p;
}

// ---- the restoration phase inside the lean launch ------------------------------------------------------------------------------------
// The restoration pass continues a few instances in a hundred (C2: about 100 of 4096), yet as a launch of its own it can only begin
// when the slowest instance of the lean launch has finished, and it holds its stream for the length of its own slowest instance.  Where
// this rule says yes, the wave of the lean launch that ends with MPCB_ST_NEEDS_RESTO calls the restoration instantiation itself, at once
// and on the same LDS; that instantiation reads z, the status and the hand-over record back from memory exactly as in a launch of its
// own, so the results are the same by construction.  The MPCB_PASS_RESTO pass stays in the plan, has no instance left to continue, and
// is not launched (pass_is_empty below).
// Only the Euler kin<0|1> kernels without GEN (plain, tracking, per-instance) do this: their restoration twins need no scratch, those of
// kin<3> and dyn<1|3> spill 230-600 B and would take the lean kernels' zero scratch with them.  -DMPCB_NO_RESTO_IN_LAUNCH: no
// instantiation does (A/B builds).  The kernels' `if constexpr` (mpcb_api.hip) and the host's launch both read restores_here().
#ifdef MPCB_NO_RESTO_IN_LAUNCH
constexpr int RESTO_HERE_NOBS_MAX = -1;
#else
constexpr int RESTO_HERE_NOBS_MAX = 1;
#endif
constexpr bool restores_here(int model, int nobs, bool gen, bool rk4) {
  return model == MPCB_MODEL_KIN && nobs <= RESTO_HERE_NOBS_MAX && !gen && !rk4;
}
constexpr bool restores_here(const Variant& v) { return restores_here(v.model, v.nobs, v.gen, v.rk4); }

// workgroups of one wave a CU holds: one per SIMD (the solve kernels' registers), and as many as its LDS has room for
constexpr int wgs_per_cu(size_t lds) { return lds == 0 || LDS_MAX_BYTES / lds >= 4 ? 4 : (int)(LDS_MAX_BYTES / lds); }

// Does launch i of the plan run the restoration phase of its instances itself?  The instantiation has the code, the plan's next pass
// is the restoration pass, and the restoration layout's LDS leaves the lean launch as many workgroups per CU as its own layout
// (N = 30: 4 and 4; N = 50: 3 and 2, so there the passes stay apart).  force: 0 never, 1 without the LDS condition (tests/emu_resto), -1 the rule.
inline bool resto_in_launch(const Variant& v, int N, const Plan& plan, int i, int force = -1) {
  if (force == 0 || !restores_here(v)) return false;
  if (plan.pass[i] == MPCB_PASS_RESTO || i + 1 >= plan.n || plan.pass[i + 1] != MPCB_PASS_RESTO) return false;
  return force == 1 || wgs_per_cu(lds_bytes(v, N, true)) >= wgs_per_cu(lds_bytes(v, N, false));
}

// Is pass i of the plan known to have no work before anything runs?  Exactly when it is the restoration pass and the pass before it
// restores in its own launch: that launch leaves no instance at MPCB_ST_NEEDS_RESTO, so every workgroup of pass i would return at once,
// yet as a launch each of them waits for a whole wave slot (the restoration kernel's registers and LDS) behind the other solves in
// flight, and the stream is held meanwhile.  The launcher skips such a pass; pass_plan and Plan describe the solve, not the launches.
inline bool pass_is_empty(const Variant& v, int N, const Plan& plan, int i, int force = -1) {
  return i > 0 && plan.pass[i] == MPCB_PASS_RESTO && resto_in_launch(v, N, plan, i - 1, force);
}

// ---- run-time variant -> compile-time template arguments ------------------------------------------------------------------------------
// visit<RESTO>(v, f) calls f(Inst<...>{}) for the instantiation that is v, and returns what f returns (an int; -1 if v is not shipped).
// f is instantiated for the shipped variants only.
template <int MODEL, int NOBS, bool GEN, bool RK4, bool TRACK, bool PARAMS, bool RESTO>
struct Inst {
  static constexpr int model = MODEL, nobs = NOBS;
  static constexpr bool gen = GEN, rk4 = RK4, track = TRACK, params = PARAMS, resto = RESTO;
};

namespace detail {
constexpr int CAPS[5] = {0, 1, 3, 5, 8};
// candidate I of the grid params x track x gen x rk4 x model x capacity
constexpr Variant candidate(int I) { return {(I / 5) % 2 ? MPCB_MODEL_DYN : MPCB_MODEL_KIN, CAPS[I % 5], (I / 20) % 2 != 0, (I / 10) % 2 != 0, (I / 40) % 2 != 0, (I / 80) % 2 != 0}; }
constexpr int CANDIDATES = 160;
constexpr int count_shipped() { int n = 0; for (int i = 0; i < CANDIDATES; ++i) n += shipped(candidate(i)) ? 1 : 0; return n; }
static_assert(2 * count_shipped() == 62, "the library ships 62 solve instantiations");

template <bool RESTO, int I, class F>
bool visit_one(const Variant& v, F& f, int& rc) {
  constexpr Variant c = candidate(I);
  if constexpr (shipped(c)) {
    if (v == c) { rc = f(Inst<c.model, c.nobs, c.gen, c.rk4, c.track, c.params, RESTO>{}); return true; }
  }
  return false;
}
template <bool RESTO, class F, int... I>
int visit_all(const Variant& v, F& f, std::integer_sequence<int, I...>) {
  int rc = -1;
  (void)(visit_one<RESTO, I>(v, f, rc) || ...);
  return rc;
}
}  // namespace detail

template <bool RESTO, class F>
int visit(const Variant& v, F&& f) { return detail::visit_all<RESTO>(v, f, std::make_integer_sequence<int, detail::CANDIDATES>{}); }
template <class F>
int visit(const Variant& v, bool resto, F&& f) { return resto ? visit<true>(v, f) : visit<false>(v, f); }

}  // namespace mpcbd
