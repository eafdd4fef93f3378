"""Scenarios and the numpy / oracle reference loop of the stepwise-loop tests, shared by tests/test_loop_cpu.py (the oracle alone: the
admission conditions) and tests/test_loop_gpu.py (ControlLoop against the oracle).  A plain module: no fixtures.

A scenario is a batch of scenes driven for a few steps by an EXTERNAL plant, which is the point of the stepwise loop: a numpy RK4 step
of the kinematic bicycle (the controller's model is Euler: plant and controller disagree) plus seeded Gaussian noise on the state after
every step, and obstacles advanced in numpy.  `drive` runs any controller through it and logs, per step, what the controller was given
and what it returned.

The reference loop is teacher-forced (`teacher_forced`): at step t the oracle solves the logged inputs from the warm start w_t that
follows, in numpy, from the CONTROLLER's own earlier outputs (the executed plan is z when the status is SOLVED or ACCEPTABLE or hold is
off, else the previous w; then the shift).  A wrong commit therefore shows up as a solve that disagrees with the oracle one step later,
and one borderline instance does not send the two sides down different roads for the rest of the run.

Every scenario was admitted only after the oracle alone, driven through the same plant and noise with its own outputs
(`OracleController`), ended >= 0.95 of its (instance, step) solves SOLVED or ACCEPTABLE; tests/test_loop_cpu.py keeps that under test."""
import collections

import numpy as np

from mpc_motion_planning_amd import scenes as _scenes, _abi
from tests import config_cases as cc

N, T = 30, 0.1
NOISE_SD = np.array([0.05, 0.02, 0.002, 0.05])          # m, m, rad, m/s: added to the state after every plant step

Scenario = collections.namedtuple("Scenario", "name n_obs sampler seed B steps predict hold noise_seed")

SCENARIOS = [
    Scenario("c3_predicted_hold", 3, "c3", 7, 32, 8, True, True, 107),
    Scenario("c2_static", 1, "c2", 8, 32, 8, False, False, 108),
]
BY_NAME = {s.name: s for s in SCENARIOS}
MIN_SOLVED_SHARE = 0.95


def ids(scns):
    return [s.name for s in scns]


def config(scn, default_config):
    """default_config: solver.default_config (the product's start settings) or a callable that returns the same on the oracle's side."""
    return default_config(model=_abi.MODEL_KIN, N=N, T=T, n_obs=scn.n_obs)


def scenes(scn):
    """(x0 [B,4], xs [B,4], obs [B,n_obs,6]) of the scenario; predicted scenarios roll obs out per step (`obs_input`)."""
    if scn.sampler == "c3":
        x0, xs, ob0, _ = _scenes.sample_c3(scn.B, N=N, dt=T, seed=scn.seed, n_obs=scn.n_obs)
        return x0, xs, ob0
    x0, xs, obs = _scenes.sample_c2(scn.B, seed=scn.seed)
    return x0, xs, obs


def obs_input(scn, ob):
    """What the solve is given for the current obstacle rows: their constant-velocity roll-out, or the rows themselves."""
    return _scenes.predict_obstacles(ob, T, N) if scn.predict else ob


def solved(status):
    return (status == _abi.ST_SOLVED) | (status == _abi.ST_ACCEPTABLE)


# ---- the controller's bookkeeping in numpy: mpcb_advance's rule ------------------------------------------------------------------------
def executed_plan(w, z, status, hold):
    """The plan a step executes: this step's z, or (hold, and the solve ended neither solved nor acceptable) the previous plan w."""
    if not hold:
        return z.copy()
    return np.where(solved(status)[:, None], z, w)


def shift_plan(plan, n=N, nx=4):
    """u <- [u[1:]; u[-1]], x <- [x[1:]; x[-1]] on z = [vec(U); vec(X)] rows (main_cbf_kin_c_sim.py:16-26)."""
    B = len(plan)
    u = plan[:, :2 * n].reshape(B, n, 2)
    x = plan[:, 2 * n:].reshape(B, n + 1, nx)
    u = np.concatenate([u[:, 1:], u[:, -1:]], axis=1)
    x = np.concatenate([x[:, 1:], x[:, -1:]], axis=1)
    return np.concatenate([u.reshape(B, -1), x.reshape(B, -1)], axis=1)


# ---- the external plant ----------------------------------------------------------------------------------------------------------------
def kin_rhs(x, u, wheelbase):
    return np.stack([x[:, 3] * np.cos(x[:, 2]), x[:, 3] * np.sin(x[:, 2]), x[:, 3] * np.tan(u[:, 0]) / wheelbase, u[:, 1]], axis=1)


def rk4_plant(x, u, wheelbase, dt=T):
    k1 = kin_rhs(x, u, wheelbase)
    k2 = kin_rhs(x + 0.5 * dt * k1, u, wheelbase)
    k3 = kin_rhs(x + 0.5 * dt * k2, u, wheelbase)
    k4 = kin_rhs(x + dt * k3, u, wheelbase)
    return x + dt * (k1 + 2.0 * k2 + 2.0 * k3 + k4) / 6.0


def advance_obstacles(ob, dt=T):
    ob = ob.copy()
    ob[..., 0] += ob[..., 3] * np.cos(ob[..., 2]) * dt
    ob[..., 1] += ob[..., 3] * np.sin(ob[..., 2]) * dt
    return ob


def drive(scn, cfg, step, xs_at=None, x_ref_at=None, steps=None, noise=True, x_edit=None):
    """The scenario through the external plant.  step(t, x, xs, ob, x_ref) -> dict(u0, status, iters, z) is the controller;
    xs_at(t, xs) / x_ref_at(t, x) give this step's set-points / stage references (default: the scenario's xs, no reference);
    x_edit(t, x) may replace the state the controller sees at step t (the forced-failure test).  Returns the per-step log:
    dict(x, xs, ob, x_ref, u0, status, iters, z) with the inputs as the controller saw them."""
    x0, xs, ob = scenes(scn)
    rng = np.random.default_rng(scn.noise_seed)
    x, log = x0.copy(), []
    for t in range(scn.steps if steps is None else steps):
        if x_edit is not None:
            x = x_edit(t, x.copy(), ob)
        xs_t = xs if xs_at is None else xs_at(t, xs)
        xr_t = None if x_ref_at is None else x_ref_at(t, x)
        out = step(t, x, xs_t, ob, xr_t)
        log.append(dict(x=x.copy(), xs=xs_t.copy(), ob=ob.copy(), x_ref=xr_t, u0=out["u0"].copy(), status=out["status"].copy(),
                        iters=out["iters"].copy(), z=out["z"].copy()))
        x = rk4_plant(x, out["u0"], cfg.veh_l)
        draw = rng.normal(size=x.shape) * NOISE_SD              # drawn whether used or not: one stream per scenario
        if noise:
            x = x + draw
        if scn.predict:
            ob = advance_obstacles(ob)
    return log


class OracleController:
    """The reference loop run on its own outputs: the oracle as the controller, the warm start kept in numpy."""

    def __init__(self, scn, cfg, oracle, hold=None):
        self.scn, self.cfg, self.oracle = scn, cfg, oracle
        self.hold = scn.hold if hold is None else hold
        self.w = None

    def __call__(self, t, x, xs, ob, x_ref):
        if self.w is None:
            self.w = np.zeros((len(x), self.cfg.nz()))
        r = self.oracle.solve(self.cfg, x, xs, obs_input(self.scn, ob), z0=self.w, want_multipliers=False, x_ref=x_ref)
        plan = executed_plan(self.w, r["z"], r["status"], self.hold)
        self.w = shift_plan(plan)
        return dict(u0=plan[:, :2].copy(), status=r["status"], iters=r["iters"], z=r["z"])


def teacher_forced(scn, cfg, oracle, log, hold):
    """The oracle on every logged step, started from the w that follows from the LOGGED controller's outputs.  Returns
    (ctl, ref, plans): the controller's and the oracle's z / status / iters stacked over the steps ([steps * B, ...], what agree() of
    tests/test_gpu_parity.py takes), and per step the plan the controller had to execute according to its own outputs."""
    w = np.zeros((len(log[0]["x"]), cfg.nz()))
    ctl = {k: [] for k in ("z", "status", "iters")}
    ref = {k: [] for k in ("z", "status", "iters")}
    plans = []
    for e in log:
        r = oracle.solve(cfg, e["x"], e["xs"], obs_input(scn, e["ob"]), z0=w, want_multipliers=False, x_ref=e["x_ref"])
        for k in ctl:
            ctl[k].append(e[k]); ref[k].append(r[k])
        plan = executed_plan(w, e["z"], e["status"], hold)
        plans.append(plan)
        w = shift_plan(plan)
    return ({k: np.concatenate(v) for k, v in ctl.items()}, {k: np.concatenate(v) for k, v in ref.items()}, plans)


# ---- the library's plant step on its own: the cases of tests/golden/plant_step.npz ------------------------------------------------------
# ControlLoop.advance_device twice in a row (the second step starts from lateral speed and yaw rate that are not zero), recorded on the
# MI355X by tests/golden/make_plant_fixture.py from the build before csrc/mpcb_plant.h existed.  tests/test_loop_gpu.py asserts those
# bytes, tests/test_loop_cpu.py puts the CPU twin and the numpy statement below within 1e-10 of them.
PLANT_B, PLANT_SEED, PLANT_STEPS = 64, 29, 2
TIME_GRID = (0.08,) * 10 + (0.12,) * 20                  # T_0 = 0.08 is the plant's step, not cfg.T

# rows: the two cases of tests/config_cases.py whose configs alternate over the instances (a parameter set), or None
# move: 0 no obstacle moves, 1 every obstacle, 2 the first one only
PlantCase = collections.namedtuple("PlantCase", "name model N n_obs integrator tgrid rows move")
PLANT_CASES = [
    PlantCase("kin_euler", _abi.MODEL_KIN, 30, 1, _abi.INT_EULER, None, None, 1),
    PlantCase("kin_rk4", _abi.MODEL_KIN, 30, 1, _abi.INT_RK4, None, None, 1),
    PlantCase("dyn_euler", _abi.MODEL_DYN, 20, 1, _abi.INT_EULER, None, None, 1),
    PlantCase("time_grid", _abi.MODEL_KIN, 30, 1, _abi.INT_EULER, TIME_GRID, None, 1),
    PlantCase("rows_kin", _abi.MODEL_KIN, 30, 1, _abi.INT_EULER, None, ("default", "geometry"), 1),
    PlantCase("rows_dyn", _abi.MODEL_DYN, 20, 1, _abi.INT_EULER, None, ("dyn_default", "dyn_vehicle"), 1),
    PlantCase("obs3_all", _abi.MODEL_KIN, 30, 3, _abi.INT_EULER, None, None, 1),
    PlantCase("obs3_first", _abi.MODEL_KIN, 30, 3, _abi.INT_EULER, None, None, 2),
    PlantCase("obs3_none", _abi.MODEL_KIN, 30, 3, _abi.INT_EULER, None, None, 0),
]


def plant_inputs_key(case):
    """The cases of one model and obstacle count share their inputs."""
    return "%s%d" % ("dyn" if case.model == _abi.MODEL_DYN else "kin", case.n_obs)


def plant_configs(case, default_config):
    """(cfg, rows): the config of the handle and, for a parameter-set case, the config of every instance."""
    cfg = default_config(model=case.model, N=case.N, T=T, n_obs=case.n_obs)
    cfg.integrator = case.integrator
    if case.rows is None:
        return cfg, None
    two = [cc.base(cc.BY_NAME[n], default_config) for n in case.rows]
    return two[0], [two[b % 2] for b in range(PLANT_B)]


def plant_inputs(case, cfg):
    """(x0 [B,nx], u0 [B,2], obs [B,n_obs,6]): states of sample_c2 / sample_c4, controls uniform in the config's box, obstacles with
    headings and speeds that make both of cos and sin matter."""
    rng = np.random.default_rng(PLANT_SEED)
    if case.model == _abi.MODEL_DYN:
        x0, _, obs = _scenes.sample_c4(PLANT_B, seed=PLANT_SEED, n_obs=case.n_obs)
    else:
        x0 = _scenes.sample_c2(PLANT_B, seed=PLANT_SEED)[0]
        obs = _scenes.sample_c3(PLANT_B, N=case.N, dt=T, seed=PLANT_SEED, n_obs=case.n_obs)[2]
    obs = obs.copy()
    obs[..., 2] = rng.uniform(-0.4, 0.4, obs.shape[:2]); obs[..., 3] = rng.uniform(3.0, 12.0, obs.shape[:2])
    lo, hi = np.array(cfg.u_lo[:2]), np.array(cfg.u_hi[:2])
    return x0, lo + rng.uniform(size=(PLANT_B, 2)) * (hi - lo), obs


def plant_on_device(make_solver, case, cfg, rows, x0, u0, obs):
    """[(x, obs) after step 1, after step 2] of ControlLoop.advance_device with the control held."""
    bs = make_solver(cfg)
    if case.tgrid is not None:
        bs.set_time_grid(np.array(case.tgrid))
    ps = bs.params(rows) if rows is not None else None
    d_x, d_u, d_o = bs.device_array(x0.shape).upload(x0), bs.device_array(u0.shape).upload(u0), bs.device_array(obs.shape).upload(obs)
    out = []
    with bs.loop(PLANT_B, params=ps) as loop:
        for _ in range(PLANT_STEPS):
            loop.advance_device(d_x, d_u, d_o if case.move else None, first_only=case.move == 2, sync=True)
            out.append((d_x.download(), d_o.download()))
    for d in (d_x, d_u, d_o):
        d.free()
    if ps is not None:
        ps.close()
    bs.close()
    return out


def plant_recorded_obs(G, case, k):
    """The obstacle rows [B,n_obs,6] after step k as tests/golden/plant_step.npz holds them: the inputs with x, y replaced."""
    ob = G[plant_inputs_key(case) + "_obs"].copy()
    ob[..., :2] = G["%s_obsxy%d" % (case.name, k)]
    return ob


def _field(cfg, rows, name):
    """A config field as a scalar, or per instance [B, 1] where the case has a parameter set."""
    return getattr(cfg, name) if rows is None else np.array([getattr(r, name) for r in rows])[:, None]


def model_rhs(cfg, rows, x, u):
    """f(x, u) of the configured model in numpy, rows of x / u per instance (kin.py:153-156, dyn.py:156-170)."""
    c = lambda name: _field(cfg, rows, name)   # noqa: E731
    x, u = x[:, :, None], u[:, :, None]
    if cfg.model == _abi.MODEL_KIN:
        return np.concatenate([x[:, 3] * np.cos(x[:, 2]), x[:, 3] * np.sin(x[:, 2]), x[:, 3] * np.tan(u[:, 0]) / c("veh_l"), u[:, 1]], axis=1)
    phi, vx, vy, r, df, ax = x[:, 2], x[:, 3], x[:, 4], x[:, 5], u[:, 0], u[:, 1]
    af, ar = df - (vy + c("veh_lf") * r) / vx, -(vy - c("veh_lr") * r) / vx
    Fcf = -(c("Fymax_f") * 2 * c("aopt_f") / (c("aopt_f") ** 2 + af ** 2)) * af
    Fcr = -(c("Fymax_r") * 2 * c("aopt_r") / (c("aopt_r") ** 2 + ar ** 2)) * ar
    return np.concatenate([vx * np.cos(phi) - vy * np.sin(phi), vx * np.sin(phi) + vy * np.cos(phi), r, ax + r * vy,
                           -r * vx + 2.0 / c("veh_m") * (Fcf * np.cos(df) + Fcr), 2.0 / c("veh_Iz") * (c("veh_lf") * Fcf - c("veh_lr") * Fcr)], axis=1)


def plant_step(cfg, rows, x, u, obs, dt, move):
    """(x, obs) one step on: Euler or classical RK4 as cfg.integrator says, the control held; obstacles as `move` says."""
    k1 = model_rhs(cfg, rows, x, u)
    if cfg.integrator == _abi.INT_RK4:
        k2 = model_rhs(cfg, rows, x + 0.5 * dt * k1, u)
        k3 = model_rhs(cfg, rows, x + 0.5 * dt * k2, u)
        k4 = model_rhs(cfg, rows, x + dt * k3, u)
        k1 = (k1 + 2.0 * k2 + 2.0 * k3 + k4) / 6.0
    n = {0: 0, 1: obs.shape[1], 2: min(1, obs.shape[1])}[move]
    obs = obs.copy()
    obs[:, :n] = advance_obstacles(obs[:, :n], dt)
    return x + dt * k1, obs


# ---- per-step inputs: what a caller-supplied path or a set-point schedule looks like through the stepwise loop ------------------------
SWITCH_STEP = 3


def xs_switch(t, xs):
    """The set-point of every even instance moves to the lane y = 0 from step SWITCH_STEP on."""
    if t < SWITCH_STEP:
        return xs
    xs = xs.copy()
    xs[::2, 1] = 0.0
    return xs


def lane_change_ramp(t, x):
    """x_ref [B,N,4] rebuilt at the current states x every step: straight ahead at the current speed, y ramped between stages 5 and 20
    toward the lane y = 0.5 (even instances) or y = 3.5 (odd ones)."""
    i = np.arange(N)
    lane_y = np.where(np.arange(len(x)) % 2 == 0, 0.5, 3.5)
    r = np.zeros((len(x), N, 4))
    r[:, :, 0] = x[:, None, 0] + x[:, None, 3] * T * (i[None, :] + 1)
    r[:, :, 1] = x[:, None, 1] + (lane_y[:, None] - x[:, None, 1]) * np.clip((i[None, :] - 5) / 15.0, 0.0, 1.0)
    r[:, :, 3] = x[:, None, 3]
    return r


# name -> (scenario, keyword arguments of drive): the per-step-input runs, admitted like the scenarios themselves
PER_STEP = {
    "xs_switches_lane": (BY_NAME["c2_static"], dict(xs_at=xs_switch)),
    "x_ref_lane_change_ramp": (BY_NAME["c2_static"], dict(x_ref_at=lane_change_ramp)),
}
