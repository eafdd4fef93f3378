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
