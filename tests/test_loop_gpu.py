"""The stepwise loop on the MI355X (mpcb_loop_*, BatchSolver.loop / ControlLoop): one controller step as a call, the controller's state
resident on the device, the plant outside.

Two kinds of evidence.  Bit equality where both sides are the library: (step_device, advance_device) repeated against closed_loop, a
loop against itself after a reset / a transplanted start / on another lane.  Agreement with the CPU oracle where the plant is external:
the teacher-forced reference loop of tests/loop_cases.py, compared with agree() of tests/test_gpu_parity.py over all (instance, step)
solves of a run: status agreement >= 0.98, trajectories within 1e-5 inside the basin, at most other_basin_allowance() beyond.
Every test: B <= 64, <= 8 steps."""
import ctypes as C
import os

import numpy as np
import pytest

from mpc_motion_planning_amd import scenes, _abi
from mpc_motion_planning_amd._lib import lib, MpcbError
from mpc_motion_planning_amd.solver import default_config, vary
from tests import config_cases as cc, loop_cases as lc, params_cases as pc
from tests.test_gpu_parity import agree

pytestmark = pytest.mark.gpu

STATIC, PREDICTED, CURRENT = _abi.OBSMOVE_STATIC, _abi.OBSMOVE_PREDICTED, _abi.OBSMOVE_CURRENT
HIST = ("x_hist", "u_hist", "status", "iters", "obs_state")
MIN_SAME_STATUS = 0.98


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def stepwise(bs, x0, xs, obs, steps, motion=STATIC, hold=False, first_only=False, params=None):
    """closed_loop rebuilt from the stepwise pieces: x0, obs and u0 stay on the device, step_device(sync = 0) then advance_device, the
    histories assembled here.  Returns what closed_loop returns."""
    B, nx, no = len(x0), bs.nx, bs.cfg.n_obs
    d_x0 = bs.device_array((B, nx)).upload(x0); d_xs = bs.device_array((B, nx)).upload(xs)
    d_obs = bs.device_array((B, no, 6)).upload(obs) if no else None
    d_u0 = bs.device_array((B, 2)); d_st = bs.device_array((B,), np.int32); d_it = bs.device_array((B,), np.int32)
    xh = np.empty((B, steps + 1, nx)); uh = np.empty((B, steps, 2)); st = np.empty((B, steps), np.int32); it = np.empty((B, steps), np.int32)
    xh[:, 0] = x0
    with bs.loop(B, hold_on_failure=hold, predict=motion == PREDICTED, params=params) as loop:
        for t in range(steps):
            loop.step_device(d_x0, d_xs, d_u0, d_obs=d_obs, d_status=d_st, d_iters=d_it)
            loop.advance_device(d_x0, d_u0, d_obs if motion != STATIC else None, first_only=first_only)
            uh[:, t] = d_u0.download(); st[:, t] = d_st.download(); it[:, t] = d_it.download(); xh[:, t + 1] = d_x0.download()
        assert (loop.steps == steps).all() and np.array_equal(loop.failures, (~lc.solved(st)).sum(axis=1))
    ob = d_obs.download() if no else None
    for d in (d_x0, d_xs, d_obs, d_u0, d_st, d_it):
        if d is not None:
            d.free()
    return dict(x_hist=xh, u_hist=uh, status=st, iters=it, obs_state=ob)


def differing(a, b, keys=HIST):
    return [k for k in keys if not (a[k] is None and b[k] is None) and not bits(a[k], b[k])]


# ---- 1. (step_device, advance_device) repeated IS closed_loop -----------------------------------------------------------------------------
def _c2_moving(B, seed=21):
    x0, xs, obs = scenes.sample_c2(B, seed=seed)
    x0[:, 0] = np.minimum(x0[:, 0], 10.0)
    obs = obs.copy(); obs[:, :, 3] = 6.0
    return x0, xs, obs


def _case_c2_static():
    x0, xs, obs = scenes.sample_c2(32, seed=8)
    return default_config(N=30, n_obs=1), None, x0, xs, obs, 6, STATIC, False


def _case_c3_predict():
    x0, xs, ob0, _ = scenes.sample_c3(32, seed=7)
    return default_config(N=30, n_obs=3), None, x0, xs, ob0, 6, PREDICTED, False


def _case_c3_predict_first_only():
    return _case_c3_predict()[:7] + (True,)


def _case_c4_dyn():
    x0, xs, obs = scenes.sample_c4(16, seed=31, n_obs=1)
    return default_config(model=_abi.MODEL_DYN, N=20, n_obs=1), None, x0, xs, obs, 4, STATIC, False


def _case_rk4():
    cfg = default_config(N=30, n_obs=1); cfg.integrator = _abi.INT_RK4
    return (cfg, None) + _c2_moving(16) + (4, CURRENT, False)


def _case_time_grid():
    return (default_config(N=30, n_obs=1), np.r_[np.full(10, 0.08), np.full(20, 0.12)]) + _c2_moving(16) + (4, PREDICTED, False)


EQUAL_CASES = {"c2_static": _case_c2_static, "c3_predict": _case_c3_predict, "c3_predict_first_only": _case_c3_predict_first_only,
               "c4_dyn": _case_c4_dyn, "rk4": _case_rk4, "time_grid": _case_time_grid}


@pytest.mark.parametrize("hold", [False, True], ids=["apply", "hold"])
@pytest.mark.parametrize("name", sorted(EQUAL_CASES))
def test_step_then_advance_equals_closed_loop_bit_for_bit(gpu_solver_factory, name, hold):
    cfg, tgrid, x0, xs, obs, steps, motion, first_only = EQUAL_CASES[name]()
    bs = gpu_solver_factory(cfg)
    if tgrid is not None:
        bs.set_time_grid(tgrid)
    want = bs.closed_loop(x0, xs, obs, steps=steps, obs_motion=motion, hold_on_failure=hold, advance_first_only=first_only)
    got = stepwise(bs, x0, xs, obs, steps, motion, hold, first_only)
    bs.close()
    print("%s hold=%d: %d of %d solves solved, statuses %s" % (name, hold, lc.solved(want["status"]).sum(), want["status"].size,
                                                              np.bincount(want["status"].ravel())))
    assert differing(got, want) == []
    assert lc.solved(want["status"]).mean() >= 0.75                               # the comparison is about solved steps, not about a batch of failures
    if motion != STATIC:
        assert not np.array_equal(want["obs_state"][:, 0], obs[:, 0])
        if first_only and cfg.n_obs > 1:
            assert np.array_equal(want["obs_state"][:, 1:], obs[:, 1:])


def test_every_step_fails_and_the_held_plan_is_applied(gpu_solver_factory):
    """max_iter = 12, second_start = 0, hold on: no solve ends solved or acceptable, so every u0 is the held plan's (the zero start,
    shifted).  Nearly every status is MAXITER; an ego that coasts into the obstacle under the held zero control fails with another status
    (oracle: instance 14 ends INFEASIBLE_X0 and instance 19 RESTO_FAILED at the sixth step), which is a failed step all the same."""
    cfg = default_config(N=30, n_obs=1); cc.max_iter_12(cfg)
    x0, xs, obs = scenes.sample_c2(32, seed=8)
    bs = gpu_solver_factory(cfg)
    want = bs.closed_loop(x0, xs, obs, steps=6, hold_on_failure=True)
    got = stepwise(bs, x0, xs, obs, 6, STATIC, True)
    bs.close()
    assert differing(got, want) == []
    print("statuses %s" % np.bincount(got["status"].ravel()))
    assert not lc.solved(got["status"]).any() and (got["u_hist"] == 0.0).all()
    assert (got["status"] == _abi.ST_MAXITER).mean() >= 0.95


def test_parameter_set_of_two_interleaved_configs_equals_closed_loop_params(gpu_solver_factory):
    B, steps = 16, 6
    x0, xs, obs = scenes.sample_c2(B, seed=21)
    x0[:, 0] = np.minimum(x0[:, 0], 10.0)
    cfgs = [cc.base(cc.BY_NAME[n], default_config) for n in ("default", "geometry")]
    which = np.arange(B) % 2
    bs = gpu_solver_factory(cfgs[0])
    with bs.params(pc.rows(cfgs, which)) as ps:
        want = bs.closed_loop(x0, xs, obs, steps=steps, params=ps)
        got = stepwise(bs, x0, xs, obs, steps, STATIC, params=ps)
    plain = bs.closed_loop(x0, xs, obs, steps=steps)
    bs.close()
    assert differing(got, want) == []
    assert np.abs(got["x_hist"][which == 1] - plain["x_hist"][which == 1]).max() > 1e-4       # the other wheelbase is seen, by solve and plant


def test_advance_device_returns_the_recorded_plant_steps_bit_for_bit(gpu_solver_factory):
    """tests/golden/plant_step.npz holds ControlLoop.advance_device from the build before the glue kernels were rebuilt on
    csrc/mpcb_plant.h: since then both sides of the comparisons above are made of the same functions, and this is what ties them to
    the bits of the kernels they replaced.  Every case of lc.PLANT_CASES, 64 instances, two steps in a row."""
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plant_step.npz"))
    bad = []
    for case in lc.PLANT_CASES:
        cfg, rows = lc.plant_configs(case, default_config)
        key = lc.plant_inputs_key(case)
        got = lc.plant_on_device(gpu_solver_factory, case, cfg, rows, G[key + "_x0"], G[key + "_u0"], G[key + "_obs"])
        assert len(got) == lc.PLANT_STEPS
        for k, (x, ob) in enumerate(got, start=1):
            want_x, want_ob = G["%s_x%d" % (case.name, k)], lc.plant_recorded_obs(G, case, k)
            print("%s step %d: state %.2e, obstacles %.2e from the recording" % (case.name, k, np.abs(x - want_x).max(), np.abs(ob - want_ob).max()))
            bad += ["%s step %d %s" % (case.name, k, n) for n, a, b in (("x", x, want_x), ("obs", ob, want_ob)) if not bits(a, b)]
    assert bad == []


# ---- 2. external plant, against the oracle --------------------------------------------------------------------------------------------------
def _against_reference_loop(scn, cfg, oracle_mod, log, hold):
    ctl, ref, plans = lc.teacher_forced(scn, cfg, oracle_mod, log, hold)
    agree(ctl, ref, min_same_status=MIN_SAME_STATUS)
    for t, (e, plan) in enumerate(zip(log, plans)):
        assert bits(e["u0"], plan[:, :2]), "step %d: u0 is not the executed plan's first control at %s" % (
            t, np.nonzero((e["u0"] != plan[:, :2]).any(axis=1))[0][:8])
    return ctl


@pytest.mark.parametrize("scn", lc.SCENARIOS, ids=lc.ids(lc.SCENARIOS))
def test_external_plant_against_the_reference_loop(gpu_solver_factory, oracle_mod, scn):
    """Host-pointer step with a numpy RK4 plant and noise the controller's model knows nothing of."""
    cfg = lc.config(scn, default_config)
    bs = gpu_solver_factory(cfg)
    with bs.loop(scn.B, hold_on_failure=scn.hold, predict=scn.predict) as loop:
        log = lc.drive(scn, cfg, lambda t, x, xs, ob, xr: loop.step(x, xs, ob, x_ref=xr))
        steps, failures = loop.steps, loop.failures
    bs.close()
    ctl = _against_reference_loop(scn, cfg, oracle_mod, log, scn.hold)
    status = ctl["status"].reshape(scn.steps, scn.B)
    assert (steps == scn.steps).all() and np.array_equal(failures, (~lc.solved(status)).sum(axis=0))
    assert lc.solved(status).mean() >= 0.9


# ---- 3. forced failure and hold -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", [True, False], ids=["hold", "apply"])
def test_forced_failure(gpu_solver_factory, hold):
    """At step 3 the ego of instance 5 stands on the centre of its obstacle: MPCB_ST_INFEASIBLE_X0 for it alone."""
    scn, b, t_fail = lc.BY_NAME["c2_static"], 5, 3
    cfg = lc.config(scn, default_config)

    def move(t, x, ob):
        if t == t_fail:
            x[b, :2] = ob[b, 0, :2]
        return x

    bs = gpu_solver_factory(cfg)
    runs = {}
    for moved in (True, False):
        with bs.loop(scn.B, hold_on_failure=hold) as loop:
            runs[moved] = lc.drive(scn, cfg, lambda t, x, xs, ob, xr: loop.step(x, xs, ob), steps=t_fail + 1, x_edit=move if moved else None)
            failures = loop.failures
        if moved:
            failed = failures
    bs.close()
    log = runs[True]
    assert all(lc.solved(log[t]["status"][b]) for t in range(t_fail)), "instance %d must solve before the move" % b
    assert log[t_fail]["status"][b] == _abi.ST_INFEASIBLE_X0 == 3
    if hold:
        # the plan executed at step 2 is that step's z (it solved); shifted once it is w, whose first control is the plan's stage 1
        assert bits(log[t_fail]["u0"][b], log[t_fail - 1]["z"][b, 2:4])
        assert failed[b] == 1
    else:
        assert bits(log[t_fail]["u0"][b], log[t_fail]["z"][b, :2])
    others = np.arange(scn.B) != b
    for t in range(t_fail + 1):
        for k in ("u0", "z", "status", "iters"):
            assert bits(runs[True][t][k][others], runs[False][t][k][others]), "step %d: %s of the neighbours changed" % (t, k)
    assert lc.solved(log[t_fail]["status"][others]).sum() >= scn.B - 3


# ---- 4. per-step inputs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(lc.PER_STEP))
def test_per_step_inputs_against_the_reference_loop(gpu_solver_factory, oracle_mod, name):
    scn, kw = lc.PER_STEP[name]
    cfg = lc.config(scn, default_config)
    bs = gpu_solver_factory(cfg)
    with bs.loop(scn.B, hold_on_failure=scn.hold) as loop:
        log = lc.drive(scn, cfg, lambda t, x, xs, ob, xr: loop.step(x, xs, ob, x_ref=xr), **kw)
        plain = None
        if name == "x_ref_lane_change_ramp":
            plain = bs.solve_batch(log[0]["x"], log[0]["xs"], log[0]["ob"], z0=np.zeros((scn.B, bs.nz)))
    bs.close()
    _against_reference_loop(scn, cfg, oracle_mod, log, scn.hold)
    if plain is not None:                       # the reference is seen: step 0 differs from the set-point solve from the same start
        assert np.abs(plain["z"] - log[0]["z"]).max() > 1e-3
    else:
        assert not np.array_equal(log[lc.SWITCH_STEP]["xs"], log[0]["xs"])


def test_x_ref_where_the_solve_entries_refuse_it(gpu_solver_factory):
    """x_ref on the dynamic model and x_ref with a parameter set: the codes of mpcb_solve_device_ref, and the loop is left as it was."""
    dyn = default_config(model=_abi.MODEL_DYN, N=20, n_obs=1)
    x0, xs, obs = scenes.sample_c4(4, seed=31, n_obs=1)
    bs = gpu_solver_factory(dyn)
    d = [bs.device_array(s) for s in ((4, 6), (4, 6), (4, 20, 6), (4, 1, 6), (4, 184))]
    with pytest.raises(MpcbError) as ref_code:
        bs.solve_device(4, d[0], d[1], d[3], _abi.OBSIN_STATIC, None, d[4], d_x_ref=d[2])
    with bs.loop(4) as loop:
        with pytest.raises(MpcbError) as e:
            loop.step(x0, xs, obs, x_ref=np.zeros((4, 20, 6)))
        assert e.value.code == ref_code.value.code == _abi.E_UNSUPPORTED and "kinematic" in str(e.value)
        assert (loop.steps == 0).all() and (loop.start == 0.0).all()
        assert loop.step(x0, xs, obs)["u0"].shape == (4, 2) and (loop.steps == 1).all()
    for a in d:
        a.free()
    bs.close()
    cfg = default_config(N=30, n_obs=1)
    x0, xs, obs = scenes.sample_c2(4, seed=3)
    bs = gpu_solver_factory(cfg)
    with bs.params(vary(cfg, 4)) as ps, bs.loop(4, params=ps) as loop:
        with pytest.raises(MpcbError) as e:
            loop.step(x0, xs, obs, x_ref=np.zeros((4, 30, 4)))
        assert e.value.code == _abi.E_UNSUPPORTED and "parameter set" in str(e.value)
        assert (loop.steps == 0).all()
    bs.close()


# ---- 5. reset and start -------------------------------------------------------------------------------------------------------------------------
def test_reset_with_a_mask_and_transplanted_starts(gpu_solver_factory):
    scn, t_cut = lc.BY_NAME["c2_static"], 4
    cfg = lc.config(scn, default_config)
    mask = np.arange(scn.B) % 3 == 0
    bs = gpu_solver_factory(cfg)
    keys = ("u0", "z", "status", "iters")
    with bs.loop(scn.B) as loop:
        base = lc.drive(scn, cfg, lambda t, x, xs, ob, xr: loop.step(x, xs, ob))

    # reset with a mask before step 4
    def with_reset(loop):
        def step(t, x, xs, ob, xr):
            if t == t_cut:
                loop.reset(mask)
            return loop.step(x, xs, ob)
        return step
    with bs.loop(scn.B) as loop:
        cut = lc.drive(scn, cfg, with_reset(loop))
        assert np.array_equal(loop.steps, np.where(mask, scn.steps - t_cut, scn.steps))
    with bs.loop(scn.B) as fresh:                                  # a fresh loop fed the states the reset run went through from step 4 on
        for t in range(t_cut, scn.steps):
            r = fresh.step(cut[t]["x"], cut[t]["xs"], cut[t]["ob"])
            for k in keys:
                assert bits(r[k][mask], cut[t][k][mask]), "step %d: %s of the reset instances is not a fresh loop's" % (t, k)
    for t in range(scn.steps):
        for k in keys:
            assert bits(cut[t][k][~mask], base[t][k][~mask]), "step %d: %s of the instances that were not reset changed" % (t, k)
    assert any(not bits(cut[t]["z"][mask], base[t]["z"][mask]) for t in range(t_cut, scn.steps))      # the reset is seen

    # set_start(get_start()) changes nothing; a loop seeded with another loop's start continues it
    def with_transplant(loop, other):
        def step(t, x, xs, ob, xr):
            if t == t_cut:
                w = loop.start
                loop.start = w
                other.start = w
            if t >= t_cut + 2:
                return other.step(x, xs, ob)
            r = loop.step(x, xs, ob)
            if t == t_cut + 1:
                other.start = loop.start
            return r
        return step
    with bs.loop(scn.B) as loop, bs.loop(scn.B) as other:
        moved = lc.drive(scn, cfg, with_transplant(loop, other))
        assert (other.steps == scn.steps - t_cut - 2).all() and (loop.steps == t_cut + 2).all()
    bs.close()
    for t in range(scn.steps):
        for k in keys:
            assert bits(moved[t][k], base[t][k]), "step %d: %s differs after set_start" % (t, k)


# ---- 6. lanes -----------------------------------------------------------------------------------------------------------------------------------
def _alternating(bs, batches, steps):
    """One loop per batch (created in order: loop i runs on lane i mod inflight), stepped alternately with sync = 0; nothing waits until
    the end, every step writes its own output buffers."""
    runs = []
    for x0, xs, obs in batches:
        B = len(x0)
        runs.append(dict(B=B, loop=bs.loop(B, predict=True), d_x0=bs.device_array((B, 4)).upload(x0), d_xs=bs.device_array((B, 4)).upload(xs),
                         d_obs=bs.device_array(obs.shape).upload(obs), d_u0=[bs.device_array((B, 2)) for _ in range(steps)],
                         d_st=[bs.device_array((B,), np.int32) for _ in range(steps)], d_it=[bs.device_array((B,), np.int32) for _ in range(steps)]))
    for t in range(steps):
        for r in runs:
            r["loop"].step_device(r["d_x0"], r["d_xs"], r["d_u0"][t], d_obs=r["d_obs"], d_status=r["d_st"][t], d_iters=r["d_it"][t])
            r["loop"].advance_device(r["d_x0"], r["d_u0"][t], r["d_obs"])
    out = []
    for r in runs:
        out.append(dict(u_hist=np.stack([d.download() for d in r["d_u0"]], axis=1), status=np.stack([d.download() for d in r["d_st"]], axis=1),
                        iters=np.stack([d.download() for d in r["d_it"]], axis=1), x=r["d_x0"].download(), obs_state=r["d_obs"].download(),
                        start=r["loop"].start))
        r["loop"].close()
        for d in [r["d_x0"], r["d_xs"], r["d_obs"]] + r["d_u0"] + r["d_st"] + r["d_it"]:
            d.free()
    return out


def test_two_loops_on_two_lanes_equal_their_own_runs(gpu_solver_factory):
    cfg, steps = default_config(N=30, n_obs=3), 6
    batches = []
    for seed in (7, 11):
        x0, xs, ob0, _ = scenes.sample_c3(32, seed=seed)
        batches.append((x0, xs, ob0))
    two = gpu_solver_factory(cfg, inflight=2)
    together = _alternating(two, batches, steps)
    two.close()
    for i, batch in enumerate(batches):
        one = gpu_solver_factory(cfg, inflight=1)
        alone = _alternating(one, [batch], steps)[0]
        want = one.closed_loop(*batch, steps=steps, obs_motion=PREDICTED)
        one.close()
        keys = ("u_hist", "status", "iters", "x", "obs_state", "start")
        assert [k for k in keys if not bits(together[i][k], alone[k])] == [], "loop %d" % i
        assert bits(alone["u_hist"], want["u_hist"]) and bits(alone["x"], want["x_hist"][:, -1]) and bits(alone["status"], want["status"])
    assert not bits(together[0]["u_hist"], together[1]["u_hist"])


# ---- 7. validation --------------------------------------------------------------------------------------------------------------------------------
def test_validation_through_return_codes(gpu_solver_factory):
    L = lib()
    cfg = default_config(N=30, n_obs=1)
    x0, xs, obs = scenes.sample_c2(4, seed=3)
    bs, other = gpu_solver_factory(cfg), gpu_solver_factory(cfg)
    out = C.c_void_p()

    def code_and_text(rc, h=None):
        return rc, L.mpcb_last_error(h if h is not None else bs._h).decode()

    assert code_and_text(L.mpcb_loop_create(bs._h, 0, 0, None, C.byref(out)))[0] == _abi.E_INVALID and not out.value
    rc, text = code_and_text(L.mpcb_loop_create(bs._h, 4, 8, None, C.byref(out)))
    assert rc == _abi.E_INVALID and "flags" in text
    assert L.mpcb_loop_create(bs._h, 4, _abi.CL_ADVANCE_FIRST_ONLY, None, C.byref(out)) == _abi.E_INVALID      # a flag of advance, not of create
    assert L.mpcb_loop_create(bs._h, 4, 0, None, None) == _abi.E_INVALID

    loop, foreign = bs.loop(4, hold_on_failure=True, predict=True), other.loop(4)
    rc, text = code_and_text(L.mpcb_loop_reset(bs._h, foreign.ptr, None))
    assert rc == _abi.E_INVALID and "does not belong" in text
    assert L.mpcb_loop_destroy(bs._h, foreign.ptr) == _abi.E_INVALID
    assert L.mpcb_loop_reset(bs._h, None, None) == _abi.E_INVALID
    # required pointers
    assert L.mpcb_loop_get_start(bs._h, loop.ptr, None) == _abi.E_INVALID and L.mpcb_loop_set_start(bs._h, loop.ptr, None) == _abi.E_INVALID
    u0 = np.empty((4, 2))
    rc, text = code_and_text(L.mpcb_loop_step(bs._h, loop.ptr, None, xs.ctypes.data_as(C.POINTER(C.c_double)), None, None, 0,
                                              u0.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None))
    assert rc == _abi.E_INVALID and "NULL" in text
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    assert L.mpcb_loop_step(bs._h, loop.ptr, p(x0), p(xs), None, None, 0, p(u0), None, None, None, None) == _abi.E_INVALID      # n_obs = 1, obs NULL
    assert L.mpcb_loop_step(bs._h, loop.ptr, p(x0), p(xs), None, p(obs), 7, p(u0), None, None, None, None) == _abi.E_INVALID   # obs_kind
    assert L.mpcb_loop_step(bs._h, loop.ptr, p(x0), p(xs), None, p(obs), 0, None, None, None, None, None) == _abi.E_INVALID    # u0
    assert L.mpcb_loop_step_device(bs._h, loop.ptr, None, None, None, None, 0, None, None, None, None, None, 1) == _abi.E_INVALID
    assert L.mpcb_loop_advance_device(bs._h, loop.ptr, None, None, None, 0, 1) == _abi.E_INVALID
    d_x0, d_u0 = bs.device_array((4, 4)).upload(x0), bs.device_array((4, 2)).upload(np.zeros((4, 2)))
    assert L.mpcb_loop_advance_device(bs._h, loop.ptr, d_x0.ptr, d_u0.ptr, None, 4, 1) == _abi.E_INVALID                          # unknown flags
    assert (loop.steps == 0).all()
    r = loop.step(x0, xs, obs)                                      # after all the refusals the loop works, optional outputs may be NULL
    assert L.mpcb_loop_step(bs._h, loop.ptr, p(x0), p(xs), None, p(obs), 0, p(u0), None, None, None, None) == 0
    assert (loop.steps == 2).all() and r["u0"].shape == (4, 2)
    with pytest.raises(ValueError):
        loop.step(x0[:3], xs[:3], obs[:3])
    # parameter sets: another B, a closed set, a time grid
    ps8, ps4 = bs.params(vary(cfg, 8)), bs.params(vary(cfg, 4))
    with pytest.raises(MpcbError) as e:
        bs.loop(4, params=ps8)
    assert e.value.code == _abi.E_INVALID
    with pytest.raises(MpcbError) as e:
        other.loop(4, params=ps4)                                   # a set of another handle
    assert e.value.code == _abi.E_INVALID
    with_set = bs.loop(4, params=ps4)
    cold = bs.solve_batch(x0, xs, obs, z0=np.zeros((4, bs.nz)))
    first = with_set.step(x0, xs, obs)                              # uniform rows: the plain solve from the zero start, bit for bit
    assert bits(first["z"], cold["z"]) and bits(first["status"], cold["status"]) and bits(first["u0"], cold["z"][:, :2])
    bs.set_time_grid(np.full(30, 0.1))
    with pytest.raises(MpcbError) as e:
        with_set.step(x0, xs, obs)
    assert e.value.code == _abi.E_UNSUPPORTED
    bs.set_time_grid(None)
    ps4.close()
    with pytest.raises(MpcbError) as e:
        with_set.step(x0, xs, obs)
    assert e.value.code == _abi.E_INVALID and (with_set.ptr is not None)
    with pytest.raises(MpcbError) as e:
        with_set.reset()
    assert e.value.code == _abi.E_INVALID
    with_set.close(); with_set.close()                              # destroying it still works, twice is harmless
    ps8.close()
    # a destroyed loop is an error code, not a read of freed memory
    gone = loop.ptr
    loop.close()
    assert L.mpcb_loop_reset(bs._h, gone, None) == _abi.E_INVALID and L.mpcb_loop_destroy(bs._h, gone) == _abi.E_INVALID
    # a device group
    live = bs.loop(4)
    bs.set_devices([0])
    with pytest.raises(MpcbError) as e:
        live.step(x0, xs, obs)
    assert e.value.code == _abi.E_UNSUPPORTED
    with pytest.raises(MpcbError) as e:
        bs.loop(4)
    assert e.value.code == _abi.E_UNSUPPORTED
    for d in (d_x0, d_u0):
        d.free()
    bs.close()                                                      # with `live` alive: freed by mpcb_destroy
    live.close()                                                    # the solver is gone: nothing left to do
    foreign.step(x0, xs, obs)
    other.close()                                                   # with `foreign` alive


# ---- the integration example ----------------------------------------------------------------------------------------------------------------------
def test_sim_driver_with_an_external_plant(capsys):
    """sim/main_cbf_kin_c_sim.py --external-plant: the reference's scene through ControlLoop.step, plant and obstacles in the driver."""
    from mpc_motion_planning_amd.sim import main_cbf_kin_c_sim as drv
    xh, uh = drv.main(["--external-plant", "--sim-time", "0.8"])
    out = capsys.readouterr().out
    assert xh.shape == (9, 4) and uh.shape == (8, 2) and np.isfinite(xh).all() and np.isfinite(uh).all()
    assert "external plant: 8 steps" in out and "held steps" in out
    assert 8.0 < xh[-1, 0] - xh[0, 0] < 16.0 and np.abs(uh[:, 0]).max() <= 35 * np.pi / 180 + 1e-9       # ~15 m/s for 0.8 s, steering inside its box
