"""Non-default problem data and solver options on the device: every case of tests/config_cases.py through the compiled kernels
(BatchSolver.solve_batch) against the CPU oracle at B = 256, with the independent certificate of oracle/kkt_check.py built from the
config alone; the YAML route of the drop-in class, closed loops with a changed vehicle, the status cases, and the data-perturbing
pass of tools/fuzz_gpu_vs_oracle.py.  The CPU tier of the same table is tests/test_config_cpu.py.  Run with `-m gpu -s` to see the
measured margins (DESIGN.md §5.6 records them)."""
import os

import numpy as np
import pytest

from mpc_motion_planning_amd import scenes, _abi
from mpc_motion_planning_amd.solver import default_config, model_rhs
from tests import config_cases as cc
from tests.test_gpu_parity import agree, other_basin_allowance, TOL_Z, TOL_Z_DYN, _shift_plan, _teacher_forced_replay

pytestmark = pytest.mark.gpu


def _tol(case):
    return TOL_Z_DYN if case.model == _abi.MODEL_DYN else TOL_Z


@pytest.mark.parametrize("case", cc.SOLVE_CASES, ids=cc.ids(cc.SOLVE_CASES))
def test_case_on_device_against_oracle_and_certificate(gpu_solver_factory, oracle_mod, case):
    """One case of the table at B = 256 under the thresholds of test_every_kernel_instantiation_full_outputs: statuses equal on
    >= 0.975, at most 2 % of the instances solved on both sides in another basin and each of those certified, iteration counts equal
    on >= 0.95, lam_g to 1e-4 relative and the objective to 1e-8 (on the instances within the oracle's basin: a point in another
    basin has other multipliers by definition), and the from_config certificate on the first 24 device-solved instances."""
    cfg = cc.base(case, default_config)
    x0, xs, obs, xr = cc.scenes(case)
    assert len(x0) == cc.GPU_BATCH == 256
    g = gpu_solver_factory(cfg).solve_batch(x0, xs, obs, multipliers=True, x_ref=xr)
    r = oracle_mod.solve(cfg, x0, xs, obs, x_ref=xr)
    print("case %s:" % case.name)
    both = agree(g, r, tol=_tol(case), min_same_status=0.975, certify=lambda b: cc.certify(case, cfg, x0, xs, obs, xr, g, b))
    same_iters = (g["iters"][both] == r["iters"][both]).mean()
    sc = np.maximum(1.0, np.abs(r["lam_g"][both]).max(axis=1, keepdims=True))
    d_lam = (np.abs(g["lam_g"][both] - r["lam_g"][both]) / sc).max(axis=1)
    d_obj = np.abs(g["obj"][both] / r["obj"][both] - 1)
    near = np.abs(g["z"][both] - r["z"][both]).max(axis=1) <= _tol(case)           # multipliers and objective: within the oracle's basin
    print("case %s: oracle alone solved %.4f, lam_g rel %.2e, obj rel %.2e" % (case.name, (r["status"] == 0).mean(), d_lam[near].max(), d_obj[near].max()))
    assert same_iters >= 0.95
    assert d_lam[near].max() <= 1e-4
    assert d_obj[near].max() <= 1e-8
    solved = np.nonzero(g["status"] == 0)[0][:24]
    assert len(solved) == 24
    worst = dict(stationarity=0.0, feas_g=0.0, feas_x=0.0, compl=0.0)
    for b in solved:
        c = cc.certify(case, cfg, x0, xs, obs, xr, g, int(b))
        assert c["feas_x"] <= 1e-7, (case.name, b, c)
        for k in worst:
            worst[k] = max(worst[k], float(c[k] / (c["lam_scale"] if k == "stationarity" else 1.0)))
    print("case %s: certificate, worst over 24: %s" % (case.name, worst))


@pytest.mark.parametrize("case", cc.STATUS_CASES, ids=cc.ids(cc.STATUS_CASES))
def test_status_case_on_device(gpu_solver_factory, oracle_mod, case):
    """max_iter and the acceptable_* family: the device ends with the oracle's status on >= 0.975 of the batch and never runs past max_iter."""
    cfg = cc.base(case, default_config)
    x0, xs, obs, xr = cc.scenes(case)
    g = gpu_solver_factory(cfg).solve_batch(x0, xs, obs, x_ref=xr)
    r = oracle_mod.solve(cfg, x0, xs, obs, x_ref=xr, want_multipliers=False)
    same = (g["status"] == r["status"]).mean()
    print("case %s: status agreement %.4f, device statuses %s, iteration counts equal on %.4f, max iters %d"
          % (case.name, same, dict(zip(*[a.tolist() for a in np.unique(g["status"], return_counts=True)])), (g["iters"] == r["iters"]).mean(), g["iters"].max()))
    assert same >= 0.975
    assert (r["status"] == case.expect).mean() >= 0.95 and (g["status"] == case.expect).mean() >= 0.95
    attempts = 1 if cfg.second_start == 0 else 2                   # `iters` counts both attempts, each has max_iter of its own
    assert g["iters"].max() <= attempts * cfg.max_iter
    if case.expect == _abi.ST_MAXITER:
        assert (g["iters"][g["status"] == _abi.ST_MAXITER] == cfg.max_iter).all()
    else:
        ok = (g["status"] == case.expect) & (r["status"] == case.expect)
        far = (np.abs(g["z"][ok] - r["z"][ok]).max(axis=1) > TOL_Z).sum()
        assert far <= other_basin_allowance(ok.sum()) and (g["iters"][ok] == r["iters"][ok]).mean() >= 0.95


def test_limits_edited_in_the_yaml_reach_the_kernel(oracle_mod, tmp_path, monkeypatch):
    """A user's route to other limits: the package's mpc_parameters.yaml edited (steering, acceleration, y and steering-rate limits),
    MPC_optimize().initialize_constraints -> optimize_problem -> solver(...), against the oracle configured with the same bounds; and
    the limits hold on the returned trajectory."""
    from mpc_motion_planning_amd import MPC_CBF_optimize_kin
    src = os.path.join(os.path.dirname(__file__), "..", "mpc_motion_planning_amd", "sim", "mpc_parameters.yaml")
    text = open(src).read()
    for old, new in (("horizon: 5", "horizon: 3"), ("df_max: 35", "df_max: 20"), ("df_min: -35", "df_min: -2.0"), ("ax_max: 3.0", "ax_max: 1.2"),
                     ("ax_min: -3.0", "ax_min: -2.0"), ("Y_max: 5", "Y_max: 6"), ("Y_min: -1", "Y_min: -0.5"), ("df_dot_min: -5", "df_dot_min: -3"),
                     ("df_dot_max: 5", "df_dot_max: 6")):
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    (tmp_path / "mpc_parameters.yaml").write_text(text)
    monkeypatch.chdir(tmp_path)
    m = MPC_CBF_optimize_kin.MPC_optimize()
    N = m.N_p
    assert N == 30
    deg = np.pi / 180
    cfg = default_config(N=30, n_obs=1); cfg.second_start = 2            # what the drop-in classes configure (_mpc_base.py)
    cfg.u_lo[0], cfg.u_hi[0], cfg.u_lo[1], cfg.u_hi[1] = -2.0 * deg, 20 * deg, -2.0, 1.2
    cfg.x_lo[1], cfg.x_hi[1] = -0.5, 6.0
    cfg.du_lo[0], cfg.du_hi[0] = -3 * deg * 0.1, 6 * deg * 0.1
    obs = np.array([[50, 3.5, 0, 8, 4.8, 1.8]])
    lbg, ubg, lbx, ubx = m.initialize_constraints(obs)
    assert lbx[0] == -2.0 * deg and ubx[1] == 1.2 and lbx[2 * N + 1] == -0.5 and ubg[4 * (N + 1)] == 6 * deg * 0.1
    xs = np.array([400, 3.5, 0, 30.0]).reshape(-1, 1)
    n_solved = 0
    for x0v in ([0, 3, 0, 15.0], [10, 0.5, 0.05, 22.0], [20, 4.2, -0.05, 9.0]):
        x0 = np.array(x0v).reshape(-1, 1)
        solver = m.optimize_problem(ego_state=x0, ref_state=None, obstacle=obs)
        res = solver(x0=np.zeros((184, 1)), p=np.concatenate((x0, xs)), lbg=lbg, lbx=lbx, ubg=ubg, ubx=ubx)
        ref = oracle_mod.solve(cfg, x0.T, xs.T, obs[None], z0=np.zeros((1, 184)))
        z = res["x"].full()[:, 0]
        assert solver.stats()["status_code"] == ref["status"][0], (x0v, solver.stats(), ref["status"])
        if ref["status"][0] != 0:
            continue
        n_solved += 1
        err = np.abs(z - ref["z"][0]).max()
        print("YAML route, x0 = %s: L-inf vs oracle %.2e, iters %d / %d" % (x0v, err, solver.stats()["iter_count"], ref["iters"][0]))
        assert err <= TOL_Z
        U = z[:2 * N].reshape(N, 2); X = z[2 * N:].reshape(N + 1, 4)
        assert U[:, 0].min() >= -2.0 * deg - 1e-7 and U[:, 0].max() <= 20 * deg + 1e-7 and U[:, 1].min() >= -2.0 - 1e-7 and U[:, 1].max() <= 1.2 + 1e-7
        assert X[:, 1].min() >= -0.5 - 1e-7 and X[:, 1].max() <= 6.0 + 1e-7
        d = np.diff(U[:, 0])
        assert d.min() >= -3 * deg * 0.1 - 1e-7 and d.max() <= 6 * deg * 0.1 + 1e-7
        dflt = oracle_mod.solve(default_config(N=30, n_obs=1), x0.T, xs.T, obs[None])
        assert np.abs(dflt["z"][0] - z).max() > 1e-3                    # the edited limits bind: not the default problem's solution
    assert n_solved >= 2


def test_kinematic_closed_loop_with_another_wheelbase_and_step(gpu_solver_factory, oracle_mod):
    """mpcb_closed_loop with veh_l = 3.1 and T = 0.15, 16 scenes x 8 steps, replayed from the host teacher-forced (as
    test_gpu_parity._teacher_forced_replay does, with the right-hand side taken from the config): status, iteration count and applied
    control bit for bit, the plant step x + T f(x, U_0) with the config's wheelbase and step, and the oracle on every solve."""
    cfg = default_config(N=30, T=0.15, n_obs=1); cfg.veh_l = 3.1
    bs = gpu_solver_factory(cfg)
    B, steps = 16, 8
    x0, xs, obs = scenes.sample_c2(B, seed=21)
    x0[:, 0] = np.minimum(x0[:, 0], 10.0)
    dev = bs.closed_loop(x0, xs, obs, steps=steps)

    def rhs(x, u):
        return np.stack([x[:, 3] * np.cos(x[:, 2]), x[:, 3] * np.sin(x[:, 2]), x[:, 3] * np.tan(u[:, 0]) / cfg.veh_l, u[:, 1]], axis=1)
    z0 = np.zeros((B, bs.nz)); same = 0; far = 0; n_both = 0
    for t in range(steps):
        xc = dev["x_hist"][:, t].copy()
        g = bs.solve_batch(xc, xs, obs, z0=z0)
        assert np.array_equal(g["status"], dev["status"][:, t]) and np.array_equal(g["iters"], dev["iters"][:, t]), "step %d" % t
        assert np.array_equal(g["z"][:, :2], dev["u_hist"][:, t], equal_nan=True), "step %d: applied control" % t
        xn = xc + cfg.T * rhs(xc, g["z"][:, :2])
        fin = np.isfinite(xn).all(axis=1)
        assert np.abs(xn[fin] - dev["x_hist"][fin, t + 1]).max() <= 1e-10, "step %d: plant step" % t
        wrong = xc + 0.1 * np.stack([xc[:, 3] * np.cos(xc[:, 2]), xc[:, 3] * np.sin(xc[:, 2]), xc[:, 3] * np.tan(g["z"][:, 0]) / 2.6, g["z"][:, 1]], axis=1)
        assert np.abs(wrong[fin] - dev["x_hist"][fin, t + 1]).max() > 1e-3        # the default wheelbase and step would be seen
        for i in np.nonzero(fin)[0][:4]:
            assert np.abs(xc[i] + cfg.T * model_rhs(cfg, xc[i], g["z"][i, :2]) - dev["x_hist"][i, t + 1]).max() <= 1e-10
        r = oracle_mod.solve(cfg, xc, xs, obs, z0=z0, want_multipliers=False)
        same += int((r["status"] == g["status"]).sum())
        both = (r["status"] == 0) & (g["status"] == 0)
        e_ = np.abs(r["z"][both, :2] - g["z"][both, :2]).max(axis=1)
        far += int((e_ > TOL_Z).sum()); n_both += int(both.sum())
        z0 = _shift_plan(g["z"], cfg.N, 4)
    print("kinematic closed loop veh_l 3.1, T 0.15: status agreement with the oracle %.4f over %d solves, %d of %d in another basin, all-solved scenes %d"
          % (same / (B * steps), B * steps, far, n_both, (dev["status"] == 0).all(axis=1).sum()))
    assert same / (B * steps) >= 0.97 and far <= other_basin_allowance(n_both)
    assert (dev["status"] == 0).all(axis=1).sum() >= 8


def test_dynamic_closed_loop_with_another_vehicle(gpu_solver_factory, oracle_mod):
    """mpcb_closed_loop with the changed vehicle and tyres of the dyn_vehicle case, six steps: replayed teacher-forced (bit for bit, and
    the oracle on every solve) and every plant step against solver.model_rhs(cfg, ...)."""
    case = cc.BY_NAME["dyn_vehicle"]
    cfg = cc.base(case, default_config)
    bs = gpu_solver_factory(cfg)
    B, steps = 8, 6
    x0, xs, obs = scenes.sample_c4(B, seed=31, n_obs=1)
    dev = bs.closed_loop(x0, xs, obs, steps=steps)
    frac, n = _teacher_forced_replay(bs, cfg, dev, x0, xs, obs, steps, _abi.OBSMOVE_STATIC, oracle_mod)
    print("dynamic closed loop, changed vehicle: status agreement with the oracle %.4f over %d solves" % (frac, n))
    assert frac >= 0.97
    good = (dev["status"] == 0).all(axis=1)
    assert good.sum() >= 6
    dflt = default_config(model=_abi.MODEL_DYN, N=20, n_obs=1)
    moved = 0.0
    for i in np.nonzero(good)[0]:
        for t in range(steps):
            x, u = dev["x_hist"][i, t], dev["u_hist"][i, t]
            assert np.abs(x + cfg.T * model_rhs(cfg, x, u) - dev["x_hist"][i, t + 1]).max() <= 1e-10
            moved = max(moved, np.abs(model_rhs(cfg, x, u) - model_rhs(dflt, x, u)).max())
    assert moved > 1e-4                                                   # the default vehicle's step would be seen


def test_fuzzed_structures_with_perturbed_data_against_oracle(gpu_solver_factory):
    """tools/fuzz_gpu_vs_oracle.py with perturb_data: 24 random NLP structures whose weights, bounds, geometry and vehicle parameters
    are drawn within about +-40 % of the defaults, under the tool's own acceptance rule."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_gpu_vs_oracle", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_gpu_vs_oracle.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    assert mod.run(cases=24, seed=23, verbose=True, perturb_data=True) == 0
