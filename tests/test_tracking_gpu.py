"""Per-stage reference tracking on the MI355X (mpcb_solve_ref / mpcb_solve_device_ref / mpcb_closed_loop_ref, the mpcb_track_*
kernels).  The oracle has no tracking cost: the evidence is the equivalence with the set-point solve (rows equal to xs), the CPU
stepping of the same kernel source (tests/emu), the independent KKT certificate of oracle/kkt_check.py with the tracking
objective, and a host-driven replay of the tracking closed loop."""
import numpy as np
import pytest

from mpc_motion_planning_amd import scenes, _abi
from mpc_motion_planning_amd.solver import default_config

pytestmark = pytest.mark.gpu


def rows_of(xs, N):
    return np.ascontiguousarray(np.repeat(np.asarray(xs, dtype=np.float64)[:, None, :], N, axis=1))


def random_refs(x0, N, T, rng):
    """Ramps in y between the lane centres (0 and 3.5) and speed steps: one per instance, chosen at random."""
    B = len(x0)
    i = np.arange(N)[None, :]
    y_from = np.where(x0[:, 1] > 1.75, 3.5, 0.0)
    y_to = np.where(rng.random(B) < 0.5, 3.5 - y_from, y_from)
    start = rng.integers(0, 12, B)[:, None]; length = rng.integers(8, 20, B)[:, None]
    v_from = x0[:, 3:4]; v_to = rng.uniform(8.0, 30.0, (B, 1)); at = rng.integers(3, N - 3, B)[:, None]
    v = np.where(i < at, v_from, v_to)
    r = np.zeros((B, N, 4))
    r[:, :, 0] = x0[:, :1] + T * np.cumsum(v, axis=1)
    r[:, :, 1] = y_from[:, None] + (y_to - y_from)[:, None] * np.clip((i - start) / length, 0.0, 1.0)
    r[:, :, 3] = v
    return r


def _equal_to_set_point(bs, x0, xs, obs, name):
    a = bs.solve_batch(x0, xs, obs)
    b = bs.solve_batch(x0, xs, obs, x_ref=rows_of(xs, bs.N))
    assert np.array_equal(a["status"], b["status"]), name
    assert np.array_equal(a["iters"], b["iters"]), name
    err = np.abs(a["z"] - b["z"]).max()
    assert err <= 1e-10, (name, err)
    bitwise = np.array_equal(a["z"], b["z"]) and np.array_equal(a["obj"], b["obj"])
    print("x_ref = xs vs set point, %s: B = %d, solved %d, z L-inf %.3e, bitwise %s" % (name, len(x0), (a["status"] == 0).sum(), err, bitwise))
    return bitwise


def test_reference_equal_to_set_point_gives_the_set_point_solve(gpu_solver_factory):
    bits = []
    cfg = default_config(N=30, n_obs=1)
    x0, xs, obs = scenes.sample_c2(512, seed=101)
    bits.append(_equal_to_set_point(gpu_solver_factory(cfg), x0, xs, obs, "C2 kin<1>"))
    cfg = default_config(N=30, n_obs=3)
    x0, xs, _, traj = scenes.sample_c3(512, N=30, dt=0.1, seed=102)
    bits.append(_equal_to_set_point(gpu_solver_factory(cfg), x0, xs, traj, "C3 kin<3>"))
    for n in (5, 8):
        cfg = default_config(N=30, n_obs=n)
        x0, xs, _, traj = scenes.sample_c3(64, N=30, dt=0.1, seed=103 + n, n_obs=n)
        bits.append(_equal_to_set_point(gpu_solver_factory(cfg), x0, xs, traj, "kin<%d>" % n))
    x0, xs, obs = scenes.sample_c2(128, seed=104)
    cfg = default_config(N=30, n_obs=1); cfg.obs_mode = _abi.OBS_DCBF; cfg.gamma = 0.5
    bits.append(_equal_to_set_point(gpu_solver_factory(cfg), x0, xs, obs, "GEN<1>"))
    cfg = default_config(N=30, n_obs=1); cfg.integrator = _abi.INT_RK4
    bits.append(_equal_to_set_point(gpu_solver_factory(cfg), x0, xs, obs, "RK4<1>"))
    for ss in (0, 1, 2, 3):
        cfg = default_config(N=30, n_obs=1); cfg.second_start = ss
        bits.append(_equal_to_set_point(gpu_solver_factory(cfg), x0, xs, obs, "second_start %d" % ss))
    print("bitwise equal in %d of %d batches" % (sum(bits), len(bits)))


def test_tracking_kernel_equals_its_cpu_stepping(gpu_solver_factory):
    from tests.emu import emu
    from oracle import oracle
    B = 16
    x0, xs, obs = scenes.sample_c2(B, seed=111)
    xr = random_refs(x0, 30, 0.1, np.random.default_rng(3))
    g = gpu_solver_factory(default_config(N=30, n_obs=1)).solve_batch(x0, xs, obs, x_ref=xr)
    c = oracle.default_config(N=30, n_obs=1)
    c.init_rollout = 1; c.mu_init = 10.0; c.second_start = 3; c.start_steer = 0.03
    e = emu.solve(c, x0, xs, obs, x_ref=xr)
    assert np.array_equal(g["status"], e["status"]) and np.array_equal(g["iters"], e["iters"])
    assert (g["status"] == 0).sum() >= B // 2
    assert np.abs(g["z"] - e["z"]).max() <= 1e-9


@pytest.mark.parametrize("kind", ["C2", "C3"])
def test_random_references_pass_the_kkt_certificate(gpu_solver_factory, kind):
    from oracle import kkt_check
    rng = np.random.default_rng(7 if kind == "C2" else 8)
    if kind == "C2":
        cfg = default_config(N=30, n_obs=1)
        x0, xs, obs = scenes.sample_c2(512, seed=121)
    else:
        cfg = default_config(N=30, n_obs=3)
        x0, xs, _, obs = scenes.sample_c3(512, N=30, dt=0.1, seed=122)
    xr = random_refs(x0, 30, 0.1, rng)
    r = gpu_solver_factory(cfg).solve_batch(x0, xs, obs, x_ref=xr, multipliers=True)
    ok = np.nonzero(r["status"] == 0)[0]
    print("%s tracking: solved %d of %d (%.1f %%), statuses %s" % (kind, len(ok), len(x0), 100.0 * len(ok) / len(x0),
                                                                   np.bincount(r["status"], minlength=9).tolist()))
    assert len(ok) >= 256
    for b in ok[:256]:
        nlp = kkt_check.KinNlp(30, 0.1, x0[b], xs[b], obs[b]); nlp.xs = xr[b]
        c = kkt_check.certificate(nlp, r["z"][b], r["lam_g"][b], r["lam_x"][b])
        assert c["stationarity"] <= 1e-6 * c["lam_scale"] and c["feas_g"] <= 2e-8 and c["compl"] <= 1e-3 and c["sign"] == 0.0, (b, c)


def test_results_do_not_depend_on_inflight(gpu_solver_factory):
    cfg = default_config(N=30, n_obs=1)
    B = 256
    x0, xs, obs = scenes.sample_c2(B, seed=131)
    xr = random_refs(x0, 30, 0.1, np.random.default_rng(9))
    out = []
    for k in (1, 16):
        bs = gpu_solver_factory(cfg, inflight=k)
        d = [bs.device_array(a.shape).upload(a) for a in (x0, xs, xr, obs)]
        zs = []
        for rep in range(3):                                    # three asynchronous launches: on 3 lanes with k = 16
            dz = bs.device_array((B, bs.nz)); dst = bs.device_array((B,), np.int32); dit = bs.device_array((B,), np.int32)
            bs.solve_device(B, d[0], d[1], d[3], _abi.OBSIN_STATIC, None, dz, d_status=dst, d_iters=dit, d_x_ref=d[2])
            zs.append((dz, dst, dit))
        bs.sync()
        out.append([(z.download(), s.download(), i.download()) for z, s, i in zs])
    ref = out[0][0]
    for run in out:
        for z, s, i in run:
            assert np.array_equal(z, ref[0]) and np.array_equal(s, ref[1]) and np.array_equal(i, ref[2])
    host = gpu_solver_factory(cfg).solve_batch(x0, xs, obs, x_ref=xr)
    assert np.array_equal(host["z"], ref[0]) and np.array_equal(host["status"], ref[1])


def test_tracking_closed_loop_matches_the_host_loop(gpu_solver_factory):
    """closed_loop(aa = 0.5) against the same loop driven from the host (RefPathGenerator window with N_p = N at the device's own
    state, solve_batch(x_ref=...), plant step, shift), teacher-forced, every instance and step; closed_loop(aa = 0) is the set-point loop.
    The tracking oracle, given the same state, warm start and window at every step, ends with the same status on >= 99 % of the solves
    and with U_0 within 1e-5 wherever both solve (other basins within the allowance of agree()), as _teacher_forced_replay checks the
    set-point loop."""
    from oracle import oracle
    from tests.test_gpu_parity import other_basin_allowance
    from mpc_motion_planning_amd.RefPathGenerator import RefPathGenerator
    from mpc_motion_planning_amd.shift import shift
    from mpc_motion_planning_amd._mpc_base import ModelFunction
    cfg = default_config(N=30, n_obs=1)
    bs = gpu_solver_factory(cfg)
    N, T, aa = cfg.N, cfg.T, 0.5
    B, steps = 16, 12
    x0, xs, obs = scenes.sample_c2(B, seed=141)
    x0[:, 0] = np.minimum(x0[:, 0], 10.0)
    dev = bs.closed_loop(x0, xs, obs, steps=steps, aa=aa)
    f = ModelFunction(bs.cfg)
    paths = [RefPathGenerator() for _ in range(B)]
    for b in range(B):
        paths[b].define_ref_path(x0[b], xs[b], T)
    last = [0] * B
    z0 = np.zeros((B, bs.nz))
    same = total = far = n_both = 0; worst = 0.0
    for t in range(steps):
        xc = dev["x_hist"][:, t].copy()
        xr = np.zeros((B, N, 4))
        for b in range(B):
            win, last[b] = paths[b].find_ref_traj(xc[b], xs[b], N * T, T, last[b], N_p=N)
            xr[b] = aa * win[1:] + (1 - aa) * xs[b]
        g = bs.solve_batch(xc, xs, obs, z0=z0, x_ref=xr)
        r = oracle.solve(cfg, xc, xs, obs, z0=z0, x_ref=xr, want_multipliers=False)
        same += int((r["status"] == g["status"]).sum()); total += B
        both = (r["status"] == 0) & (g["status"] == 0)
        if both.any():
            e_ = np.abs(r["z"][both, :2] - g["z"][both, :2]).max(axis=1)
            far += int((e_ > 1e-5).sum()); n_both += int(both.sum())
            worst = max(worst, float(e_[e_ <= 1e-5].max()) if (e_ <= 1e-5).any() else 0.0)
        assert np.array_equal(g["status"], dev["status"][:, t]), t
        assert np.array_equal(g["iters"], dev["iters"][:, t]), t
        assert np.array_equal(g["z"][:, :2], dev["u_hist"][:, t]), t
        for b in range(B):
            U = g["z"][b, :2 * N].reshape(N, 2); X = g["z"][b, 2 * N:].reshape(N + 1, 4)
            _, xn, u_sh, x_sh = shift(T, 0.0, xc[b], U, X, f)
            if np.isfinite(xn).all():
                assert np.abs(xn[:, 0] - dev["x_hist"][b, t + 1]).max() <= 1e-10, (t, b)
            z0[b] = np.concatenate([u_sh.reshape(-1), x_sh.reshape(-1)])
    print("tracking closed loop vs oracle: status agreement %.4f over %d solves, U_0 worst L-inf %.2e, %d of %d in another basin"
          % (same / total, total, worst, far, n_both))
    assert same / total >= 0.99 and far <= other_basin_allowance(n_both), (same / total, far, n_both)
    assert (dev["status"] == 0).all(axis=1).sum() >= 8
    base = bs.closed_loop(x0, xs, obs, steps=steps)
    zero = bs.closed_loop(x0, xs, obs, steps=steps, aa=0.0)
    for k in ("x_hist", "u_hist", "status", "iters"):
        assert np.array_equal(base[k], zero[k]), k
    assert not np.array_equal(base["x_hist"], dev["x_hist"])           # the window does pull the loop elsewhere


def test_unsupported_and_invalid_requests_return_their_codes(gpu_solver_factory):
    from mpc_motion_planning_amd._lib import MpcbError
    x0, xs, obs = scenes.sample_c2(4, seed=151)
    bs = gpu_solver_factory(default_config(N=30, n_obs=1))
    for aa in (-0.1, 1.5, float("nan")):
        with pytest.raises(MpcbError) as e:
            bs.closed_loop(x0, xs, obs, steps=2, aa=aa)
        assert e.value.code == _abi.E_INVALID
    bs.set_time_grid(np.full(30, 0.1))
    with pytest.raises(MpcbError) as e:
        bs.closed_loop(x0, xs, obs, steps=2, aa=0.5)
    assert e.value.code == _abi.E_UNSUPPORTED
    bs.set_time_grid(None)
    assert (bs.solve_batch(x0, xs, obs, x_ref=rows_of(xs, 30))["status"] >= 0).all()     # the handle still works
    dyn = gpu_solver_factory(default_config(model=_abi.MODEL_DYN, N=20, n_obs=0))
    d0 = np.tile(scenes.DYN_X0, (2, 1)); ds = np.tile(scenes.DYN_XS, (2, 1))
    with pytest.raises(MpcbError) as e:
        dyn.solve_batch(d0, ds, x_ref=rows_of(ds, 20))
    assert e.value.code == _abi.E_UNSUPPORTED
    with pytest.raises(MpcbError) as e:
        dyn.closed_loop(d0, ds, steps=2, aa=0.5)
    assert e.value.code == _abi.E_UNSUPPORTED
    grp = gpu_solver_factory(default_config(N=30, n_obs=1))
    grp.set_devices([0])
    with pytest.raises(MpcbError) as e:
        grp.solve_batch(x0, xs, obs, x_ref=rows_of(xs, 30))
    assert e.value.code == _abi.E_UNSUPPORTED


def test_drop_in_with_aa_follows_the_window_on_the_shipped_scene():
    """mpc.aa = 0.5 on the reference's scene at its shipped horizon (N_p = 50): every step solves, the car passes the obstacle and
    returns to the lane centre at the path's speed instead of accelerating toward the set-point x = 400."""
    from mpc_motion_planning_amd.sim import main_cbf_kin_c_sim
    xh, uh = main_cbf_kin_c_sim.main(["--aa", "0.5", "--sim-time", "6.0"])
    h = ((xh[:, 0] - 50) / 5.8) ** 2 + ((xh[:, 1] - 3.5) / 2.3) ** 2 - 1
    assert h.min() >= -1e-6 and xh[-1, 0] > 60.0                    # past the obstacle without touching it
    assert abs(xh[-1, 1] - 3.5) < 0.5                                # back near the lane centre
    base_xh, _ = main_cbf_kin_c_sim.main(["--sim-time", "6.0"])
    assert xh[-1, 3] < base_xh[-1, 3]                                # the window's preview speed, not the set-point's 30 m/s dash


# ----- every tracking kernel against the tracking oracle (oracle.solve(x_ref=...)) ------------------------------------------------

def _refs(x0, N, T, rng):
    """random_refs for any horizon: the first N stages of a 30-stage lane ramp / speed step when N < 30."""
    return np.ascontiguousarray(random_refs(x0, max(N, 30), T, rng)[:, :N])


def _scene(n_obs, B, seed, N=30, c3=False):
    if n_obs <= 1 and not c3:
        x0, xs, obs = scenes.sample_c2(B, seed=seed)
        return x0, xs, obs[:, :n_obs]
    x0, xs, _, traj = scenes.sample_c3(B, N=N, dt=0.1, seed=seed, n_obs=max(n_obs, 1))
    return x0, xs, traj[:, :n_obs]


def _against_oracle(gpu_solver_factory, cfg, x0, xs, obs, xr, name, z0=None, tgrid=None, min_same_status=0.975, full=True):
    """The tracking solve on the device against the tracking oracle: agree() (instances in another basin certified, where KinNlp
    expresses the NLP), equal iteration counts on >= 95 % of the instances solved on both sides, and with full = True lam_g, lam_x and
    the objective with the thresholds of test_every_kernel_instantiation_full_outputs."""
    from oracle import oracle
    from tests.test_gpu_parity import agree, kin_certifier
    o = obs if cfg.n_obs else None
    bs = gpu_solver_factory(cfg)
    if tgrid is not None:
        bs.set_time_grid(tgrid)
    g = bs.solve_batch(x0, xs, o, z0=z0, multipliers=True, x_ref=xr)
    r = oracle.solve(cfg, x0, xs, o, z0=z0, x_ref=xr, tgrid=tgrid)
    print("tracking vs oracle, %s: B = %d, statuses gpu %s oracle %s" % (name, len(x0), np.bincount(g["status"], minlength=9).tolist(),
                                                                          np.bincount(r["status"], minlength=9).tolist()))
    both = agree(g, r, min_same_status=min_same_status, certify=None if tgrid is not None else kin_certifier(cfg, x0, xs, obs, g, xr))
    assert (g["iters"][both] == r["iters"][both]).mean() >= 0.95, name
    near = both & (np.abs(g["z"] - r["z"]).max(axis=1) <= 1e-5)
    if full:
        sc_g = np.maximum(1.0, np.abs(r["lam_g"][near]).max(axis=1, keepdims=True))
        assert (np.abs(g["lam_g"][near] - r["lam_g"][near]) / sc_g).max() <= 1e-4, name
        sc_x = np.maximum(1.0, np.abs(r["lam_x"][near]).max(axis=1, keepdims=True))
        assert (np.abs(g["lam_x"][near] - r["lam_x"][near]) / sc_x).max() <= 1e-3, name
        assert np.abs(g["obj"][near] / r["obj"][near] - 1).max() <= 1e-8, name
    return g, r


TRACK_KERNELS = [("kin<0>", 0, ""), ("kin<1>", 1, ""), ("kin<3> (2 obstacles)", 2, ""), ("kin<3>", 3, ""), ("kin<5>", 5, ""),
                 ("kin<8>", 8, ""), ("kin<1, GEN>", 1, "gen"), ("kin<3, GEN>", 3, "gen"), ("kin<8, GEN>", 8, "gen"),
                 ("kin<0, RK4>", 0, "rk4"), ("kin<1, RK4>", 1, "rk4"), ("kin<3, RK4>", 3, "rk4")]


@pytest.mark.parametrize("name,n_obs,kind", TRACK_KERNELS, ids=[k[0] for k in TRACK_KERNELS])
def test_every_tracking_instantiation_full_outputs(gpu_solver_factory, name, n_obs, kind):
    """Each main tracking kernel as mpcb_api.hip dispatches it, 96 instances with random lane ramps and speed steps, every output
    array against the tracking oracle."""
    cfg = default_config(N=30, n_obs=n_obs)
    if kind == "gen":
        cfg.obs_mode = _abi.OBS_DCBF; cfg.gamma = 0.5
    if kind == "rk4":
        cfg.integrator = _abi.INT_RK4
    x0, xs, obs = _scene(n_obs, 96, 600 + 10 * n_obs + len(kind), c3=kind == "gen")
    xr = random_refs(x0, 30, 0.1, np.random.default_rng(600 + n_obs))
    _against_oracle(gpu_solver_factory, cfg, x0, xs, obs, xr, name)


@pytest.mark.parametrize("N", [1, 2, 20, 33, 50, 63])
def test_tracking_horizons_against_the_oracle(gpu_solver_factory, N):
    """kin<1> at horizons where the lane layout changes: N = 1, 2 (no rate rows at N = 1), 33 (past 32 lanes), 63 (the last lane is
    the terminal node, the row copy into LDS takes four trips)."""
    cfg = default_config(N=N, n_obs=1)
    x0, xs, obs = _scene(1, 64, 700 + N)
    xr = _refs(x0, N, 0.1, np.random.default_rng(700 + N))
    _against_oracle(gpu_solver_factory, cfg, x0, xs, obs, xr, "N = %d" % N, min_same_status=0.98)


def test_tracking_warm_start_against_the_oracle(gpu_solver_factory):
    """The next step of a receding horizon: the shifted plan of a solved batch as z0, X_1 as x0, the next stage window as x_ref."""
    from tests.test_gpu_parity import _shift_plan
    cfg = default_config(N=30, n_obs=1)
    x0, xs, obs = _scene(1, 128, 711)
    path = random_refs(x0, 31, 0.1, np.random.default_rng(711))
    first = gpu_solver_factory(cfg).solve_batch(x0, xs, obs, x_ref=path[:, :30])
    ok = np.nonzero(first["status"] == 0)[0][:96]
    assert len(ok) >= 64
    z0 = _shift_plan(first["z"][ok], 30, 4)
    x1 = first["z"][ok, 64:68].copy()
    g, r = _against_oracle(gpu_solver_factory, cfg, x1, xs[ok], obs[ok], path[ok, 1:], "warm start", z0=z0)
    assert np.median(g["iters"]) < np.median(first["iters"][ok])


@pytest.mark.parametrize("second_start", [0, 1, 2, 3])
def test_tracking_second_start_modes_against_the_oracle(gpu_solver_factory, second_start):
    cfg = default_config(N=30, n_obs=3); cfg.second_start = second_start
    x0, xs, obs = _scene(3, 96, 720 + second_start)
    xr = random_refs(x0, 30, 0.1, np.random.default_rng(720 + second_start))
    _against_oracle(gpu_solver_factory, cfg, x0, xs, obs, xr, "second_start %d" % second_start)


@pytest.mark.parametrize("n_obs", [1, 5, 8])
def test_tracking_restoration_twins_against_the_oracle(gpu_solver_factory, n_obs):
    """Batches in which the restoration pass runs (second_start = 0: the first attempt's own restoration pass), through the
    mpcb_track_kin_resto<1|5|8> kernels (always a launch of their own).  MPCB_ST_INFEASIBLE is a status only the restoration phase
    gives: the oracle reports it on these batches and the device must too."""
    from oracle import oracle
    cfg = default_config(N=30, n_obs=n_obs); cfg.second_start = 0
    x0, xs, obs = _scene(n_obs, 256, 500 + (n_obs if n_obs > 1 else 0))
    xr = random_refs(x0, 30, 0.1, np.random.default_rng(n_obs))
    g, r = _against_oracle(gpu_solver_factory, cfg, x0, xs, obs, xr, "restoration, n_obs %d" % n_obs, full=False)
    resto = (r["status"] == _abi.ST_INFEASIBLE) & (g["status"] == _abi.ST_INFEASIBLE)
    cfg.restoration = 0
    off = oracle.solve(cfg, x0, xs, obs, x_ref=xr, want_multipliers=False)
    print("restoration, n_obs %d: %d instances MPCB_ST_INFEASIBLE on both sides, %d end with MPCB_ST_LINESEARCH without the pass"
          % (n_obs, resto.sum(), (off["status"] == _abi.ST_LINESEARCH).sum()))
    assert resto.sum() >= 2 and (off["status"][resto] == _abi.ST_LINESEARCH).all()


def test_tracking_with_a_time_grid_against_the_oracle(gpu_solver_factory):
    """set_time_grid plus x_ref (mpcb_solve_ref accepts a grid) against oracle.solve(tgrid=..., x_ref=...)."""
    cfg = default_config(N=30, n_obs=1)
    tg = np.concatenate([np.full(24, 0.1), np.full(6, 0.5)])
    x0, xs, obs = _scene(1, 96, 731)
    xr = random_refs(x0, 30, 0.1, np.random.default_rng(731))
    _against_oracle(gpu_solver_factory, cfg, x0, xs, obs, xr, "time grid", tgrid=tg, min_same_status=0.98)
