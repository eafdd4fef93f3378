"""The restoration phase inside the lean launch on the device: two handles of one build, one created with MPCB_RESTO_IN_LAUNCH=0 in the
environment (every restoration phase in a launch of its own, as before), one without.  The restoration instantiation reads z, the status
and the hand-over record back from memory in both, so every output must be equal bit for bit; MPCB_ST_NEEDS_RESTO (7) never leaves a
solve.  With the rule on, the restoration launch of the plan still runs over the outputs afterwards and finds no instance to continue:
what the lean launch returned is what the caller gets.  The CPU tier is tests/test_resto_in_launch_cpu.py."""
import numpy as np
import pytest

from mpc_motion_planning_amd import scenes, _abi
from mpc_motion_planning_amd.solver import default_config

pytestmark = pytest.mark.gpu
OUT = ("z", "obj", "status", "iters", "kkt", "lam_g", "lam_x")
NEEDS_RESTO = 7


def straight_cfg(second_start, N=30, n_obs=1):
    """The straight roll-out start (cfg.start_steer = 0): the batches on which the restoration phase has work to do."""
    c = default_config(N=N, n_obs=n_obs)
    c.start_steer = 0.0; c.second_start = second_start
    return c


@pytest.fixture
def pair(gpu_solver_factory, monkeypatch):
    """pair(cfg, **kw) -> (handle with the rule, handle created under MPCB_RESTO_IN_LAUNCH=0)"""
    def make(cfg, **kw):
        monkeypatch.delenv("MPCB_RESTO_IN_LAUNCH", raising=False)
        on = gpu_solver_factory(cfg, **kw)
        monkeypatch.setenv("MPCB_RESTO_IN_LAUNCH", "0")
        off = gpu_solver_factory(cfg, **kw)
        monkeypatch.delenv("MPCB_RESTO_IN_LAUNCH")
        return on, off
    return make


def same_bits(a, b, name):
    for k in OUT:
        if k in a:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
    assert not (a["status"] == NEEDS_RESTO).any(), name


SEED3 = scenes.sample_c2(256, seed=3)


@pytest.mark.parametrize("second_start", [0, 1, 2, 3])
def test_both_handles_return_the_same_bits_and_the_oracles_statuses(pair, oracle_mod, second_start):
    """sample_c2(256, seed=3) from the straight start: about 70 instances use the restoration phase (the CPU tier counts them).  Status
    agreement with the oracle >= 0.96, the threshold tests/test_gpu_parity.py uses where many instances end through the restoration
    phase: one such instance in eight differs in status on rounding alone (tests/config_cases.py), 70 / 8 of 256 is 3.4 %."""
    x0, xs, obs = SEED3
    cfg = straight_cfg(second_start)
    on, off = pair(cfg)
    a = on.solve_batch(x0, xs, obs, multipliers=True); b = off.solve_batch(x0, xs, obs, multipliers=True)
    same_bits(a, b, "second_start %d" % second_start)
    r = oracle_mod.solve(cfg, x0, xs, obs, want_multipliers=False)
    same = (a["status"] == r["status"]).mean()
    print("second_start %d: statuses %s, status agreement with the oracle %.4f, iteration counts equal on %.4f"
          % (second_start, np.bincount(a["status"], minlength=9).tolist(), same, (a["iters"] == r["iters"]).mean()))
    assert same >= 0.96, same
    # a start vector: under second_start = 3 the plan becomes FIRST, RESTO, SECOND, RESTO and both lean launches restore in place
    z0 = np.zeros_like(a["z"]); z0[:, 0:60:2] = 0.01
    same_bits(on.solve_batch(x0, xs, obs, z0=z0), off.solve_batch(x0, xs, obs, z0=z0), "second_start %d, start vector" % second_start)


@pytest.mark.parametrize("second_start", [0, 3])
def test_tracking_and_parameter_set_entry_points(pair, second_start):
    x0, xs, obs = (a[:128] for a in SEED3)
    cfg = straight_cfg(second_start)
    on, off = pair(cfg)
    plain = on.solve_batch(x0, xs, obs, multipliers=True)
    x_ref = np.repeat(xs[:, None, :], 30, axis=1)
    rng = np.random.default_rng(5)
    x_ref[:, :, 1] += rng.uniform(-0.5, 0.5, (128, 1))                          # a reference beside the set-point
    same_bits(on.solve_batch(x0, xs, obs, multipliers=True, x_ref=x_ref), off.solve_batch(x0, xs, obs, multipliers=True, x_ref=x_ref), "tracking")
    with on.params([cfg] * 128) as p_on, off.params([cfg] * 128) as p_off:
        a = on.solve_batch(x0, xs, obs, multipliers=True, params=p_on)
        same_bits(a, off.solve_batch(x0, xs, obs, multipliers=True, params=p_off), "parameter set")
        same_bits(a, plain, "uniform rows against the plain solve")


def test_four_lanes_with_rotated_output_buffers(pair):
    """mpcb_solve_device on four lanes: every lane has its own hand-over records and the launches overlap."""
    x0, xs, obs = SEED3
    x1, _, ob1 = scenes.sample_c2(256, seed=8)
    cfg = straight_cfg(3)
    K, B = 4, 256
    got = []
    for h in pair(cfg, inflight=K):
        dx = [h.device_array((B, 4)).upload(a) for a in (x0, x1)]; dxs = h.device_array((B, 4)).upload(xs)
        dob = [h.device_array(a.shape).upload(a) for a in (obs, ob1)]
        ring = [dict(z=h.device_array((B, 184)), st=h.device_array((B,), np.int32), it=h.device_array((B,), np.int32)) for _ in range(K)]
        for j in range(2 * K + 1):
            q = ring[j % K]
            h.solve_device(B, dx[j % 2], dxs, dob[j % 2], _abi.OBSIN_STATIC, None, q["z"], None, q["st"], q["it"], None)
        h.sync()
        got.append([{k: q[k].download() for k in ("z", "st", "it")} for q in ring])
        h.set_inflight(1)
        ref = [h.solve_batch(x0, xs, obs), h.solve_batch(x1, xs, ob1)]
        for s_ in range(K):
            j_ = max(j for j in range(2 * K + 1) if j % K == s_)
            r = ref[j_ % 2]
            assert np.array_equal(got[-1][s_]["z"], r["z"]) and np.array_equal(got[-1][s_]["st"], r["status"]) and np.array_equal(got[-1][s_]["it"], r["iters"])
    for s_ in range(K):
        for k in ("z", "st", "it"):
            assert got[0][s_][k].tobytes() == got[1][s_][k].tobytes(), (s_, k)
        assert not (got[0][s_]["st"] == NEEDS_RESTO).any()


@pytest.mark.parametrize("N,B", [(50, 64), (1, 32), (2, 32), (63, 32)])
def test_other_horizons(pair, N, B):
    """N = 50: the restoration layout would cost the lean launch a workgroup per CU, the rule says no and the passes stay apart.  N = 1, 2,
    63: the shortest horizons and the longest."""
    x0, xs, obs = (a[:B] for a in SEED3)
    cfg = straight_cfg(0, N=N)
    on, off = pair(cfg)
    a = on.solve_batch(x0, xs, obs, multipliers=True)
    same_bits(a, off.solve_batch(x0, xs, obs, multipliers=True), "N = %d" % N)
    print("N = %d: statuses %s" % (N, np.bincount(a["status"], minlength=9).tolist()))
