"""The restoration phase inside the lean launch (mpcbd::resto_in_launch, mpc_motion_planning_amd/csrc/mpcb_dispatch.h) without a GPU: the
rule against a table written out here, and the kernel source stepped on the CPU (tests/emu_resto: the stepping of tests/emu with the
wrapper of the kernels that restore in place) with the rule forced on against forced off.  On: the wave that ends its last attempt
with MPCB_ST_NEEDS_RESTO calls the restoration instantiation at once, on the LDS of the restoration layout; off: the restoration pass is a pass of its own, as it was.  Every output must be equal bit for bit, and both must
agree with the oracle.  The device tier is tests/test_resto_in_launch_gpu.py."""
import itertools

import numpy as np
import pytest

from mpc_motion_planning_amd import _abi, scenes
from oracle import oracle
from tests import params_cases as pc
from tests.emu import emu
from tests.emu_resto import emu_resto

KIN, DYN = _abi.MODEL_KIN, _abi.MODEL_DYN
OUT = ("z", "obj", "status", "iters", "kkt", "lam_g", "lam_x")
CU_LDS = 160 * 1024


def product_cfg(N=30, n_obs=1, model=KIN):
    c = oracle.default_config(model=model, N=N, n_obs=n_obs)
    c.init_rollout = 1; c.mu_init = 10.0; c.second_start = 3; c.start_steer = 0.03        # the settings mpcb_default_config ships
    return c


def straight_cfg(second_start, N=30, n_obs=1):
    """The straight roll-out start (cfg.start_steer = 0): the batches on which the restoration phase has work to do."""
    c = product_cfg(N, n_obs); c.start_steer = 0.0; c.second_start = second_start
    return c


def dispatch(cfg, **kw):
    """What mpcb_dispatch.h decides for one solve (tests/emu), with the rule for its first launch (tests/emu_resto): resto_in_launch, lds_first."""
    d = emu.dispatch(cfg, **kw)
    if d["code"] == 0:
        r = emu_resto.dispatch(cfg, **kw)
        assert r["code"] == 0 and r["passes"] == d["passes"], (d, r)         # the passes stay pass_plan's
        d.update(r)
    return d


# ----- 1. the rule ---------------------------------------------------------------------------------------------------------------------

def test_rule_by_variant():
    """Yes for the Euler kin<0|1> kernels without general-gamma rows, plain, tracking and per-instance; no for kin<3|5|8>, GEN, RK4 and
    the dynamic model.  The passes stay pass_plan's, and the first launch gets the restoration layout's LDS exactly where the rule says yes."""
    seen_yes = set()
    for n, rows, rk4, use in itertools.product(range(9), ("keepout", "gamma_half"), (False, True), ("plain", "track", "params")):
        if rk4 and (n > 3 or rows == "gamma_half"):
            continue                                         # check_cfg lets neither through
        c = product_cfg(30, n)
        if rows == "gamma_half":
            c.obs_mode = _abi.OBS_DCBF; c.obs_terminal = 0; c.gamma = 0.5
        c.integrator = _abi.INT_RK4 if rk4 else _abi.INT_EULER
        d = dispatch(c, track=use == "track", params=use == "params")
        if d["code"] != 0:
            continue                                         # not shipped (tests/test_dispatch_cpu.py has the table)
        want = n <= 1 and not d["gen"] and not rk4
        assert d["resto_in_launch"] == want, (n, rows, rk4, use, d)
        assert d["lds_first"] == (d["lds_resto"] if want else d["lds"]), (n, rows, rk4, use, d)
        # a cold start under second_start = 3: MPCB_PASS_FIRST, (MPCB_PASS_SECOND where the kernel does not fuse,) MPCB_PASS_RESTO
        assert d["passes"] == ([0, 2] if d["fuses"] else [0, 1, 2]), d
        if want:
            seen_yes.add((d["capacity"], use))
    assert seen_yes == {(0, "plain"), (1, "plain"), (0, "track"), (1, "track"), (0, "params"), (1, "params")}
    for n in (1, 3, 5, 8):
        d = dispatch(product_cfg(40, n, DYN))
        assert d["code"] == 0 and not d["resto_in_launch"] and d["lds_first"] == d["lds"], (n, d)


def test_rule_by_plan():
    """Only a lean launch that the restoration pass follows directly restores in place."""
    c = product_cfg()
    assert dispatch(c)["resto_in_launch"]
    off = c.copy(); off.restoration = 0
    assert not dispatch(off)["resto_in_launch"] and dispatch(off)["passes"] == [0]
    for ss in range(4):
        for start in (False, True):
            c.second_start = ss
            d = dispatch(c, start_given=start)
            assert d["resto_in_launch"] == (len(d["passes"]) > 1 and d["passes"][1] == 2), (ss, start, d)
            assert d["resto_in_launch"], (ss, start, d)      # kin<1> fuses: every plan with restoration is FIRST, RESTO[, SECOND, RESTO]
    # planned as if the kernel did not fuse, kind 1 puts the second attempt between the first launch and the restoration pass
    c.second_start = 1
    d = dispatch(c, fused=False)
    assert d["passes"] == [0, 1, 2] and not d["resto_in_launch"] and d["lds_first"] == d["lds"]


def wgs_per_cu(lds):
    return min(4, CU_LDS // lds)


@pytest.mark.parametrize("N,want", [(30, True), (50, False), (1, None), (2, None), (63, None)])
def test_rule_by_lds(N, want):
    """The restoration layout must leave the lean launch its workgroups per CU, min(4, 160 KiB // LDS): N = 30 keeps 4, N = 50 would fall
    from 3 (52 504 B) to 2 (61 656 B).  N = 1, 2, 63: as computed from emu.lds_bytes."""
    c = product_cfg(N, 1)
    first, resto = emu.lds_bytes(c), emu.lds_bytes(c, True)
    rule = wgs_per_cu(resto) >= wgs_per_cu(first)
    if want is not None:
        assert rule == want
    if N == 50:
        assert (first, resto, wgs_per_cu(first), wgs_per_cu(resto)) == (52504, 61656, 3, 2)
    d = dispatch(c)
    print("N = %d: LDS %d / %d B, workgroups per CU %d / %d, rule %s" % (N, first, resto, wgs_per_cu(first), wgs_per_cu(resto), rule))
    assert d["resto_in_launch"] == rule and d["lds_first"] == (resto if rule else first) and d["passes"] == [0, 2]


# ----- 2. stepped on the CPU: forced on against forced off -----------------------------------------------------------------------------

def same_as_oracle(e, r, name):
    """The stepped source against the oracle as tests/test_emu_kernel.py compares batches: equal statuses, iteration counts equal but for
    at most one instance that takes one step more on one side, trajectories of the instances solved on both sides to 1e-9."""
    assert np.array_equal(e["status"], r["status"]), (name, e["status"], r["status"])
    d = np.abs(e["iters"] - r["iters"])
    assert d.max() <= 1 and (d != 0).sum() <= 1, (name, e["iters"], r["iters"])
    both = (e["status"] == 0) & (r["status"] == 0)
    if both.any():
        assert np.abs(e["z"][both] - r["z"][both]).max() <= 1e-9, name


def on_off(cfg, x0, xs, obs, name, **kw):
    on = emu_resto.solve(cfg, x0, xs, obs, resto_in_launch=True, **kw)
    off = emu_resto.solve(cfg, x0, xs, obs, resto_in_launch=False, **kw)
    print("%s: status %s iters %s" % (name, on["status"].tolist(), on["iters"].tolist()))
    assert pc.bit_equal(on, off, keys=OUT) == [], name
    if len(on["status"]) <= 4:                               # the small batches: forced off is what tests/emu itself steps
        assert pc.bit_equal(off, emu.solve(cfg, x0, xs, obs, **kw), keys=OUT) == [], name
    assert not (on["status"] == 7).any(), name               # MPCB_ST_NEEDS_RESTO never leaves a solve
    return on


SEED3 = scenes.sample_c2(256, seed=3)
_USES = {}


def uses_restoration(second_start):
    """The instances of sample_c2(256, seed=3) whose oracle result differs between restoration = 1 and 0 under the straight start, and the
    oracle's result with restoration (computed once per second_start)."""
    if second_start not in _USES:
        x0, xs, obs = SEED3
        c = straight_cfg(second_start); off = c.copy(); off.restoration = 0
        a = oracle.solve(c, x0, xs, obs); b = oracle.solve(off, x0, xs, obs)
        differs = (a["status"] != b["status"]) | (a["iters"] != b["iters"]) | (a["z"] != b["z"]).any(axis=1)
        _USES[second_start] = (np.nonzero(differs)[0], a)
    return _USES[second_start]


@pytest.mark.parametrize("second_start", [0, 1, 2, 3])
def test_forced_on_equals_forced_off_where_restoration_is_used(second_start):
    idx, ref = uses_restoration(second_start)
    print("second_start %d: %d of 256 instances use the restoration phase" % (second_start, len(idx)))
    assert len(idx) >= 32                                    # admission
    sel = idx[:8]
    x0, xs, obs = (a[sel] for a in SEED3)
    cfg = straight_cfg(second_start)
    assert dispatch(cfg)["resto_in_launch"]
    on = on_off(cfg, x0, xs, obs, "second_start %d" % second_start)
    same_as_oracle(on, {k: ref[k][sel] for k in ("status", "iters", "z")}, "second_start %d" % second_start)


def shift_plan(z, N, nx=4):
    B = len(z)
    U = z[:, :2 * N].reshape(B, N, 2); X = z[:, 2 * N:].reshape(B, N + 1, nx)
    return np.concatenate([np.concatenate([U[:, 1:], U[:, -1:]], axis=1).reshape(B, -1),
                           np.concatenate([X[:, 1:], X[:, -1:]], axis=1).reshape(B, -1)], axis=1)


def test_start_vector():
    """A shifted solution as the start (a warm start: second_start = 3 acts as 2, so both lean launches of FIRST, RESTO, SECOND, RESTO
    restore in place), from the states the shifted plans begin at."""
    idx, _ = uses_restoration(0)
    sel = idx[:4]
    x0, xs, obs = (a[sel] for a in SEED3)
    cfg = straight_cfg(3)
    z0 = shift_plan(oracle.solve(cfg, x0, xs, obs)["z"], 30)
    x1 = np.ascontiguousarray(z0[:, 60:64])
    assert dispatch(cfg, start_given=True)["passes"] == [0, 2, 1, 2]
    on = on_off(cfg, x1, xs, obs, "start vector", z0=z0)
    same_as_oracle(on, oracle.solve(cfg, x1, xs, obs, z0=z0), "start vector")


def test_no_obstacle():
    cfg = straight_cfg(3, n_obs=0)
    x0, xs, _ = scenes.sample_c2(4, seed=3)
    assert dispatch(cfg)["resto_in_launch"] and dispatch(cfg)["capacity"] == 0
    on = on_off(cfg, x0, xs, None, "n_obs = 0")
    same_as_oracle(on, oracle.solve(cfg, x0, xs, None), "n_obs = 0")


def test_tracking_rows_equal_to_xs():
    """The tracking kernels with rows equal to xs: the set-point solve of the same instances."""
    idx, ref = uses_restoration(0)
    sel = idx[:4]
    x0, xs, obs = (a[sel] for a in SEED3)
    cfg = straight_cfg(0)
    assert dispatch(cfg, track=True)["resto_in_launch"]
    on = on_off(cfg, x0, xs, obs, "tracking", x_ref=np.repeat(xs[:, None, :], 30, axis=1))
    same_as_oracle(on, {k: ref[k][sel] for k in ("status", "iters", "z")}, "tracking")


def test_uniform_parameter_rows():
    """The per-instance kernels with every row equal to the handle's config."""
    idx, ref = uses_restoration(1)
    sel = idx[:4]
    x0, xs, obs = (a[sel] for a in SEED3)
    cfg = straight_cfg(1)
    assert dispatch(cfg, params=True)["resto_in_launch"]
    on = on_off(cfg, x0, xs, obs, "uniform rows", cfgs=[cfg] * 4)
    same_as_oracle(on, {k: ref[k][sel] for k in ("status", "iters", "z")}, "uniform rows")


@pytest.mark.parametrize("N", [2, 63])
def test_shortest_and_longest_horizon(N):
    cfg = straight_cfg(0, N=N)
    x0, xs, obs = scenes.sample_c2(4, seed=3)
    on = on_off(cfg, x0, xs, obs, "N = %d" % N)
    same_as_oracle(on, oracle.solve(cfg, x0, xs, obs), "N = %d" % N)
