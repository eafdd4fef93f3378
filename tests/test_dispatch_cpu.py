"""The launch policy of mpc_motion_planning_amd/csrc/mpcb_dispatch.h (which kernel instantiation serves a config, its LDS, whether it fuses
its second attempt, the order of the passes), read through tests/emu and compared with tables written out here.  The tables are
transcribed from the if / else ladders mpcb_api.hip dispatched by before the policy had a header of its own.  No GPU, no solve."""
import itertools

from mpc_motion_planning_amd import _abi
from oracle import oracle
from tests.emu import emu

KIN, DYN = _abi.MODEL_KIN, _abi.MODEL_DYN
FIRST, SECOND, RESTO = 0, 1, 2            # MPCB_PASS_*

# obstacle-row capacity of the instantiation that serves n_obs = 0..8 (index = n_obs)
CAP_KIN = [0, 1, 3, 3, 5, 5, 8, 8, 8]
CAP_GEN = [None, 1, 3, 3, 8, 8, 8, 8, 8]  # general-gamma rows exist from one obstacle on; no <5>
CAP_RK4 = [0, 1, 3, 3]
CAP_DYN = [1, 1, 3, 3, 5, 5, 8, 8, 8]
CAP_PARAMS = {KIN: [0, 1, 3, 3], DYN: [1, 1, 3, 3]}

ROWS = ("keepout", "dcbf_gamma_1", "dcbf_gamma_half")
NOT_SHIPPED = {
    "track_dyn": "per-stage reference tracking is built for the kinematic model only",
    "params_gen": "parameter sets: general-gamma discrete-CBF rows have no per-instance kernel (keep-out or gamma = 1 rows only)",
    "params_rk4": "parameter sets: MPCB_INT_RK4 has no per-instance kernel (MPCB_INT_EULER only)",
    "params_nobs": "parameter sets: n_obs = %d, the per-instance kernels are built for up to 3 obstacles",
}


def config(model, n_obs, rows, rk4, N=30):
    c = oracle.default_config(model=model, N=N, n_obs=n_obs)
    if rows != "keepout":
        c.obs_mode = _abi.OBS_DCBF; c.obs_terminal = 0
        c.gamma = 1.0 if rows == "dcbf_gamma_1" else 0.5
    c.integrator = _abi.INT_RK4 if rk4 else _abi.INT_EULER
    return c


def accepted(model, n_obs, rows, rk4):
    """What check_cfg lets through on these axes: general gamma and RK4 on the kinematic model only, RK4 up to 3 obstacles and never with
    general gamma."""
    if model == DYN:
        return rows != "dcbf_gamma_half" and not rk4
    return not (rk4 and (n_obs > 3 or rows == "dcbf_gamma_half"))


def test_variant_capacity_fusing_and_the_combinations_that_are_not_shipped():
    seen = set()
    for model, n, rows, rk4, use in itertools.product((KIN, DYN), range(9), ROWS, (False, True), ("plain", "track", "params")):
        if not accepted(model, n, rows, rk4):
            continue
        d = emu.dispatch(config(model, n, rows, rk4), track=use == "track", params=use == "params")
        gen = model == KIN and rows == "dcbf_gamma_half" and n > 0
        why = None
        if use == "track" and model == DYN:
            why = NOT_SHIPPED["track_dyn"]
        elif use == "params" and gen:
            why = NOT_SHIPPED["params_gen"]
        elif use == "params" and rk4:
            why = NOT_SHIPPED["params_rk4"]
        elif use == "params" and n > 3:
            why = NOT_SHIPPED["params_nobs"] % n
        if why is not None:
            assert d == dict(code=_abi.E_UNSUPPORTED, why=why), (model, n, rows, rk4, use, d)
            continue
        if use == "params":
            cap = CAP_PARAMS[model][n]
        elif model == DYN:
            cap = CAP_DYN[n]
        else:
            cap = CAP_GEN[n] if gen else CAP_RK4[n] if rk4 else CAP_KIN[n]
        got = (d["code"], d["model"], d["capacity"], d["gen"], d["rk4"], d["track"], d["params"])
        assert got == (0, model, cap, gen, rk4 and model == KIN, use == "track", use == "params"), (model, n, rows, rk4, use, d)
        # the second attempt runs inside the first launch on kin<0|1|3> without GEN / RK4 (plain, tracking, per-instance) and on dyn<1|3>
        assert d["fuses"] == (cap <= 3 and not gen and not rk4), (model, n, rows, rk4, use, d)
        seen.add(got[1:])
    assert len(seen) == 31       # every shipped instantiation is reached: 11 kin, 11 tracking, 4 dyn, 3 + 2 per-instance (x 2 passes = 62 kernels)
    both = emu.dispatch(config(KIN, 1, "keepout", False), track=True, params=True)
    assert both == dict(code=_abi.E_UNSUPPORTED, why="a parameter set together with a per-stage reference")


# the launches of one solve.  Kind of the second start: None = there is none, 1 = instead of the first attempt's restoration pass (fused
# into the first launch where the instantiation fuses), 2 = after it
PLAN = {
    (None, 0): [FIRST],
    (None, 1): [FIRST, RESTO],
    (1, 0, False): [FIRST, SECOND],
    (1, 0, True): [FIRST],
    (1, 1, False): [FIRST, SECOND, RESTO],
    (1, 1, True): [FIRST, RESTO],
    (2, 0): [FIRST, SECOND],
    (2, 1): [FIRST, RESTO, SECOND, RESTO],
}
# second_start -> kind, without and with a start vector; a second start exists only after a roll-out start
KIND = {0: (None, None), 1: (1, 1), 2: (2, 2), 3: (1, 2)}


def test_pass_plan():
    for resto, ss, rollout, start, fused in itertools.product((0, 1), range(4), (0, 1), (False, True), (False, True)):
        c = config(KIN, 1, "keepout", False)
        c.restoration = resto; c.second_start = ss; c.init_rollout = rollout
        kind = KIND[ss][start] if rollout else None
        want = PLAN[(kind, resto, fused)] if kind == 1 else PLAN[(kind, resto)]
        assert emu.dispatch(c, start_given=start, fused=fused)["passes"] == want, (resto, ss, rollout, start, fused)
    # asked without an override, the plan follows the instantiation: kin<1> fuses, kin<5> does not
    c = config(KIN, 1, "keepout", False); c.second_start = 1; c.init_rollout = 1; c.restoration = 1
    assert emu.dispatch(c)["passes"] == [FIRST, RESTO]
    c.n_obs = 4
    assert emu.dispatch(c)["passes"] == [FIRST, SECOND, RESTO]


LDS_KIN30_1 = LDS_KIN30_3 = (32824, 38456)      # C2, C3 / C5
LDS_KIN50_1 = (52504, 61656)
LDS_DYN40_3 = (52872, 62280)                    # C4
LDS_KIN63_8 = (82120, 93560)
LDS_DYN63_8 = (98296, 112856)


def test_lds_bytes():
    """The six instances of test_emu_kernel.py's budget test: the bytes the harness reported for them when it carried a formula of its own
    (first pass, restoration pass).  And one RK4 config: the RK4 kernels' entry table has the four rows more of the general-gamma kernels
    (27 instead of 23 rows of ld = 31 doubles), which that formula left out."""
    want = {
        (KIN, 30, 1): LDS_KIN30_1, (KIN, 30, 3): LDS_KIN30_3, (KIN, 50, 1): LDS_KIN50_1,
        (DYN, 40, 3): LDS_DYN40_3, (KIN, 63, 8): LDS_KIN63_8, (DYN, 63, 8): LDS_DYN63_8,
    }
    for (model, N, n), (first, resto) in want.items():
        c = oracle.default_config(model=model, N=N, n_obs=n)
        d = emu.dispatch(c)
        assert (d["lds"], d["lds_resto"]) == (first, resto), (model, N, n, d)
        assert (emu.lds_bytes(c), emu.lds_bytes(c, True)) == (first, resto)
    rk4 = emu.dispatch(config(KIN, 1, "keepout", True))
    assert rk4["lds"] == LDS_KIN30_1[0] + 4 * 31 * 8 == 33816
    assert rk4["lds_resto"] == LDS_KIN30_1[1] + 4 * 31 * 8
