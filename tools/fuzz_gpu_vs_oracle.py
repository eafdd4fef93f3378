"""Differential fuzz: random NLP structures (model, horizon, obstacle count / kind / row form, tolerance, start) solved by the
HIP library and by the CPU oracle; reports every disagreement.  Run on a GPU box:
    python tools/fuzz_gpu_vs_oracle.py [cases] [seed] [data]
With `data` (perturb_data=True) the problem data is random as well: weights, boxes, rate bounds, geometry and vehicle / tyre
parameters within about +-40 % of the defaults, u_last and du0_cost; drawn from a second generator, so the structures of a seed
are the same with and without it.
Exit code 1 if any case disagrees beyond the test-suite tolerances (tests/test_gpu_parity.py, which also runs a short
fixed-seed pass of `run`)."""
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mpc_motion_planning_amd import scenes, _abi                                  # noqa: E402
from mpc_motion_planning_amd.solver import BatchSolver, default_config            # noqa: E402
from oracle import oracle                                                         # noqa: E402


def perturb(cfg, rng2):
    """Problem data within about +-40 % of the defaults (the ellipse at most 15 % larger: the samplers keep x0 out of the default one)."""
    def u(lo=0.6, hi=1.4):
        return float(rng2.uniform(lo, hi))
    nx = cfg.nx()
    for i in range(nx):
        cfg.Q[i] *= u()
    for i in range(2):
        cfg.R[i] *= u(); cfg.DR[i] *= u(); cfg.u_lo[i] *= u(); cfg.u_hi[i] *= u()
        if np.isfinite(cfg.du_lo[i]):
            cfg.du_lo[i] *= u()
        if np.isfinite(cfg.du_hi[i]):
            cfg.du_hi[i] *= u()
    cfg.u_last[0] = float(rng2.uniform(-0.05, 0.05)); cfg.u_last[1] = float(rng2.uniform(-1.0, 1.0))
    if rng2.random() < 0.3:
        cfg.du0_cost = 1 - cfg.du0_cost
    cfg.x_lo[1] *= u(); cfg.x_hi[1] *= u(0.92, 1.4)               # the scenes start at y in [-0.5, 4.5]
    cfg.x_hi[3] *= u(0.7, 1.4)
    if nx == 6:
        cfg.x_lo[4] *= u(); cfg.x_hi[4] *= u()
        for k in ("veh_m", "veh_lf", "veh_lr", "veh_Iz", "aopt_f", "aopt_r", "Fymax_f", "Fymax_r"):
            setattr(cfg, k, getattr(cfg, k) * u())
    cfg.veh_l *= u()
    for k in ("ego_hl", "ego_hw", "safe_disl", "safe_disw", "obs_sx_fixed", "obs_sy_fixed"):
        setattr(cfg, k, getattr(cfg, k) * u(0.6, 1.15))


def one_case(rng, c, rng2=None):
    dyn = rng.random() < 0.35
    N = int(rng.choice([1, 2, 3, 5, 8, 13, 20, 30, 31, 32, 33, 40, 50, 62, 63]))
    n_obs = int(rng.choice([0, 1, 1, 2, 3, 3, 4, 5, 8]))
    B = int(rng.choice([1, 3, 17, 64]))
    seed = int(rng.integers(1 << 30))
    kind = "static"
    if dyn:
        cfg = default_config(model=_abi.MODEL_DYN, N=N, n_obs=n_obs); tol = 1e-4
        x0, xs, obs = scenes.sample_c4(B, seed=seed, n_obs=max(n_obs, 1)); obs = obs[:, :n_obs]
    else:
        cfg = default_config(N=N, n_obs=n_obs); tol = 1e-5
        if n_obs == 0:
            x0, xs, obs = scenes.sample_c2(B, seed=seed); obs = obs[:, :0]
        else:
            if rng.random() < 0.5:
                kind = "predicted"
            x0, xs, ob0, traj = scenes.sample_c3(B, N=N, dt=0.1, seed=seed, n_obs=n_obs)
            obs = traj if kind == "predicted" else ob0
        if n_obs and rng.random() < 0.3:
            cfg.obs_mode = _abi.OBS_DCBF
            if rng.random() < 0.5:
                cfg.gamma = float(rng.uniform(0.1, 0.95))      # general-gamma rows (GEN kernels)
        if rng.random() < 0.2 and not (cfg.obs_mode == _abi.OBS_DCBF and cfg.gamma < 1.0):
            cfg.obs_terminal = 1
    if rng.random() < 0.2:
        cfg.tol = 1e-6
    if rng.random() < 0.2 and not dyn:          # dyn from z0 = 0 without the roll-out starts at vx = bound_push (1/vx in the tyre
        cfg.init_rollout = 0                     # model): both solvers fail there, in different ways
    desc = "case %d: %s N=%d n_obs=%d(%s) B=%d mode=%d gamma=%.2f term=%d tol=%g rollout=%d" % (
        c, "dyn" if dyn else "kin", N, n_obs, kind, B, cfg.obs_mode, cfg.gamma, cfg.obs_terminal, cfg.tol, cfg.init_rollout)
    if rng2 is not None:
        perturb(cfg, rng2)
        desc += " data: veh_l=%.2f Q1=%.3g R0=%.3g u_hi=(%.3f,%.2f) y=[%.2f,%.2f] du0_cost=%d" % (
            cfg.veh_l, cfg.Q[1], cfg.R[0], cfg.u_hi[0], cfg.u_hi[1], cfg.x_lo[1], cfg.x_hi[1], cfg.du0_cost)
    import os
    if os.environ.get("MPCB_FUZZ_VERBOSE"):
        print("  starting " + desc, flush=True)
    try:
        bs = BatchSolver(cfg)
    except Exception as e:                       # configurations the library refuses are refused by design; show them
        return True, desc + " -> refused: " + str(e)[:80]
    ob = obs if n_obs else None
    g = bs.solve_batch(x0, xs, ob, multipliers=True)
    r = oracle.solve(cfg, x0, xs, ob)
    bs.close()
    same = (g["status"] == r["status"]).mean()
    both = (g["status"] == 0) & (r["status"] == 0)
    errs = np.abs(g["z"][both] - r["z"][both]).max(axis=1) if both.any() else np.zeros(0)
    lim = tol * (10 if cfg.tol > 1e-8 else 1)
    far = int((errs > lim).sum())                # solved on both sides at different trajectories: another basin of the non-convex NLP
    err = float(errs[errs <= lim].max()) if (errs <= lim).any() else 0.0
    # what must agree: WHICH instances are solved (the way a failing instance fails — iteration cap, line search, numerics —
    # may differ between two roundings of the same algorithm), allowing one borderline instance per batch
    flips = int(((g["status"] == 0) != (r["status"] == 0)).sum())
    ok = flips <= max(1, B // 16) and far <= max(1, B // 32) and bool(np.all(np.isfinite(g["z"])))     # (round 2: B // 10 and B // 20; measured over 3 x 100 cases since: at most 3 of 64 flips, 1 other basin)
    return ok, desc + " -> status agreement %.2f, solved %d/%d, solved on one side only %d, L-inf(z) %.2e, other basin %d%s" % (same, int(both.sum()), B, flips, err, far, "" if ok else "  <-- MISMATCH")


def run(cases=60, seed=0, verbose=True, perturb_data=False):
    rng = np.random.default_rng(seed)
    rng2 = np.random.default_rng([seed, 1]) if perturb_data else None       # a generator of its own: rng's sequence does not depend on it
    bad = 0
    for c in range(cases):
        ok, line = one_case(rng, c, rng2)
        if verbose or not ok:
            print(line)
        bad += 0 if ok else 1
    if verbose:
        print("mismatching cases:", bad)
    return bad


if __name__ == "__main__":
    sys.exit(1 if run(int(sys.argv[1]) if len(sys.argv) > 1 else 60, int(sys.argv[2]) if len(sys.argv) > 2 else 0,
                      perturb_data=len(sys.argv) > 3 and sys.argv[3] == "data") else 0)
