"""The mixed batches of the per-instance-config tests, shared by tests/test_params_cpu.py (the PARAMS instantiations of the kernel
source stepped on the CPU) and tests/test_params_gpu.py (the compiled mpcb_param_* kernels).  A plain module: no fixtures.

Instance b of a mixed batch takes scene b of the population its cases share (tests/config_cases.py: sample_c2 seed 3 for the kinematic
cases, sample_c4 seed 9 for the dynamic ones) and the config of case b mod K.  The reference result is the oracle called once per
distinct config on that config's instances and scattered back: the oracle takes a config per call, so it needs no change."""
import numpy as np

from tests import config_cases as cc

KIN_MIX = ["default", "weights", "bounds", "geometry", "u_last", "u_last_sets_the_scaling", "scaling", "no_pull_along_the_road"]
DYN_MIX = ["dyn_default", "dyn_vehicle", "dyn_weights", "dyn_bounds"]


def mix(names, B, cfg_of):
    """(cases, cfgs, which, x0, xs, obs): cfgs[k] = cfg_of(cases[k]), instance b is solved under cfgs[which[b]], which[b] = b mod K."""
    cases = [cc.BY_NAME[n] for n in names]
    assert len({(c.model, c.N, c.n_obs, c.sampler, c.seed, c.T) for c in cases}) == 1, "one population and one structure per mix"
    assert B <= cc.GPU_BATCH
    x0, xs, obs, _ = cc.scenes(cases[0])            # the population of GPU_BATCH scenes, then its first B: a smaller draw is another population
    x0, xs, obs = x0[:B], xs[:B], obs[:B]
    return cases, [cfg_of(c) for c in cases], np.arange(B) % len(cases), x0, xs, obs


def rows(cfgs, which):
    """The per-instance config list of a mixed batch (what BatchSolver.params and emu.solve take)."""
    return [cfgs[k] for k in which]


def per_config(solve, cfgs, which, x0, xs, obs, keys=("z", "obj", "status", "iters", "lam_g", "lam_x")):
    """solve(cfg, x0, xs, obs) once per distinct config on that config's instances, scattered back into batch order."""
    out = {}
    for k, cfg in enumerate(cfgs):
        idx = np.nonzero(which == k)[0]
        if len(idx) == 0:
            continue
        r = solve(cfg, x0[idx], xs[idx], None if obs is None else obs[idx])
        for key in keys:
            if r.get(key) is None:
                continue
            if key not in out:
                out[key] = np.zeros((len(which),) + r[key].shape[1:], r[key].dtype)
            out[key][idx] = r[key]
    return out


def bit_equal(a, b, keys=("z", "obj", "status", "iters", "lam_g", "lam_x")):
    """Names of the outputs in which two result dicts differ in any bit (NaNs at the same places count as equal)."""
    bad = []
    for key in keys:
        if key in a and key in b and a[key] is not None and b[key] is not None:
            x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
            if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
                bad.append(key)
    return bad
