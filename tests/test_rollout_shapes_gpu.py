"""The first-pass Euler kernels kin<0>, kin<1>, kin<3> at the horizons where the forward roll-out's two-stage trip and its lane layout
can go wrong (tests/rollout_cases.py), from a cold and from a warm start, 16 instances each: against the oracle with the helper and the
tolerances test_gpu_parity.py uses for horizons (agree(): trajectories 1e-5, statuses 98 %, which at 16 instances means all of them),
and once per shape the plain kernel against the per-instance kernel (mpcb_param_*) with uniform rows, bit for bit."""
import numpy as np
import pytest

from mpc_motion_planning_amd.solver import vary
from tests import params_cases as pc, rollout_cases as rc
from tests.test_gpu_parity import agree

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_obs", rc.N_OBS)
@pytest.mark.parametrize("N", rc.HORIZONS)
def test_rollout_shape_against_oracle_and_param_kernel(gpu_solver_factory, oracle_mod, N, n_obs):
    cfg, x0, xs, obs = rc.scene(N, n_obs)
    cold_ref, (x1, z0), warm_ref = rc.reference(N, n_obs)
    bs = gpu_solver_factory(cfg)
    try:
        cold = bs.solve_batch(x0, xs, obs, multipliers=True)
        warm = bs.solve_batch(x1, xs, obs, z0=z0)
        with bs.params(vary(cfg, rc.B)) as ps:
            par = bs.solve_batch(x0, xs, obs, multipliers=True, params=ps)
    finally:
        bs.close()
    print("N %d, %d obstacles: cold statuses %s iters %s, warm statuses %s iters %s" % (
        N, n_obs, cold["status"].tolist(), cold["iters"].tolist(), warm["status"].tolist(), warm["iters"].tolist()))
    assert pc.bit_equal(cold, par, keys=("z", "obj", "status", "iters", "kkt", "lam_g", "lam_x")) == []
    agree(cold, cold_ref, min_same_status=0.98)
    agree(warm, warm_ref, min_same_status=0.98)
    assert np.all(np.isfinite(cold["z"])) and np.all(np.isfinite(warm["z"]))
