"""CPU twin of test_rollout_shapes_gpu.py: the kernel source stepped on the CPU (tests/emu, one host thread per lane, the wv:: primitives'
emulation halves) against the oracle at the same horizons, obstacle capacities and starts.  The stepped source runs the same
instantiations the library ships, so a wrong lane mapping of the roll-out (a component picked up from the wrong lane of its row, a trip
that reads a stage too far) shows here before any GPU time is spent.  Bounds as in test_emu_kernel.py: the same status and the
trajectory within 1e-8 wherever both solve.  EMU_B instances per shape instead of the GPU twin's 16: a stepped solve costs 64 threads
meeting at a barrier at every cross-lane operation."""
import numpy as np
import pytest

from tests import rollout_cases as rc
from tests.emu import emu

EMU_B = 2


@pytest.mark.parametrize("n_obs", rc.N_OBS)
@pytest.mark.parametrize("N", rc.HORIZONS)
def test_stepped_rollout_shape_against_oracle(N, n_obs):
    cfg, x0, xs, obs = rc.scene(N, n_obs, EMU_B)
    cold_ref, (x1, z0), warm_ref = rc.reference(N, n_obs, EMU_B)
    cold = emu.solve(cfg, x0, xs, obs)
    warm = emu.solve(cfg, x1, xs, obs, z0=z0)
    for e, r, what in ((cold, cold_ref, "cold"), (warm, warm_ref, "warm")):
        print("N %d, %d obstacles, %s: statuses %s / %s, iters %s / %s" % (N, n_obs, what, e["status"].tolist(), r["status"].tolist(),
                                                                            e["iters"].tolist(), r["iters"].tolist()))
        assert np.array_equal(e["status"], r["status"]), what
        both = (e["status"] == 0) & (r["status"] == 0)
        if both.any():
            assert np.abs(e["z"][both] - r["z"][both]).max() <= 1e-8, what
        assert np.all(np.isfinite(e["z"])), what
