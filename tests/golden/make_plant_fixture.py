"""Records tests/golden/plant_step.npz on an MI355X: inputs and outputs of ControlLoop.advance_device (the library's plant step and
obstacle move, no solve in it) for the cases of tests/loop_cases.py (PLANT_CASES), 64 instances each, two steps in a row.

The committed file was recorded from the build BEFORE the plant step, the shift and the hold rule moved into csrc/mpcb_plant.h; it anchors
the kernels built from that header to the bits of the kernels it replaced.  Recording it again from a later build only restates that
build, so do that only for a change that is meant to move the plant's bits.

    python tests/golden/make_plant_fixture.py [output.npz]

Inputs are stored once per (model, n_obs) under <key>_x0 / _u0 / _obs; per case <name>_x<k> and <name>_obsxy<k> after step k = 1, 2
(of the obstacle rows only x, y can change).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mpc_motion_planning_amd.solver import BatchSolver, default_config      # noqa: E402
from tests import loop_cases as lc                                          # noqa: E402

out = {}
for case in lc.PLANT_CASES:
    cfg, rows = lc.plant_configs(case, default_config)
    x0, u0, obs = lc.plant_inputs(case, cfg)
    key = lc.plant_inputs_key(case)
    for name, a in (("x0", x0), ("u0", u0), ("obs", obs)):
        assert np.array_equal(out.setdefault("%s_%s" % (key, name), a), a)
    for k, (x, ob) in enumerate(lc.plant_on_device(BatchSolver, case, cfg, rows, x0, u0, obs), start=1):
        assert np.array_equal(ob[..., 2:], obs[..., 2:]) and np.isfinite(x).all()
        out["%s_x%d" % (case.name, k)] = x
        out["%s_obsxy%d" % (case.name, k)] = ob[..., :2].copy()
    print("%-10s |x2 - x0| max %.3e, obstacles moved: %s" % (case.name, np.abs(x - x0).max(), (ob[..., :2] != obs[..., :2]).any(axis=(0, 2))))

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "plant_step.npz")
np.savez_compressed(path, **out)
print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
