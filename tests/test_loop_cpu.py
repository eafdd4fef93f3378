"""The stepwise loop (mpcb_loop_*) without a GPU: the C ABI of the new entry points, the resource rows of its glue kernels, and the
admission conditions of the scenarios tests/test_loop_gpu.py drives (tests/loop_cases.py): the oracle alone, run through the external
plant with its own outputs, solves enough of every scenario for a comparison against it to mean something."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mpc_motion_planning_amd import _abi, _lib
from tests import config_cases as cc, loop_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the eight entries the stepwise loop consists of, and the read-out of its counters
LOOP_ENTRIES = ["mpcb_loop_create", "mpcb_loop_destroy", "mpcb_loop_reset", "mpcb_loop_get_start", "mpcb_loop_set_start", "mpcb_loop_step",
                "mpcb_loop_step_device", "mpcb_loop_advance_device"]
COUNTERS_ENTRY = "mpcb_loop_counters"


def test_library_exports_the_loop_entries_and_signatures_cover_them():
    L = _lib.lib()
    for name in LOOP_ENTRIES + [COUNTERS_ENTRY]:
        assert hasattr(L, name), "libmpcbatch.so lacks %s" % name
        assert name in _lib.SIGNATURES, "_lib.SIGNATURES lacks %s" % name
    text = open(os.path.join(ROOT, "include", "mpcbatch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mpcb_loop_[a-z_]+)\s*\(", text))
    assert declared == set(LOOP_ENTRIES + [COUNTERS_ENTRY])
    assert "#define MPCB_LOOP_PREDICT 4" in text and _abi.LOOP_PREDICT == 4
    assert "#define MPCB_ABI_VERSION 3" in text and _abi.ABI_VERSION == 3            # additive: the version stays


def test_null_handle_and_null_loop_are_error_codes():
    L = _lib.lib()
    out = C.c_void_p()
    assert L.mpcb_loop_create(None, 4, 0, None, C.byref(out)) == _abi.E_INVALID and not out.value
    assert b"handle" in L.mpcb_last_error(None)
    assert L.mpcb_loop_destroy(None, None) == _abi.E_INVALID
    assert L.mpcb_loop_reset(None, None, None) == _abi.E_INVALID
    assert L.mpcb_loop_get_start(None, None, None) == _abi.E_INVALID
    assert L.mpcb_loop_set_start(None, None, None) == _abi.E_INVALID
    assert L.mpcb_loop_counters(None, None, None, None) == _abi.E_INVALID
    assert L.mpcb_loop_step(None, None, None, None, None, None, 0, None, None, None, None, None) == _abi.E_INVALID
    assert L.mpcb_loop_step_device(None, None, None, None, None, None, 0, None, None, None, None, None, 0) == _abi.E_INVALID
    assert L.mpcb_loop_advance_device(None, None, None, None, None, 0, 0) == _abi.E_INVALID


def test_shipped_resource_table_lists_the_glue_kernels_without_scratch():
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "r03_kernel_resources.txt")):
        m = re.match(r"^(mpcb_loop_\w+(?:<\d>)?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
        if m:
            rows[m.group(1)] = [int(v) for v in m.groups()[1:]]
    for name in ("mpcb_loop_commit<4>", "mpcb_loop_commit<6>", "mpcb_loop_plant<4>", "mpcb_loop_plant<6>"):
        assert name in rows, "profiles/r03_kernel_resources.txt has no row %s" % name
        vgpr, agpr, scratch_bytes, n_instr, ds, scratch_instr, flat, glob = rows[name]
        assert scratch_instr == 0, "%s: %d scratch instructions" % (name, scratch_instr)
        assert glob > 0 and n_instr > 0
    assert not any(n.startswith("mpcb_kernel_") for n in rows)                          # tests/test_kernel_isa.py counts that prefix


def test_python_surface_without_a_device():
    from mpc_motion_planning_amd import solver
    assert callable(solver.BatchSolver.loop)
    for name in ("step", "step_device", "advance_device", "reset", "close", "__enter__", "__exit__"):
        assert callable(getattr(solver.ControlLoop, name)), name
    for name in ("start", "steps", "failures"):
        assert isinstance(getattr(solver.ControlLoop, name), property), name
    assert solver.ControlLoop.start.fset is not None


def test_numpy_bookkeeping_of_the_reference_loop():
    """shift_plan and executed_plan on a plan whose entries name their place: u_i -> u_{i+1} (last repeated), x_k -> x_{k+1}."""
    n, nx = lc.N, 4
    z = np.arange(2 * n + nx * (n + 1), dtype=float)[None].repeat(3, axis=0)
    z[1] += 1000.0; z[2] += 2000.0
    s = lc.shift_plan(z)
    assert np.array_equal(s[0, :2 * (n - 1)], z[0, 2:2 * n]) and np.array_equal(s[0, 2 * (n - 1):2 * n], z[0, 2 * n - 2:2 * n])
    assert np.array_equal(s[0, 2 * n:2 * n + nx * n], z[0, 2 * n + nx:]) and np.array_equal(s[0, -nx:], z[0, -nx:])
    w = -np.ones_like(z)
    st = np.array([_abi.ST_SOLVED, _abi.ST_MAXITER, _abi.ST_ACCEPTABLE], np.int32)
    held = lc.executed_plan(w, z, st, True)
    assert np.array_equal(held[0], z[0]) and np.array_equal(held[1], w[1]) and np.array_equal(held[2], z[2])
    assert np.array_equal(lc.executed_plan(w, z, st, False), z)


@pytest.mark.parametrize("scn", lc.SCENARIOS, ids=lc.ids(lc.SCENARIOS))
def test_oracle_alone_solves_enough_of_every_scenario(oracle_mod, scn):
    """Admission condition: >= 0.95 of the (instance, step) solves end SOLVED or ACCEPTABLE when the oracle itself is the controller
    (shares when the scenarios were admitted: c3_predicted_hold 0.988, c2_static 1.000 with the draws the issue used; this file's draws are
    printed)."""
    cfg = lc.config(scn, lambda **kw: cc.product(oracle_mod.default_config(**kw)))
    log = lc.drive(scn, cfg, lc.OracleController(scn, cfg, oracle_mod))
    status = np.stack([e["status"] for e in log], axis=1)
    share = lc.solved(status).mean()
    print("scenario %s: solved share %.4f over %d x %d solves, statuses %s" % (scn.name, share, scn.B, scn.steps, np.bincount(status.ravel())))
    assert status.shape == (scn.B, scn.steps) and scn.B <= 64 and scn.steps <= 8
    assert share >= lc.MIN_SOLVED_SHARE


@pytest.mark.parametrize("name", sorted(lc.PER_STEP))
def test_oracle_alone_solves_enough_of_the_per_step_input_runs(oracle_mod, name):
    """The same admission condition on the runs whose set-points switch mid-run / that pass stage references every step."""
    scn, kw = lc.PER_STEP[name]
    cfg = lc.config(scn, lambda **k: cc.product(oracle_mod.default_config(**k)))
    log = lc.drive(scn, cfg, lc.OracleController(scn, cfg, oracle_mod), **kw)
    status = np.stack([e["status"] for e in log], axis=1)
    share = lc.solved(status).mean()
    print("run %s: solved share %.4f over %d x %d solves, statuses %s" % (name, share, scn.B, scn.steps, np.bincount(status.ravel())))
    assert share >= lc.MIN_SOLVED_SHARE
    if name == "xs_switches_lane":
        assert not np.array_equal(log[lc.SWITCH_STEP]["xs"], log[lc.SWITCH_STEP - 1]["xs"])
