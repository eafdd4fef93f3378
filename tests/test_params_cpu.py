"""Per-instance problem data without a GPU: the PARAMS instantiations of the kernel source stepped on the CPU (tests/emu) over
the mixed batches of tests/params_cases.py against the oracle and against tests/emu run under each instance's own config, the
host-side validation of a parameter set, solver.vary, and the machine code of the ten mpcb_param_* kernels.  The device tier is
tests/test_params_gpu.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from oracle import oracle
from tests import config_cases as cc, params_cases as pc
from tests.emu import emu
from mpc_motion_planning_amd import scenes, _abi, _lib
from mpc_motion_planning_amd.solver import BatchSolver, default_config, vary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")

NEW_ENTRIES = ["mpcb_params_check", "mpcb_params_create", "mpcb_params_destroy", "mpcb_solve_params", "mpcb_solve_device_params",
               "mpcb_closed_loop_params"]


def _ocfg(case):
    return cc.oracle_cfg(case, oracle)


# ----- 1. admission -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [pc.KIN_MIX, pc.DYN_MIX], ids=["kin", "dyn"])
def test_oracle_solves_enough_of_every_mixed_batch(names):
    """The admission rule of tests/config_cases.py for the mixed batches of the device tier: the oracle alone, called once per distinct
    config, solves >= 0.95 of the 256 instances."""
    cases, cfgs, which, x0, xs, obs = pc.mix(names, cc.GPU_BATCH, _ocfg)
    r = pc.per_config(lambda c, a, b, o: oracle.solve(c, a, b, o, want_multipliers=False), cfgs, which, x0, xs, obs, keys=("status",))
    frac = (r["status"] == 0).mean()
    print("mixed batch %s: oracle alone solves %d of %d" % (names[0], (r["status"] == 0).sum(), len(x0)))
    assert len(x0) == 256 and frac >= 0.95, frac


# ----- 2. the stepped PARAMS source against the oracle and against tests/emu under each instance's own config -----------------------
@pytest.mark.parametrize("names", [pc.KIN_MIX, pc.DYN_MIX], ids=["kin", "dyn"])
def test_stepped_mixed_batch_against_oracle_and_per_instance_emu(names):
    """Instance b is scene b under case b (B = 8 kinematic, B = 4 dynamic), the handle's config is case 0's.  Statuses and iteration
    counts equal the oracle's and z lies within 1e-9 of it (the margin of tests/test_tracking_oracle.py for stepped source against
    oracle); against tests/emu run per instance under that instance's config every output is bit-equal: same source, same arithmetic."""
    K = len(names)
    cases, cfgs, which, x0, xs, obs = pc.mix(names, K, _ocfg)
    e = emu.solve(cfgs[0], x0, xs, obs, cfgs=pc.rows(cfgs, which))
    r = pc.per_config(lambda c, a, b, o: oracle.solve(c, a, b, o), cfgs, which, x0, xs, obs)
    one = pc.per_config(lambda c, a, b, o: emu.solve(c, a, b, o), cfgs, which, x0, xs, obs)
    dz = np.abs(e["z"] - r["z"]).max(axis=1)
    print("stepped mix %s: status %s iters %s oracle iters %s L-inf(z) per instance %s"
          % (names[0], e["status"].tolist(), e["iters"].tolist(), r["iters"].tolist(), ["%.1e" % v for v in dz]))
    assert pc.bit_equal(e, one) == []
    assert np.array_equal(e["status"], r["status"]) and (r["status"] == 0).all()
    assert np.array_equal(e["iters"], r["iters"])
    assert dz.max() <= 1e-9
    # the rows are read: under the handle's config alone instances 1 and 3 (other weights; another geometry or other bounds) end elsewhere
    base_only = emu.solve(cfgs[0], x0[[1, 3]], xs[[1, 3]], obs[[1, 3]])
    assert (np.abs(base_only["z"] - e["z"][[1, 3]]).max(axis=1) > 1e-4).all()


# ----- 3. uniform rows --------------------------------------------------------------------------------------------------------------
def _restoration_batch():
    """Scenes 1 and 2 of sample_c2(8, seed=3) under the geometry case: the first of them is the borderline instance the docstring of
    tests/config_cases.py names, its first attempt finds no acceptable step; the second one solves in its first attempt."""
    cfg = _ocfg(cc.BY_NAME["geometry"])
    x0, xs, obs = scenes.sample_c2(8, seed=3)
    return cfg, x0[1:3], xs[1:3], obs[1:3]


@pytest.mark.parametrize("second_start", [0, 1])
def test_uniform_rows_equal_the_plain_stepped_source(second_start):
    """A set whose rows all equal the handle's config returns bitwise what tests/emu returns; with second_start = 0 the batch holds an
    instance that runs the restoration pass (it ends MPCB_ST_LINESEARCH when restoration is switched off), with second_start = 1 one
    that runs the second attempt."""
    cfg, x0, xs, obs = _restoration_batch()
    cfg.second_start = second_start
    plain = emu.solve(cfg, x0, xs, obs)
    e = emu.solve(cfg, x0, xs, obs, cfgs=[cfg] * len(x0))
    print("uniform rows, second_start %d: status %s iters %s" % (second_start, e["status"].tolist(), e["iters"].tolist()))
    assert pc.bit_equal(e, plain) == []
    off = cfg.copy(); off.restoration = 0; off.second_start = 0
    first = emu.solve(off, x0, xs, obs)
    assert first["status"].tolist() == [_abi.ST_LINESEARCH, _abi.ST_SOLVED]        # the later passes had work to do on instance 0 ...
    assert plain["status"][0] not in (_abi.ST_LINESEARCH, _abi.ST_MAXITER)         # ... and did it: the restoration pass sets another status
    if second_start == 1:
        assert plain["iters"][0] > first["iters"][0]                               # the second attempt's iterations are counted on top


# ----- 4. validation on the host ----------------------------------------------------------------------------------------------------
def _check(base, cfgs):
    bad = C.c_int32(-7)
    rc = _lib.lib().mpcb_params_check(C.byref(base), cfgs, len(cfgs), C.byref(bad))
    msg = _lib.lib().mpcb_last_error(None).decode()
    return rc, bad.value, msg


def test_validation_accepts_data_and_rejects_structure_with_the_first_bad_row():
    cfg = default_config(N=30, n_obs=1)
    B = 12
    rng = np.random.default_rng(0)
    ok = vary(cfg, B, Q=rng.uniform(1, 1e4, (B, 4)), veh_l=rng.uniform(2, 3, B), tol=np.full(B, 1e-7), start_steer=np.full(B, 0.02),
              x_lo=np.column_stack([np.full(B, -INF), rng.uniform(-2, -1, B)]), u_last=rng.uniform(-0.1, 0.1, (B, 2)))
    assert _check(cfg, ok)[:2] == (_abi.OK, -1)
    for field, row, edit in (("N", 5, lambda c: setattr(c, "N", 29)),
                             ("du0_cost", 0, lambda c: setattr(c, "du0_cost", 0)),
                             ("T", 11, lambda c: setattr(c, "T", 0.15)),
                             ("x_lo", 7, lambda c: c.x_lo.__setitem__(1, -INF)),
                             ("veh_l", 3, lambda c: setattr(c, "veh_l", 0.0)),
                             ("second_start", 4, lambda c: setattr(c, "second_start", 1)),
                             ("gamma", 2, lambda c: setattr(c, "gamma", 0.5)),
                             ("struct_size", 9, lambda c: setattr(c, "struct_size", 8))):
        rows = vary(cfg, B)
        edit(rows[row]); edit(rows[B - 1])                         # two bad rows: the FIRST is reported
        rc, bad, msg = _check(cfg, rows)
        assert rc == _abi.E_INVALID and bad == row and field in msg and ("row %d" % row) in msg, (field, rc, bad, msg)
    # what the per-instance kernels are not built for is refused as such, whatever the rows say
    for edit in (lambda c: (setattr(c, "obs_mode", _abi.OBS_DCBF), setattr(c, "gamma", 0.5)), lambda c: setattr(c, "integrator", _abi.INT_RK4),
                 lambda c: setattr(c, "n_obs", 5)):
        base = cfg.copy(); edit(base)
        rc, bad, msg = _check(base, vary(base, 4))
        assert rc == _abi.E_UNSUPPORTED and bad == -1 and "parameter sets" in msg, (rc, bad, msg)
    # "is there a bound" as the kernels decide it (L > -1e300, U < 1e300): +inf as a lower bound IS one, a finite value beyond 1e300 is
    # none: such rows have another pattern than the handle's and are refused
    for field, edit in (("x_lo", lambda c: c.x_lo.__setitem__(0, INF)), ("x_hi", lambda c: c.x_hi.__setitem__(3, 2e300)),
                        ("du_lo", lambda c: c.du_lo.__setitem__(0, -1.5e300)), ("u_hi", lambda c: c.u_hi.__setitem__(1, INF))):
        rows = vary(cfg, B); edit(rows[6])
        rc, bad, msg = _check(cfg, rows)
        assert rc == _abi.E_INVALID and bad == 6 and field in msg, (field, rc, bad, msg)
    rows = vary(cfg, B); rows[6].x_hi[4] = 1.5e300; rows[6].x_lo[5] = -2e300      # no bound either way, as the handle's +-inf
    assert _check(cfg, rows)[:2] == (_abi.OK, -1)
    dyn = default_config(model=_abi.MODEL_DYN, N=20, n_obs=3)
    assert _check(dyn, vary(dyn, 4, veh_m=np.array([1300.0, 1500, 1700, 1900])))[0] == _abi.OK
    assert _check(dyn, vary(dyn, 4, veh_m=np.array([1300.0, 1500, -1, 1900])))[:2] == (_abi.E_INVALID, 2)


def test_new_entry_points_in_header_bindings_and_library():
    text = open(os.path.join(ROOT, "include", "mpcbatch.h")).read()
    names = set(re.findall(r"\b(mpcb_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    L = _lib.lib()
    for n in NEW_ENTRIES:
        assert n in names and n in _lib.SIGNATURES and hasattr(L, n), n
    assert re.search(r"#define MPCB_ABI_VERSION 3\b", text) and _abi.ABI_VERSION == 3
    assert L.mpcb_version().decode().startswith("mpcbatch 0.4 ")
    # a NULL handle is refused by every new entry, before anything else is looked at
    cfg = default_config(N=30, n_obs=1); rows = vary(cfg, 2); p = C.c_void_p(); bad = C.c_int32()
    assert L.mpcb_params_create(None, rows, 2, C.byref(p), C.byref(bad)) == _abi.E_INVALID and not p.value
    assert L.mpcb_params_destroy(None, None) == _abi.E_INVALID
    assert L.mpcb_solve_params(None, 1, None, None, None, None, 0, None, None, None, None, None, None, None, None) == _abi.E_INVALID
    assert L.mpcb_solve_device_params(None, 1, None, None, None, None, 0, None, None, None, None, None, None, None, None, 0) == _abi.E_INVALID
    assert L.mpcb_closed_loop_params(None, 1, 1, None, None, None, None, 0, 0, None, None, None, None) == _abi.E_INVALID
    assert L.mpcb_params_check(None, rows, 2, C.byref(bad)) == _abi.E_INVALID
    assert L.mpcb_params_check(C.byref(cfg), None, 2, C.byref(bad)) == _abi.E_INVALID
    assert L.mpcb_params_check(C.byref(cfg), rows, 0, C.byref(bad)) == _abi.E_INVALID


# ----- 5. vary() --------------------------------------------------------------------------------------------------------------------
def test_vary_fills_fields_and_refuses_what_it_does_not_know():
    cfg = default_config(N=30, n_obs=1)
    B = 5
    q = np.arange(B * 4, dtype=float).reshape(B, 4) + 1; l = np.linspace(2.0, 3.0, B)
    rows = vary(cfg, B, Q=q, veh_l=l, max_iter=np.arange(B) + 50)
    assert len(rows) == B and isinstance(rows, C.Array)
    for b in range(B):
        assert list(rows[b].Q[:4]) == list(q[b]) and list(rows[b].Q[4:]) == list(cfg.Q[4:])
        assert rows[b].veh_l == l[b] and rows[b].max_iter == 50 + b
        ref = cfg.copy(); ref.veh_l = l[b]; ref.max_iter = 50 + b
        for i in range(4):
            ref.Q[i] = q[b, i]
        assert bytes(rows[b]) == bytes(ref)                                   # nothing else moved
    assert cfg.veh_l == 2.6                                                   # the template is copied, not edited
    for kw in (dict(wheelbase=l), dict(Q=q[:, :0]), dict(Q=np.ones((B, 7))), dict(Q=np.ones(B)), dict(Q=np.ones((B + 1, 4))), dict(veh_l=q),
               dict(veh_l=l[:-1]), dict(veh_l=2.6), dict(max_iter=np.arange(B) + 50.5)):
        with pytest.raises(ValueError):
            vary(cfg, B, **kw)
    with pytest.raises(ValueError):
        vary(cfg, 0)


def test_params_with_a_reference_is_refused_before_any_library_call():
    bs = BatchSolver.__new__(BatchSolver)                        # no handle: the error must come before the library is called
    bs.nx, bs.N, bs.nz = 4, 30, 2 * 30 + 4 * 31
    bs._h = None
    with pytest.raises(ValueError, match="params"):
        bs.solve_batch(np.zeros((2, 4)), np.zeros((2, 4)), x_ref=np.zeros((2, 30, 4)), params=object())
    with pytest.raises(ValueError, match="params"):
        bs.solve_device(2, 0, 0, 0, 0, None, 0, d_x_ref=1, params=object())
    with pytest.raises(ValueError, match="params"):
        bs.closed_loop(np.zeros((2, 4)), np.zeros((2, 4)), aa=0.5, params=object())


# ----- 6. machine code of the ten kernels: the rules of tests/test_kernel_isa.py -----------------------------------------------------
sys.path.insert(0, ROOT)
from tools import kernel_resources as kr   # noqa: E402

needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(kr.LLVM, "llvm-objdump")), reason="ROCm LLVM tools not installed")

TWINS = {"mpcb_param_kin<%d>" % n: "mpcb_kernel_kin<%d, false, false>" % n for n in (0, 1, 3)}
TWINS.update({"mpcb_param_kin_resto<%d>" % n: "mpcb_kernel_kin_resto<%d, false, false>" % n for n in (0, 1, 3)})
TWINS.update({"mpcb_param_dyn<%d>" % n: "mpcb_kernel_dyn<%d>" % n for n in (1, 3)})
TWINS.update({"mpcb_param_dyn_resto<%d>" % n: "mpcb_kernel_dyn_resto<%d>" % n for n in (1, 3)})
NO_SCRATCH = ["mpcb_param_kin<0>", "mpcb_param_kin<1>", "mpcb_param_kin<3>", "mpcb_param_kin_resto<0>", "mpcb_param_kin_resto<1>",
              "mpcb_param_dyn<1>", "mpcb_param_dyn<3>"]


@pytest.fixture(scope="module")
def shipped():
    return kr.kernels()


@needs_llvm
def test_the_ten_param_kernels_exist_and_the_others_are_all_there(shipped):
    ks, non_kernels = shipped
    assert non_kernels == []
    assert sorted(k for k in ks if k.startswith("mpcb_param_")) == sorted(TWINS) and len(TWINS) == 10
    assert not [k for k in ks if k.startswith("mpcb_advance_params")]             # mpcb_advance<NX> reads the rows itself
    assert "mpcb_advance<4>" in ks and "mpcb_advance<6>" in ks
    assert len([k for k in ks if k.startswith("mpcb_kernel_")]) == 30
    assert len([k for k in ks if k.startswith("mpcb_track_kin")]) == 22


@needs_llvm
@pytest.mark.parametrize("name", sorted(TWINS))
def test_param_kernel_meets_the_resource_conditions(shipped, name):
    ks = shipped[0]
    k, twin = ks[name], ks[TWINS[name]]
    assert k["instr"].get("flat_", 0) == 0, (name, k["instr"])
    assert k["instr"].get("s_barrier", 0) == 0, name
    assert k["wg_max"] == 64 and k["lds_static"] == 0, name
    assert k["scratch"] <= twin["scratch"], "%s: %d B scratch, its twin %d B" % (name, k["scratch"], twin["scratch"])
    if name in NO_SCRATCH:
        assert k["scratch"] == 0 and k["instr"].get("scratch_", 0) == 0, (name, k["scratch"])


@needs_llvm
def test_existing_rows_of_the_committed_resource_table_are_unchanged():
    """No existing behaviour changes, stated for the compiled code: every row profiles/r03_kernel_resources.txt held before the
    parameter sets is still the shipped library's row, byte for byte; the table only gained rows."""
    now = kr.table().splitlines()
    kept = open(os.path.join(ROOT, "profiles", "r03_kernel_resources.txt")).read().splitlines()
    assert now == kept
    new = [l for l in now if l.startswith("mpcb_param_")]
    assert len(new) == 10
