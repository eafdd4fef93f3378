"""Evaluate and certify any point on the MI355X (mpcb_evaluate / mpcb_evaluate_device, the mpcb_eval kernels): the table of
tests/eval_cases.py against oracle/kkt_check.py, the refusals, NULL outputs, the launch lanes, and the audit of a whole launch.  The CPU
tier (the same device source stepped by tests/emu_eval) is tests/test_evaluate_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from mpc_motion_planning_amd import scenes, _abi
from mpc_motion_planning_amd._abi import dptr
from mpc_motion_planning_amd._lib import MpcbError, lib
from mpc_motion_planning_amd.solver import default_config, vary
from tests import eval_cases as ec
from tests import params_cases as pc

pytestmark = pytest.mark.gpu

OUT_KEYS = ("obj", "g", "grad_lag") + _abi.EVAL_NAMES


def _same(a, b, keys=OUT_KEYS):
    return pc.bit_equal(a, b, keys=keys)


@pytest.mark.parametrize("case", ec.CASES, ids=ec.ids(ec.CASES))
def test_evaluation_against_kkt_check(gpu_solver_factory, case):
    """The table, 32 instances per case, at the device's own solution with its multipliers and at a random point with random
    multipliers: obj, every entry of g and grad_lag and every residual of every instance (tolerances: tests/eval_cases.py)."""
    prob = ec.problem(case, default_config, ec.GPU_BATCH)
    if not case.create:                                  # the kinematic solve kernels have no interleaved order: there is no handle
        with pytest.raises(MpcbError) as e:
            gpu_solver_factory(prob["cfg"])
        assert e.value.code == _abi.E_UNSUPPORTED
        return
    bs = gpu_solver_factory(prob["cfg"])
    ps = bs.params(prob["rows"]) if prob["params"] else None
    sol = bs.solve_batch(prob["x0"], prob["xs"], prob["obs"], multipliers=True, x_ref=prob["x_ref"], params=ps)
    point = (sol["z"], sol["lam_g"], sol["lam_x"])
    for label, (z, lg, lx) in (("solution", point), ("random", ec.random_point(case, sol["z"], bs.ng))):
        out = bs.evaluate(prob["x0"], prob["xs"], prob["obs"], z, lg, lx, x_ref=prob["x_ref"], params=ps, want_grad=True)
        ec.check(case, prob, z, lg, lx, out, label)
        if label == "solution":                          # the objective a solved instance reports is the objective of its point
            ok = sol["status"] == _abi.ST_SOLVED
            assert np.allclose(out["obj"][ok], sol["obj"][ok], rtol=1e-12, atol=0.0)
    bs.close()


def test_a_gamma_half_handle_is_evaluated_and_still_has_no_parameter_set(gpu_solver_factory):
    """mpcb_params_create refuses a general-gamma handle, so there is no set to evaluate under; without a set the handle is evaluated
    (the table's kin_dcbf_gamma_0.5), and the solve entries refuse what they refused."""
    prob = ec.problem(ec.BY_NAME["kin_dcbf_gamma_0.5"], default_config, 4)
    bs = gpu_solver_factory(prob["cfg"])
    with pytest.raises(MpcbError) as e:
        bs.params(vary(prob["cfg"], 4))
    assert e.value.code == _abi.E_UNSUPPORTED
    z = np.zeros((4, bs.nz))
    assert np.isfinite(bs.evaluate(prob["x0"], prob["xs"], prob["obs"], z)["obj"]).all()
    bs.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.25


class _Raw:
    """The C entries called with explicit pointers, outputs pre-filled with a sentinel."""

    def __init__(self, bs, prob, z, lg, lx):
        self.bs, self.B = bs, len(z)
        c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)      # noqa: E731
        self.inp = dict(x0=c(prob["x0"]), xs=c(prob["xs"]), x_ref=c(prob["x_ref"]), obs=c(prob["obs"]), z=c(z), lam_g=c(lg), lam_x=c(lx))
        self.kind = _abi.OBSIN_PREDICTED if prob["obs"] is not None and prob["obs"].ndim == 4 else _abi.OBSIN_STATIC
        self.dev = {k: (None if v is None else bs.device_array(v.shape).upload(v)) for k, v in self.inp.items()}
        self.shapes = dict(obj=(self.B,), g=(self.B, bs.ng), grad_lag=(self.B, bs.nz), res=(self.B, _abi.EVAL_COLS))

    def host(self, params=None, drop=(), **over):
        a = dict(self.inp); a.update(over)
        out = {k: (None if k in drop else np.full(s, SENTINEL)) for k, s in self.shapes.items()}
        rc = lib().mpcb_evaluate(self.bs._h, self.B, params, dptr(a["x0"]), dptr(a["xs"]), dptr(a["x_ref"]), dptr(a["obs"]), self.kind, dptr(a["z"]),
                                 dptr(a["lam_g"]), dptr(a["lam_x"]), dptr(out["obj"]), dptr(out["g"]), dptr(out["grad_lag"]), dptr(out["res"]))
        return rc, out

    def device(self, params=None, drop=(), **over):
        a = dict(self.dev); a.update(over)
        d = {k: (None if k in drop else self.bs.device_array(s).upload(np.full(s, SENTINEL))) for k, s in self.shapes.items()}
        p = lambda v: None if v is None else v.ptr                                          # noqa: E731
        rc = lib().mpcb_evaluate_device(self.bs._h, self.B, params, p(a["x0"]), p(a["xs"]), p(a["x_ref"]), p(a["obs"]), self.kind, p(a["z"]),
                                        p(a["lam_g"]), p(a["lam_x"]), p(d["obj"]), p(d["g"]), p(d["grad_lag"]), p(d["res"]), 1)
        out = {k: (None if v is None else v.download()) for k, v in d.items()}
        for v in d.values():
            if v is not None:
                v.free()
        return rc, out


def _untouched(out):
    return all(v is None or (v == SENTINEL).all() for v in out.values())


def _as_dict(out):
    d = dict(obj=out["obj"], g=out["g"], grad_lag=out["grad_lag"])
    if out["res"] is not None:
        d.update({n: out["res"][:, i].copy() for i, n in enumerate(_abi.EVAL_NAMES)})
    return d


def test_refusals_come_before_the_first_launch(gpu_solver_factory):
    """Every refusal of both entries: its code, the outputs untouched, and the evaluation that follows is the one before."""
    case = ec.BY_NAME["kin_C2"]
    prob = ec.problem(case, default_config, 8)
    bs = gpu_solver_factory(prob["cfg"])
    other = gpu_solver_factory(prob["cfg"])
    sol = bs.solve_batch(prob["x0"], prob["xs"], prob["obs"], multipliers=True)
    raw = _Raw(bs, prob, sol["z"], sol["lam_g"], sol["lam_x"])
    xr = np.repeat(prob["xs"][:, None, :], 30, axis=1)
    d_xr = bs.device_array(xr.shape).upload(xr)
    ps, ps_other, ps4 = bs.params(vary(prob["cfg"], 8)), other.params(vary(prob["cfg"], 8)), bs.params(vary(prob["cfg"], 4))
    for call, xref in ((raw.host, xr), (raw.device, d_xr)):
        rc, good = call()
        assert rc == 0 and not _untouched(good)
        refused = [
            (_abi.E_INVALID, dict(z=None)),
            (_abi.E_INVALID, dict(lam_x=None)),                                  # one multiplier array without the other
            (_abi.E_INVALID, dict(lam_g=None)),
            (_abi.E_INVALID, dict(lam_g=None, lam_x=None)),                      # grad_lag without multipliers
            (_abi.E_INVALID, dict(x0=None)),
            (_abi.E_INVALID, dict(obs=None)),
            (_abi.E_UNSUPPORTED, dict(x_ref=xref, params=ps.ptr)),               # x_ref together with a set
            (_abi.E_INVALID, dict(params=ps_other.ptr)),                         # a set of another handle
            (_abi.E_INVALID, dict(params=ps4.ptr)),                              # a set of another B
        ]
        for code, kw in refused:
            rc, out = call(**kw)
            assert rc == code and _untouched(out), (kw.keys(), rc)
            assert lib().mpcb_last_error(bs._h)
        bs.set_time_grid(np.full(30, 0.1))                                       # kkt_check has no time-grid NLP to test one against
        rc, out = call()
        assert rc == _abi.E_UNSUPPORTED and _untouched(out)
        bs.set_time_grid(None)
        rc, again = call()
        assert rc == 0 and _same(_as_dict(again), _as_dict(good)) == []
        rc, with_set = call(params=ps.ptr)                                       # rows equal to the handle's config: the same numbers
        assert rc == 0 and _same(_as_dict(with_set), _as_dict(good)) == []
    ec.check(case, prob, sol["z"], sol["lam_g"], sol["lam_x"], _as_dict(good), "after refusals")
    # a set whose structure is no longer the handle's: mpcb_set_bounds after mpcb_params_create takes the y box away (the re-check of
    # mpcb_solve_params); without the set the handle is evaluated, and with the bounds back the set is the handle's again
    from oracle import kkt_check
    nlp = kkt_check.KinNlp.from_config(prob["cfg"], prob["x0"][0], prob["xs"][0], prob["obs"][0])
    lbx, ubx = nlp.lbx.copy(), nlp.ubx.copy()
    lbx[2 * 30 + 1::4] = -np.inf; ubx[2 * 30 + 1::4] = np.inf
    bs.set_bounds(lbx, ubx, nlp.lbg, nlp.ubg)
    for call in (raw.host, raw.device):
        rc, out = call(params=ps.ptr)
        assert rc == _abi.E_INVALID and _untouched(out) and b"changed since" in lib().mpcb_last_error(bs._h)
        rc, out = call()
        assert rc == 0 and not _untouched(out)
    bs.set_bounds(nlp.lbx, nlp.ubx, nlp.lbg, nlp.ubg)
    for call in (raw.host, raw.device):
        rc, back = call(params=ps.ptr)
        assert rc == 0 and _same(_as_dict(back), _as_dict(good)) == []
    stale = _Closed(ps)
    with pytest.raises(MpcbError) as e:                                          # a destroyed set: looked up among the live ones, never read
        bs.evaluate(prob["x0"], prob["xs"], prob["obs"], sol["z"], params=stale)
    assert e.value.code == _abi.E_INVALID
    # x_ref on the dynamic model, both entries
    dcase = ec.BY_NAME["dyn_vehicle"]
    dprob = ec.problem(dcase, default_config, 4)
    dyn = gpu_solver_factory(dprob["cfg"])
    zd = np.zeros((4, dyn.nz)); zd[:, 2 * 20 + 3::6] = 10.0
    with pytest.raises(MpcbError) as e:
        dyn.evaluate(dprob["x0"], dprob["xs"], dprob["obs"], zd, x_ref=np.zeros((4, 20, 6)))
    assert e.value.code == _abi.E_UNSUPPORTED
    draw = _Raw(dyn, dprob, zd, None, None)
    xr6 = np.zeros((4, 20, 6))
    for call, xref in ((draw.host, xr6), (draw.device, dyn.device_array(xr6.shape).upload(xr6))):
        rc, out = call(drop=("grad_lag",), x_ref=xref)
        assert rc == _abi.E_UNSUPPORTED and _untouched(out)
        rc, out = call(drop=("grad_lag",))
        assert rc == 0 and np.isfinite(out["obj"]).all()
    dyn.close()
    other.close(); bs.close()


def test_a_device_group_is_refused(gpu_solver_factory):
    prob = ec.problem(ec.BY_NAME["kin_C2"], default_config, 8)
    bs = gpu_solver_factory(prob["cfg"])
    raw = _Raw(bs, prob, np.zeros((8, bs.nz)), None, None)
    rc, good = raw.host(drop=("grad_lag",))
    assert rc == 0 and not _untouched(good)
    bs.set_devices([0])
    for call in (raw.host, raw.device):
        rc, out = call(drop=("grad_lag",))
        assert rc == _abi.E_UNSUPPORTED and _untouched(out)
    bs.close()


class _Closed:
    """A parameter set closed behind the wrapper's back: its pointer is stale."""

    def __init__(self, ps):
        self.ptr = C.c_void_p(ps.ptr.value)
        ps.close()


def test_null_outputs_in_every_combination_of_one(gpu_solver_factory):
    prob = ec.problem(ec.BY_NAME["kin_C3_predicted"], default_config, 8)
    bs = gpu_solver_factory(prob["cfg"])
    sol = bs.solve_batch(prob["x0"], prob["xs"], prob["obs"], multipliers=True)
    raw = _Raw(bs, prob, sol["z"], sol["lam_g"], sol["lam_x"])
    for call in (raw.host, raw.device):
        rc, full = call()
        assert rc == 0
        for name in ("obj", "g", "grad_lag", "res"):
            rc, out = call(drop=(name,))
            assert rc == 0 and out[name] is None
            for k in out:
                if k != name:
                    assert out[k].tobytes() == full[k].tobytes(), (name, k)
        rc, out = call(drop=("obj", "g", "grad_lag", "res"))                     # nothing asked for is not an error
        assert rc == 0
        rc, bare = call(drop=("grad_lag",), lam_g=None, lam_x=None)              # without multipliers
        assert rc == 0 and np.isnan(bare["res"][:, 3:]).all() and bare["res"][:, :3].tobytes() == full["res"][:, :3].tobytes()
        assert bare["g"].tobytes() == full["g"].tobytes() and bare["obj"].tobytes() == full["obj"].tobytes()
    bs.close()


def test_host_pointer_evaluate_is_bit_equal_to_evaluate_device(gpu_solver_factory):
    for name in ("kin_C2", "dyn_C4"):
        prob = ec.problem(ec.BY_NAME[name], default_config, ec.GPU_BATCH)
        bs = gpu_solver_factory(prob["cfg"])
        sol = bs.solve_batch(prob["x0"], prob["xs"], prob["obs"], multipliers=True)
        raw = _Raw(bs, prob, sol["z"], sol["lam_g"], sol["lam_x"])
        (rh, host), (rd, dev) = raw.host(), raw.device()
        assert rh == 0 and rd == 0 and _same(_as_dict(host), _as_dict(dev)) == []
        via_wrapper = bs.evaluate(prob["x0"], prob["xs"], prob["obs"], sol["z"], sol["lam_g"], sol["lam_x"], want_grad=True)
        assert _same(via_wrapper, _as_dict(host)) == []
        bs.close()


def test_a_point_that_holds_a_nan_passes_no_gate(gpu_solver_factory):
    """The compiled kernels (v_max_f64 / v_min_f64 drop a NaN): one NaN in z or in a multiplier of a certified instance, and it passes no
    gate; either model."""
    for name in ("kin_C2", "dyn_vehicle"):
        prob = ec.problem(ec.BY_NAME[name], default_config, 8)
        bs = gpu_solver_factory(prob["cfg"])
        sol = bs.solve_batch(prob["x0"], prob["xs"], prob["obs"], multipliers=True)
        b = int(np.nonzero(sol["status"] == _abi.ST_SOLVED)[0][0])
        ec.check_nan_is_never_certified(lambda z, lg, lx: bs.evaluate(prob["x0"], prob["xs"], prob["obs"], z, lg, lx, want_g=False),
                                        bs.N, bs.nx, bs.nz, bs.ng, sol["z"], sol["lam_g"], sol["lam_x"], b)
        bs.close()


# ---- lanes -------------------------------------------------------------------------------------------------------------------------
def _pairs(bs, B, n_pairs):
    """n_pairs (solve_device, evaluate_device) pairs on rotated buffers, one buffer set per pair, then one more solve; everything downloaded."""
    sets = []
    for j in range(n_pairs + 1):
        x0, xs, obs = scenes.sample_c2(B, seed=40 + j)
        d = dict(x0=bs.device_array(x0.shape).upload(x0), xs=bs.device_array(xs.shape).upload(xs), obs=bs.device_array(obs.shape).upload(obs),
                 z=bs.device_array((B, bs.nz)), lam_g=bs.device_array((B, bs.ng)), lam_x=bs.device_array((B, bs.nz)),
                 sobj=bs.device_array((B,)), status=bs.device_array((B,), np.int32), iters=bs.device_array((B,), np.int32),
                 obj=bs.device_array((B,)), g=bs.device_array((B, bs.ng)), grad_lag=bs.device_array((B, bs.nz)), res=bs.device_array((B, _abi.EVAL_COLS)))
        sets.append(d)
    bs.sync()
    for j in range(n_pairs):
        d = sets[j]
        bs.solve_device(B, d["x0"], d["xs"], d["obs"], _abi.OBSIN_STATIC, None, d["z"], d_obj=d["sobj"], d_status=d["status"], d_iters=d["iters"],
                        d_lam_g=d["lam_g"], d_lam_x=d["lam_x"])
        bs.evaluate_device(B, d["x0"], d["xs"], d["obs"], _abi.OBSIN_STATIC, d["z"], d["lam_g"], d["lam_x"], d_obj=d["obj"], d_g=d["g"],
                           d_grad_lag=d["grad_lag"], d_res=d["res"])
    d = sets[n_pairs]
    bs.solve_device(B, d["x0"], d["xs"], d["obs"], _abi.OBSIN_STATIC, None, d["z"], d_obj=d["sobj"], d_status=d["status"], d_iters=d["iters"],
                    d_lam_g=d["lam_g"], d_lam_x=d["lam_x"])
    bs.sync()
    out = [{k: v.download() for k, v in d.items() if k not in ("x0", "xs", "obs")} for d in sets]
    for d in sets:
        for v in d.values():
            v.free()
    return out


def test_pairs_on_four_lanes_equal_pairs_on_one_lane(gpu_solver_factory):
    """Eight (solve, evaluate_device) pairs with rotated buffers on a four-lane handle are bit-equal in every output to the same pairs on a
    one-lane handle (the evaluation runs behind its solve, on its lane, and does not advance the rotation), and a solve issued after
    them is bit-equal to one on a fresh handle."""
    cfg = default_config(N=30, n_obs=1)
    B, n = 64, 8
    res = {}
    for k in (4, 1):
        bs = gpu_solver_factory(cfg, inflight=k)
        res[k] = _pairs(bs, B, n)
        bs.close()
    solve_keys = ("z", "lam_g", "lam_x", "sobj", "status", "iters")
    for j in range(n + 1):                               # (the last buffer set took the closing solve alone: nothing wrote its evaluation outputs)
        assert pc.bit_equal(res[4][j], res[1][j], keys=tuple(res[1][0].keys()) if j < n else solve_keys) == [], "pair %d" % j
        if j < n:
            assert (res[4][j]["res"][:, 0] >= 0).all() and np.isfinite(res[4][j]["obj"]).all()      # the evaluation did run
            ok = res[4][j]["status"] == 0
            assert np.allclose(res[4][j]["obj"][ok], res[4][j]["sobj"][ok], rtol=1e-12, atol=0.0)    # ... on ITS solve's point
    fresh = gpu_solver_factory(cfg)
    x0, xs, obs = scenes.sample_c2(B, seed=40 + n)
    f = fresh.solve_batch(x0, xs, obs, multipliers=True)
    last = res[4][n]
    assert pc.bit_equal(dict(z=last["z"], obj=last["sobj"], status=last["status"], iters=last["iters"], lam_g=last["lam_g"], lam_x=last["lam_x"]), f) == []
    fresh.close()


# ---- the audit of a whole launch ---------------------------------------------------------------------------------------------------
def test_audit_of_a_launch(gpu_solver_factory):
    """256 C2 scenes, the device's solution evaluated on the device: every instance the solve calls SOLVED meets the bounds DESIGN.md §5.6
    records for the numpy certificate (feas_g <= 1.01e-8: the bound relaxation is 1e-8; sign = 0; stationarity / lam_scale <= 1e-8;
    compl <= 1e-4: the compl_inf_tol gate), and every unsolved instance fails at least one of them."""
    cfg = default_config(N=30, n_obs=1)
    x0, xs, obs = scenes.sample_c2(256, seed=11)
    bs = gpu_solver_factory(cfg)
    sol = bs.solve_batch(x0, xs, obs, multipliers=True)
    ev = bs.evaluate(x0, xs, obs, sol["z"], sol["lam_g"], sol["lam_x"], want_g=False)
    bs.close()
    passes = (ev["feas_g"] <= 1.01e-8) & (ev["sign"] == 0.0) & (ev["stationarity"] / ev["lam_scale"] <= 1e-8) & (ev["compl"] <= 1e-4)
    solved = sol["status"] == _abi.ST_SOLVED
    print("audit: %d of 256 SOLVED; worst of them: feas_g %.3e, sign %.3e, stationarity/lam_scale %.3e, compl %.3e; unsolved %d, of which pass %d" % (
        solved.sum(), ev["feas_g"][solved].max(), ev["sign"][solved].max(), (ev["stationarity"] / ev["lam_scale"])[solved].max(),
        ev["compl"][solved].max(), (~solved).sum(), (passes & ~solved).sum()))
    assert solved.sum() >= 1
    assert passes[solved].all(), np.nonzero(solved & ~passes)[0]
    assert not passes[~solved].any(), np.nonzero(~solved & passes)[0]
