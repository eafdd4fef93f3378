"""The multi-start solve on the MI355X (mpcb_solve_multi / mpcb_solve_multi_device, the kernels mpcb_multi_expand and mpcb_multi_select): the
table of tests/multi_cases.py against a plain solve of the expanded batch, against the selection rule stated in Python, and against the
oracle; K = 1 against mpcb_solve_device; the refusals; the launch lanes; host against device pointers.  The CPU tier (the same device
source stepped by tests/emu_multi) is tests/test_multi_cpu.py."""

import numpy as np
import pytest

from mpc_motion_planning_amd import _abi
from mpc_motion_planning_amd._abi import dptr, iptr
from mpc_motion_planning_amd._lib import lib
from mpc_motion_planning_amd.solver import default_config
from tests import multi_cases as mc

pytestmark = pytest.mark.gpu

TOL_Z, TOL_Z_DYN = 1e-5, 1e-4          # the trajectory margins of tests/test_gpu_parity.py
MIN_SAME_STATUS = 0.98                 # its status margin for batches of this size
SOLVE_KEYS = ("z", "obj", "status", "iters", "kkt", "lam_g", "lam_x")
_RUNS = {}


def _bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _obs_kind(p):
    return _abi.OBSIN_PREDICTED if p["obs"] is not None and np.asarray(p["obs"]).ndim == 4 else _abi.OBSIN_STATIC


def _plain_solve_device(bs, x0, xs, obs, kind, z0):
    """One mpcb_solve_device call over a batch with start vectors, every output downloaded."""
    B = len(x0)
    up = lambda a: None if a is None else bs.device_array(np.asarray(a).shape).upload(a)      # noqa: E731
    d_in = [up(x0), up(xs), up(obs), up(z0)]
    d = dict(z=bs.device_array((B, bs.nz)), obj=bs.device_array((B,)), status=bs.device_array((B,), np.int32), iters=bs.device_array((B,), np.int32),
             kkt=bs.device_array((B, 4)), lam_g=bs.device_array((B, bs.ng)), lam_x=bs.device_array((B, bs.nz)))
    bs.solve_device(B, d_in[0], d_in[1], d_in[2], kind, d_in[3], d["z"], d["obj"], d["status"], d["iters"], d["kkt"], d["lam_g"], d["lam_x"], sync=True)
    out = {k: v.download() for k, v in d.items()}
    for v in list(d.values()) + [v for v in d_in if v is not None]:
        v.free()
    return out


def _run(case, gpu_solver_factory):
    """The case solved once by solve_multi (host pointers, everything asked for) and once as a plain solve of the numpy-expanded batch."""
    if case.name not in _RUNS:
        p = mc.problem(case, default_config)
        cfg, B, K = p["cfg"], p["B"], p["K"]
        bs = gpu_solver_factory(cfg)
        multi = bs.solve_multi(p["x0"], p["xs"], p["obs"], z0=p["z0"], controls=p["controls"], multipliers=True, want_all=True)
        x0_e, xs_e, obs_e, z0_e = mc.expand_rule(cfg.N, p["x0"], p["xs"], p["obs"], p["controls"], p["z0"])
        plain = _plain_solve_device(bs, x0_e, xs_e, obs_e, _obs_kind(p), z0_e)
        bs.close()
        _RUNS[case.name] = (p, multi, plain)
    return _RUNS[case.name]


# ---- K = 1 is the plain solve ---------------------------------------------------------------------------------------------------------
def test_k1_with_a_caller_start_is_solve_device_bit_for_bit(gpu_solver_factory):
    p = mc.problem(mc.BY_NAME["kin_caller_z0_k3"], default_config)
    bs = gpu_solver_factory(p["cfg"])
    plain = _plain_solve_device(bs, p["x0"], p["xs"], p["obs"], _abi.OBSIN_STATIC, p["z0"])
    for controls in ([[0.3, -2.0]], None):                       # with a start, controls[0] is ignored; the C entry also takes NULL
        if controls is None:
            B = p["B"]
            out = dict(z=np.empty((B, bs.nz)), obj=np.empty(B), status=np.empty(B, np.int32), iters=np.empty(B, np.int32), kkt=np.empty((B, 4)),
                       lam_g=np.empty((B, bs.ng)), lam_x=np.empty((B, bs.nz)), which=np.empty(B, np.int32), n_ok=np.empty(B, np.int32),
                       n_basins=np.empty(B, np.int32))
            x0 = np.ascontiguousarray(p["x0"]); xs = np.ascontiguousarray(p["xs"]); obs = np.ascontiguousarray(p["obs"]); z0 = np.ascontiguousarray(p["z0"])
            rc = lib().mpcb_solve_multi(bs._h, B, 1, dptr(x0), dptr(xs), dptr(obs), _abi.OBSIN_STATIC, dptr(z0), None, 1e-9, 1e-4, dptr(out["z"]),
                                        dptr(out["obj"]), iptr(out["status"]), iptr(out["iters"]), dptr(out["kkt"]), dptr(out["lam_g"]),
                                        dptr(out["lam_x"]), iptr(out["which"]), iptr(out["n_ok"]), iptr(out["n_basins"]), None, None, None, None)
            assert rc == 0
        else:
            out = bs.solve_multi(p["x0"], p["xs"], p["obs"], z0=p["z0"], controls=controls, multipliers=True)
        for k in SOLVE_KEYS:
            assert _bits(out[k], plain[k]), k
        ok = np.array([mc.eligible(s, f) for s, f in zip(plain["status"], plain["obj"])], dtype=np.int32)
        assert ok.sum() >= 1 and not out["which"].any() and np.array_equal(out["n_ok"], ok) and np.array_equal(out["n_basins"], ok)
    bs.close()


# ---- the table -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.CASES, ids=mc.ids(mc.CASES))
def test_all_candidates_equal_one_plain_solve_of_the_expanded_batch(gpu_solver_factory, case):
    p, multi, plain = _run(case, gpu_solver_factory)
    B, K = p["B"], p["K"]
    for k in ("z", "obj", "status", "iters"):
        assert _bits(multi[k + "_all"].reshape((B * K,) + multi[k + "_all"].shape[2:]), plain[k]), k


@pytest.mark.parametrize("case", mc.CASES, ids=mc.ids(mc.CASES))
def test_winner_and_counts_equal_the_python_rule_on_the_devices_own_candidates(gpu_solver_factory, case):
    p, multi, plain = _run(case, gpu_solver_factory)
    B, K = p["B"], p["K"]
    which, n_ok, n_basins = mc.select_rule(multi["z_all"], multi["obj_all"], multi["status_all"])
    assert np.array_equal(multi["which"], which) and np.array_equal(multi["n_ok"], n_ok) and np.array_equal(multi["n_basins"], n_basins), (
        multi["which"], which, multi["n_ok"], n_ok, multi["n_basins"], n_basins)
    for k in ("z", "obj", "status", "iters"):
        assert _bits(multi[k], mc.gather(multi[k + "_all"], which)), k
    for k in ("kkt", "lam_g", "lam_x"):                          # no *_all of these leaves the call: the plain solve's rows are the candidates'
        assert _bits(multi[k], mc.gather(plain[k].reshape((B, K) + plain[k].shape[1:]), which)), k


@pytest.mark.parametrize("case", mc.CASES, ids=mc.ids(mc.CASES))
def test_candidates_and_choice_against_the_oracle(gpu_solver_factory, oracle_mod, case):
    """Every candidate against the oracle's with the margins of tests/test_gpu_parity.py (status agreement, trajectories within TOL_Z where
    both solve, up to the other-basin allowance); then the choice: `which` is the oracle's wherever its decisive gap exceeds 1e-6 and the
    candidates themselves agree, and the winner's objective is within 1e-8 relative where `which` agrees."""
    p, multi, plain = _run(case, gpu_solver_factory)
    ref = mc.oracle_pipeline(case.name)
    tol = TOL_Z_DYN if case.model == _abi.MODEL_DYN else TOL_Z
    same = multi["status_all"] == ref["status_all"]
    both = (multi["status_all"] == 0) & (ref["status_all"] == 0)
    err = np.where(both, np.abs(multi["z_all"] - ref["z_all"]).max(axis=2), 0.0)
    far = err > tol
    print("%s: status agreement %.4f over %d candidates, %d solved on both sides, %d of them in another basin, worst L-inf within the basin %.2e"
          % (case.name, same.mean(), same.size, both.sum(), far.sum(), err[~far].max()))
    assert same.sum() >= same.size - max(1, int((1 - MIN_SAME_STATUS) * same.size)), "status agreement %.4f" % same.mean()
    assert far.sum() <= max(1, int(0.02 * both.sum())), "%d of %d candidates beyond %.0e" % (far.sum(), both.sum(), tol)
    gap = mc.decisive_gap(ref["obj_all"], ref["status_all"])
    elig = lambda r: np.array([[mc.eligible(s, f) for s, f in zip(ss, ff)] for ss, ff in zip(r["status_all"], r["obj_all"])])      # noqa: E731
    comparable = (gap > 1e-6) & (elig(multi) == elig(ref)).all(axis=1) & ~far.any(axis=1)
    # (each of the two allowances above excuses at least one candidate, hence up to two instances; beyond that a tenth of the batch)
    assert comparable.sum() >= len(gap) - max(2, int(0.1 * len(gap))), "only %d of %d instances can be compared" % (comparable.sum(), len(gap))
    assert np.array_equal(multi["which"][comparable], ref["which"][comparable]), (multi["which"], ref["which"], comparable)
    assert np.array_equal(multi["n_ok"][comparable], ref["n_ok"][comparable]) and np.array_equal(multi["n_basins"][comparable], ref["n_basins"][comparable])
    agree = comparable & (ref["n_ok"] > 0)
    if agree.any():
        rel = np.abs(multi["obj"][agree] - ref["obj"][agree]) / np.maximum(1.0, np.abs(ref["obj"][agree]))
        print("%s: winner's objective against the oracle's, worst relative difference %.2e over %d instances" % (case.name, rel.max(), agree.sum()))
        assert rel.max() <= 1e-8


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.25
ISENT = -77


class _Raw:
    """The two C entries called with explicit pointers, every output pre-filled with a sentinel."""

    def __init__(self, bs, p):
        self.bs, self.B, self.K = bs, p["B"], p["K"]
        c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)      # noqa: E731
        self.inp = dict(x0=c(p["x0"]), xs=c(p["xs"]), obs=c(p["obs"]), z0=c(p["z0"]))
        self.controls = c(p["controls"])
        self.kind = _obs_kind(p)
        self.dev = {k: (None if v is None else bs.device_array(v.shape).upload(v)) for k, v in self.inp.items()}

    def free(self):
        for v in self.dev.values():
            if v is not None:
                v.free()

    def shapes(self, B, K):
        bs = self.bs
        f = dict(z=(B, bs.nz), obj=(B,), kkt=(B, 4), lam_g=(B, bs.ng), lam_x=(B, bs.nz), z_all=(B, K, bs.nz), obj_all=(B, K))
        i = dict(status=(B,), iters=(B,), which=(B,), n_ok=(B,), n_basins=(B,), status_all=(B, K), iters_all=(B, K))
        return f, i

    ORDER = ("z", "obj", "status", "iters", "kkt", "lam_g", "lam_x", "which", "n_ok", "n_basins", "z_all", "obj_all", "status_all", "iters_all")

    def call(self, device, B=None, K=None, controls="own", obj_margin=1e-9, basin_tol=1e-4, drop=(), alloc=None, **over):
        """alloc: (B, K) the output buffers are sized for, when the call's own B or K are not fit to size anything"""
        B = self.B if B is None else B
        K = self.K if K is None else K
        ctl = self.controls if isinstance(controls, str) else (None if controls is None else np.ascontiguousarray(controls, dtype=np.float64))
        f, i = self.shapes(*(alloc or (B, K)))
        out = {k: np.full(s, SENTINEL) for k, s in f.items()}
        out.update({k: np.full(s, ISENT, np.int32) for k, s in i.items()})
        for k in drop:
            out[k] = None
        if device:
            a = dict(self.dev); a.update(over)
            d = {k: (None if v is None else self.bs.device_array(v.shape, v.dtype).upload(v)) for k, v in out.items()}
            p = lambda v: None if v is None else v.ptr                                          # noqa: E731
            rc = lib().mpcb_solve_multi_device(self.bs._h, B, K, p(a["x0"]), p(a["xs"]), p(a["obs"]), self.kind, p(a["z0"]), dptr(ctl), obj_margin,
                                               basin_tol, *[p(d[k]) for k in self.ORDER], 1)
            out = {k: (None if v is None else v.download()) for k, v in d.items()}
            for v in d.values():
                if v is not None:
                    v.free()
        else:
            a = dict(self.inp); a.update(over)
            ptr = lambda v: None if v is None else (dptr(v) if v.dtype == np.float64 else iptr(v))     # noqa: E731
            rc = lib().mpcb_solve_multi(self.bs._h, B, K, dptr(a["x0"]), dptr(a["xs"]), dptr(a["obs"]), self.kind, dptr(a["z0"]), dptr(ctl), obj_margin,
                                        basin_tol, *[ptr(out[k]) for k in self.ORDER])
        return rc, out


def _untouched(out):
    return all(v is None or (v == (SENTINEL if v.dtype == np.float64 else ISENT)).all() for v in out.values())


def test_refusals_return_their_code_and_leave_the_outputs_alone(gpu_solver_factory):
    p = mc.problem(mc.BY_NAME["kin_caller_z0_k3"], default_config)
    bs = gpu_solver_factory(p["cfg"])
    raw = _Raw(bs, p)
    B, K = p["B"], p["K"]
    bad_ctl = p["controls"].copy(); bad_ctl[2, 1] = np.inf
    nan_ctl = p["controls"].copy(); nan_ctl[1, 0] = np.nan
    nine = mc.turn_starts(9)
    for device in (False, True):
        rc, good = raw.call(device)
        assert rc == 0 and not _untouched(good) and (good["status"] != ISENT).all() and (good["n_basins"] >= 0).all()
        refused = [
            dict(K=0, alloc=(B, K)), dict(K=9, controls=nine, alloc=(B, K)), dict(K=-1, alloc=(B, K)),
            dict(B=-1, alloc=(B, K)),
            dict(B=2 ** 30, K=8, controls=mc.turn_starts(8), alloc=(B, K)),          # K * B = 2^33: beyond int32 and the grid limit
            dict(controls=bad_ctl), dict(controls=nan_ctl),
            dict(controls=None),                                                     # K = 3 without controls
            dict(K=1, controls=None, z0=None, alloc=(B, K)),                         # K = 1 without controls needs a start vector
            dict(drop=("z",)),
            dict(obj_margin=-1e-9), dict(obj_margin=np.nan), dict(obj_margin=np.inf),
            dict(basin_tol=-1.0), dict(basin_tol=np.nan), dict(basin_tol=np.inf),
            dict(x0=None), dict(xs=None), dict(obs=None),
        ]
        for kw in refused:
            rc, out = raw.call(device, **kw)
            assert rc == _abi.E_INVALID and _untouched(out), (device, list(kw), rc)
            assert lib().mpcb_last_error(bs._h)
        rc, out = raw.call(device, B=0, alloc=(B, K))                                # nothing to do is no error
        assert rc == 0 and _untouched(out)
        rc, out = raw.call(device, drop=("obj", "status", "iters", "kkt", "lam_g", "lam_x", "which", "n_ok", "n_basins", "z_all", "obj_all",
                                         "status_all", "iters_all"))                 # every output but z may be NULL
        assert rc == 0 and _bits(out["z"], good["z"])
    bs.set_devices([0])                                                              # a device group
    for device in (False, True):
        rc, out = raw.call(device)
        assert rc == _abi.E_UNSUPPORTED and _untouched(out)
    raw.free()
    bs.close()


# ---- launch lanes, host and device pointers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kin_n30_c2_seed12", "dyn_n40_c4_seed5", "kin_caller_z0_k3"])
def test_lanes_and_pointer_kinds_give_the_same_bits(gpu_solver_factory, name):
    """inflight = 4 against inflight = 1, host against device pointers; with asynchronous solves of other buffers in flight on the lanes
    when the call comes (it waits for them and runs on the handle's own stream)."""
    case = mc.BY_NAME[name]
    p, multi, _ = _run(case, gpu_solver_factory)
    cfg, B, K = p["cfg"], p["B"], p["K"]
    for inflight in (1, 4):
        bs = gpu_solver_factory(cfg, inflight=inflight)
        raw = _Raw(bs, p)
        if inflight > 1:                                         # three plain solves on three lanes, each with buffers of its own
            busy = [[bs.device_array((B, bs.nz)), bs.device_array((B,), np.int32)] for _ in range(3)]
            for z, st in busy:
                bs.solve_device(B, raw.dev["x0"], raw.dev["xs"], raw.dev["obs"], raw.kind, None, z, d_status=st)
        rc, dev = raw.call(True)
        assert rc == 0
        rc, host = raw.call(False)
        assert rc == 0
        for k in _Raw.ORDER:
            assert _bits(dev[k], host[k]), (inflight, k)
            assert _bits(host[k], multi[k]), (inflight, k)
        raw.free()
        bs.close()
