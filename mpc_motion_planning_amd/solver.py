"""BatchSolver — thin Python front of the C ABI (include/mpcbatch.h) for batches of MPC instances.

This is the batched extension of the reference's per-step  `solver = ca.nlpsol(...)` / `res = solver(x0=, p=, ...)`
pair (CasaDi_MPC_Optimize_Multishoot/MPC_CBF_optimize_kin.py:251-254, main_cbf_kin_c_sim.py:100): one handle per
NLP structure, one call per batch of parameter vectors and obstacle sets.  numpy + ctypes only.
"""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import MpcbConfig, dptr, iptr
from ._lib import lib, check


def default_config(model=_abi.MODEL_KIN, N=30, T=0.1, n_obs=0):
    cfg = MpcbConfig()
    check(lib().mpcb_default_config(C.byref(cfg), model, N, T))
    cfg.n_obs = n_obs
    return cfg


def dims(cfg):
    nx, nz, ng = C.c_int32(), C.c_int32(), C.c_int32()
    check(lib().mpcb_dims(C.byref(cfg), C.byref(nx), C.byref(nz), C.byref(ng)))
    return nx.value, nz.value, ng.value


def device_count():
    return lib().mpcb_device_count()


def shard_bounds(B, world, rank):
    """Contiguous slice [lo, hi) of `rank` among `world` (mpcb_shard_bounds: the rule the library itself shards with)."""
    lo, hi = C.c_int64(), C.c_int64()
    check(lib().mpcb_shard_bounds(int(B), int(world), int(rank), C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def comm_unique_id():
    """128 bytes that identify a new RCCL group (ncclGetUniqueId); rank 0 makes them, every rank passes them to comm_init."""
    buf = C.create_string_buffer(_abi.UNIQUE_ID_BYTES)
    check(lib().mpcb_comm_unique_id(C.cast(buf, C.c_void_p)))
    return buf.raw


def model_rhs(cfg, x, u):
    """f(x,u) of the configured model (the reference's `mpc_solver.f`, kin.py:159)."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
    u = np.ascontiguousarray(np.asarray(u, dtype=np.float64).reshape(-1))
    out = np.zeros(cfg.nx())
    check(lib().mpcb_model_rhs(C.byref(cfg), dptr(x), dptr(u), dptr(out)))
    return out


def turn_starts(K=3, steer=0.03, accel=0.0):
    """The K constant-control starts of solve_multi, [K, 2] rows (steer, accel): straight on, then a slight turn to either side, then
    twice that turn, ...:  [[0, a], [+s, a], [-s, a], [+2s, a], [-2s, a], ...] cut to K rows."""
    K = int(K)
    if K < 1:
        raise ValueError("K must be >= 1")
    rows = [[0.0, float(accel)]]
    m = 1
    while len(rows) < K:
        rows.append([m * float(steer), float(accel)])
        rows.append([-m * float(steer), float(accel)])
        m += 1
    return np.array(rows[:K], dtype=np.float64)


def vary(cfg, B, **fields):
    """A ctypes array of B configs copied from `cfg`, with each named field set per instance from an array of shape [B] (scalar
    fields) or [B, k] (array fields of length k):  vary(cfg, B, Q=q[B,4], veh_l=l[B]).  An array field may be given fewer columns
    than it has (Q is [6], the kinematic model uses 4); the rest keep cfg's values.  The result is what BatchSolver.params takes."""
    B = int(B)
    if B < 1:
        raise ValueError("B must be >= 1")
    types = dict(MpcbConfig._fields_)
    cols = {}
    for name, val in fields.items():
        if name not in types:
            raise ValueError("mpcb_config has no field %r" % name)
        ftype = types[name]
        v = np.asarray(val)
        if issubclass(ftype, C.Array):
            if v.ndim != 2 or v.shape[0] != B or not 1 <= v.shape[1] <= ftype._length_:
                raise ValueError("%s must be [B, k] = [%d, 1..%d], got %s" % (name, B, ftype._length_, v.shape))
            cols[name] = v.astype(np.float64)
        else:
            if v.shape != (B,):
                raise ValueError("%s must be [B] = [%d], got %s" % (name, B, v.shape))
            if ftype is C.c_double:
                cols[name] = v.astype(np.float64)
            else:
                if not np.all(np.asarray(v, dtype=np.float64) == np.round(np.asarray(v, dtype=np.float64))):
                    raise ValueError("%s is an integer field, got non-integral values" % name)
                cols[name] = np.asarray(v, dtype=np.float64).astype(np.int64)
    out = (MpcbConfig * B)()
    for b in range(B):
        C.memmove(C.byref(out[b]), C.byref(cfg), C.sizeof(MpcbConfig))
        for name, v in cols.items():
            if v.ndim == 2:
                arr = getattr(out[b], name)
                for i in range(v.shape[1]):
                    arr[i] = v[b, i]
            else:
                setattr(out[b], name, v[b].item())
    return out


class ParamSet:
    """A validated, device-resident, read-only set of per-instance configs (mpcb_params_create); made by BatchSolver.params.
    Pass it as `params=` to solve_batch / solve_device / closed_loop; close() it (or use it as a context manager) before the solver.
    Closing the solver first is safe as well: mpcb_destroy frees the sets it still holds, and close() then has nothing left to do."""

    def __init__(self, solver, ptr, B):
        self.solver, self.ptr, self.B = solver, ptr, int(B)

    def close(self):
        if self.ptr is not None and self.solver._h:
            check(lib().mpcb_params_destroy(self.solver._h, self.ptr), self.solver._h)
        self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class DeviceArray:
    """A caller-owned device buffer (row-major, float64 or int32)."""

    def __init__(self, solver, shape, dtype=np.float64):
        self.solver = solver
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        check(lib().mpcb_dev_alloc(solver._h, self.nbytes, C.byref(p)), solver._h)
        self.ptr = p

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.size * a.itemsize == self.nbytes, "size mismatch"
        check(lib().mpcb_dev_upload(self.solver._h, self.ptr, a.ctypes.data_as(C.c_void_p), self.nbytes), self.solver._h)
        return self

    def download(self):
        out = np.empty(self.shape, dtype=self.dtype)
        check(lib().mpcb_dev_download(self.solver._h, out.ctypes.data_as(C.c_void_p), self.ptr, self.nbytes), self.solver._h)
        return out

    def free(self):
        if self.ptr is not None and self.solver._h:
            lib().mpcb_dev_free(self.solver._h, self.ptr)
        self.ptr = None


def _devptr(v):
    """c_void_p of a DeviceArray / int / c_void_p (None stays None)."""
    if v is None:
        return None
    if isinstance(v, DeviceArray):
        return v.ptr
    return v if isinstance(v, C.c_void_p) else C.c_void_p(int(v))


class ControlLoop:
    """One receding-horizon controller for B instances whose state (warm start, counters) stays on the device between steps
    (mpcb_loop_create); made by BatchSolver.loop.  The caller steps its own plant: `step` takes this step's states, set-points,
    obstacles and (optionally) stage references and returns the control to apply.  close() it (or use it as a context manager)
    before the solver; closing the solver first is safe as well."""

    def __init__(self, solver, ptr, B, hold_on_failure, predict, params):
        self.solver, self.ptr, self.B = solver, ptr, int(B)
        self.hold_on_failure, self.predict, self.params = bool(hold_on_failure), bool(predict), params

    def close(self):
        if self.ptr is not None and self.solver._h:
            check(lib().mpcb_loop_destroy(self.solver._h, self.ptr), self.solver._h)
        self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def step(self, x0, xs, obs=None, x_ref=None, want_z=True):
        """x0, xs [B,nx]; obs [B,n_obs,6] | [B,n_obs,N+1,6]; x_ref [B,N,nx] | None  ->  dict(u0 [B,2], status, iters, z, obj).
        u0 is the first control of the executed plan (with hold_on_failure: of the previous plan where this step's solve failed);
        z, obj, status and iters are the solve's own.  want_z=False leaves the iterate on the device (z is None): per instance only
        u0, status, iters and obj come back."""
        s, B = self.solver, self.B
        x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64))
        xs = np.ascontiguousarray(np.asarray(xs, dtype=np.float64))
        if x0.shape != (B, s.nx) or xs.shape != (B, s.nx):
            raise ValueError("x0 and xs must be [B,%d] = [%d,%d]" % (s.nx, B, s.nx))
        if x_ref is not None:
            x_ref = np.ascontiguousarray(np.asarray(x_ref, dtype=np.float64))
            if x_ref.shape != (B, s.N, s.nx):
                raise ValueError("x_ref must be [B,N,nx] = [%d,%d,%d], got %s" % (B, s.N, s.nx, x_ref.shape))
        obs, kind = s._obs(obs, B)
        u0 = np.empty((B, 2)); z = np.empty((B, s.nz)) if want_z else None
        obj = np.empty(B); st = np.empty(B, np.int32); it = np.empty(B, np.int32)
        check(lib().mpcb_loop_step(s._h, self.ptr, dptr(x0), dptr(xs), dptr(x_ref), dptr(obs), kind, dptr(u0), iptr(st), iptr(it), dptr(z),
                                   dptr(obj)), s._h)
        return dict(u0=u0, status=st, iters=it, z=z, obj=obj)

    def step_device(self, d_x0, d_xs, d_u0, d_obs=None, obs_kind=_abi.OBSIN_STATIC, d_x_ref=None, d_status=None, d_iters=None, d_z=None,
                    d_obj=None, sync=False):
        """step on device buffers (DeviceArray / raw pointers), asynchronous on the loop's lane unless sync."""
        s = self.solver
        check(lib().mpcb_loop_step_device(s._h, self.ptr, _devptr(d_x0), _devptr(d_xs), _devptr(d_x_ref), _devptr(d_obs), int(obs_kind),
                                          _devptr(d_u0), _devptr(d_status), _devptr(d_iters), _devptr(d_z), _devptr(d_obj), 1 if sync else 0), s._h)

    def advance_device(self, d_x0, d_u0, d_obs=None, first_only=False, sync=False):
        """The library's plant step d_x0 <- d_x0 + T f(d_x0, d_u0) and one constant-velocity step of the obstacles in d_obs [B,n_obs,6]
        (first_only: of obstacle 0 alone; None: of none), on the loop's lane: the other half of closed_loop's step."""
        s = self.solver
        check(lib().mpcb_loop_advance_device(s._h, self.ptr, _devptr(d_x0), _devptr(d_u0), _devptr(d_obs),
                                             _abi.CL_ADVANCE_FIRST_ONLY if first_only else 0, 1 if sync else 0), s._h)

    def reset(self, mask=None):
        """Warm start and counters back to zero: every instance, or those where mask [B] is true (an episode restarts)."""
        if mask is not None:
            mask = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.int32)
            if mask.shape != (self.B,):
                raise ValueError("mask must be [B] = [%d]" % self.B)
        check(lib().mpcb_loop_reset(self.solver._h, self.ptr, iptr(mask)), self.solver._h)

    @property
    def start(self):
        """The warm start [B,nz] the next step solves from (the executed plan shifted one stage; zero after create / reset)."""
        w = np.empty((self.B, self.solver.nz))
        check(lib().mpcb_loop_get_start(self.solver._h, self.ptr, dptr(w)), self.solver._h)
        return w

    @start.setter
    def start(self, w):
        w = np.ascontiguousarray(np.asarray(w, dtype=np.float64))
        if w.shape != (self.B, self.solver.nz):
            raise ValueError("start must be [B,nz] = [%d,%d], got %s" % (self.B, self.solver.nz, w.shape))
        check(lib().mpcb_loop_set_start(self.solver._h, self.ptr, dptr(w)), self.solver._h)

    def _counters(self):
        n = np.empty(self.B, np.int32); f = np.empty(self.B, np.int32)
        check(lib().mpcb_loop_counters(self.solver._h, self.ptr, iptr(n), iptr(f)), self.solver._h)
        return n, f

    @property
    def steps(self):
        """Steps per instance since the last reset [B]."""
        return self._counters()[0]

    @property
    def failures(self):
        """Steps per instance since the last reset whose solve ended neither solved nor acceptable [B]."""
        return self._counters()[1]


class BatchSolver:
    def __init__(self, cfg, device=0, inflight=1):
        """inflight: launch lanes of the handle (mpcb_set_inflight).  With k > 1 consecutive asynchronous `solve_device` calls
        overlap on the GPU and one large call is cut into chunks that do; results do not depend on it."""
        self.cfg = cfg.copy()
        self._h = C.c_void_p()
        rc = lib().mpcb_create(C.byref(self.cfg), device, C.byref(self._h))
        if rc != 0:
            check(rc, None)
        self.nx, self.nz, self.ng = dims(self.cfg)
        self.N = self.cfg.N
        self.device = device
        self.inflight = 1
        if inflight != 1:
            self.set_inflight(inflight)

    def set_inflight(self, k):
        check(lib().mpcb_set_inflight(self._h, int(k)), self._h)
        self.inflight = int(k)

    def close(self):
        if self._h:
            lib().mpcb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------------
    def set_bounds(self, lbx, ubx, lbg, ubg):
        """Adopt (and validate) the four lists `initialize_constraints` returns (kin.py:84-134)."""
        lbx = np.ascontiguousarray(lbx, dtype=np.float64); ubx = np.ascontiguousarray(ubx, dtype=np.float64)
        lbg = np.ascontiguousarray(lbg, dtype=np.float64); ubg = np.ascontiguousarray(ubg, dtype=np.float64)
        if lbx.shape != ubx.shape or lbg.shape != ubg.shape:
            raise ValueError("lbx/ubx or lbg/ubg lengths differ")
        check(lib().mpcb_set_bounds(self._h, dptr(lbx), dptr(ubx), lbx.size, dptr(lbg), dptr(ubg), lbg.size), self._h)

    def set_time_grid(self, T_i=None):
        """Step length of every stage (N values), or None for cfg.T everywhere (the reference's behaviour)."""
        if T_i is None:
            check(lib().mpcb_set_time_grid(self._h, None, 0), self._h)
        else:
            t = np.ascontiguousarray(T_i, dtype=np.float64).reshape(-1)
            check(lib().mpcb_set_time_grid(self._h, dptr(t), t.size), self._h)

    def _obs(self, obs, B):
        if self.cfg.n_obs == 0:
            return None, _abi.OBSIN_STATIC
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        n = self.cfg.n_obs
        if obs.size == B * n * 6:
            return obs.reshape(B, n, 6), _abi.OBSIN_STATIC
        if obs.size == B * n * (self.N + 1) * 6:
            return obs.reshape(B, n, self.N + 1, 6), _abi.OBSIN_PREDICTED
        raise ValueError("obs has %d values; expected [B,%d,6] or [B,%d,%d,6]" % (obs.size, n, n, self.N + 1))

    def params(self, cfgs):
        """A ParamSet from B configs (the array vary() returns, or a sequence of MpcbConfig): row b is the config instance b is solved
        under.  Every row must pass the checks of BatchSolver(cfg) and equal this solver's config in every structural field
        (include/mpcbatch.h, mpcb_params_create); a row that does not raises ValueError with the library's message and the row's index."""
        if not (isinstance(cfgs, C.Array) and cfgs._type_ is MpcbConfig):
            rows = list(cfgs)
            arr = (MpcbConfig * len(rows))()
            for b, r in enumerate(rows):
                C.memmove(C.byref(arr[b]), C.byref(r), C.sizeof(MpcbConfig))
            cfgs = arr
        B = len(cfgs)
        p = C.c_void_p(); bad = C.c_int32(-1)
        rc = lib().mpcb_params_create(self._h, cfgs, B, C.byref(p), C.byref(bad))
        if rc == _abi.E_INVALID:
            msg = lib().mpcb_last_error(self._h)
            raise ValueError("parameter set rejected, first bad row %d: %s" % (bad.value, msg.decode("utf-8", "replace") if msg else ""))
        check(rc, self._h)
        return ParamSet(self, p, B)

    def loop(self, B, hold_on_failure=False, predict=False, params=None):
        """A ControlLoop of B instances (mpcb_loop_create): the receding-horizon controller one step at a time, for a plant, obstacles
        and episode ends that are the caller's.  hold_on_failure: a step whose solve fails applies and keeps the previous plan.
        predict: static obstacle rows [B,n_obs,6] given to a step are rolled out at constant velocity over the horizon before the solve.
        params: a ParamSet of B rows, instance b is solved (and advanced by advance_device) under row b."""
        flags = (_abi.CL_HOLD_ON_FAILURE if hold_on_failure else 0) | (_abi.LOOP_PREDICT if predict else 0)
        p = C.c_void_p()
        check(lib().mpcb_loop_create(self._h, int(B), flags, params.ptr if params is not None else None, C.byref(p)), self._h)
        return ControlLoop(self, p, B, hold_on_failure, predict, params)

    def solve_batch(self, x0, xs, obs=None, z0=None, multipliers=False, x_ref=None, params=None):
        """x0, xs [B,nx]; obs [B,n_obs,6] | [B,n_obs,N+1,6]; z0 [B,nz] | None  ->  dict(z, obj, status, iters, kkt[, lam_g, lam_x])
        x_ref [B,N,nx] | None: per-stage reference, row i replaces xs in stage i's cost (mpcb_solve_ref; kinematic model only).
        params: a ParamSet of B rows, instance b is solved under row b (mpcb_solve_params); not together with x_ref."""
        if params is not None and x_ref is not None:
            raise ValueError("params and x_ref cannot be combined: the parameter sets have no tracking kernels")
        x0 = np.ascontiguousarray(np.atleast_2d(np.asarray(x0, dtype=np.float64)))
        xs = np.ascontiguousarray(np.atleast_2d(np.asarray(xs, dtype=np.float64)))
        B = x0.shape[0]
        if x0.shape != (B, self.nx) or xs.shape != (B, self.nx):
            raise ValueError("x0 and xs must be [B,%d]" % self.nx)
        if x_ref is not None:
            x_ref = np.ascontiguousarray(np.asarray(x_ref, dtype=np.float64))
            if x_ref.shape != (B, self.N, self.nx):
                raise ValueError("x_ref must be [B,N,nx] = [%d,%d,%d], got %s" % (B, self.N, self.nx, x_ref.shape))
        obs, kind = self._obs(obs, B)
        if z0 is not None:
            z0 = np.ascontiguousarray(np.asarray(z0, dtype=np.float64).reshape(B, self.nz))
        z = np.empty((B, self.nz)); obj = np.empty(B); st = np.empty(B, np.int32); it = np.empty(B, np.int32)
        kkt = np.empty((B, 4))
        lam_g = np.empty((B, self.ng)) if multipliers else None
        lam_x = np.empty((B, self.nz)) if multipliers else None
        if params is not None:
            check(lib().mpcb_solve_params(self._h, B, params.ptr, dptr(x0), dptr(xs), dptr(obs), kind, dptr(z0), dptr(z), dptr(obj), iptr(st),
                                          iptr(it), dptr(kkt), dptr(lam_g), dptr(lam_x)), self._h)
        elif x_ref is None:
            check(lib().mpcb_solve(self._h, B, dptr(x0), dptr(xs), dptr(obs), kind, dptr(z0), dptr(z), dptr(obj), iptr(st),
                                   iptr(it), dptr(kkt), dptr(lam_g), dptr(lam_x)), self._h)
        else:
            check(lib().mpcb_solve_ref(self._h, B, dptr(x0), dptr(xs), dptr(x_ref), dptr(obs), kind, dptr(z0), dptr(z), dptr(obj),
                                       iptr(st), iptr(it), dptr(kkt), dptr(lam_g), dptr(lam_x)), self._h)
        out = dict(z=z, obj=obj, status=st, iters=it, kkt=kkt)
        if multipliers:
            out["lam_g"] = lam_g; out["lam_x"] = lam_x
        return out

    def solve_trace(self, x0, xs, obs=None, z0=None):
        """One instance with its iteration log: dict(z, status, iters, trace[iters+1, 8]) with trace columns
        mu, scaled error, theta, f, alpha_primal_max, alpha, alpha_dual, delta_w."""
        x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(1, self.nx)); xs = np.ascontiguousarray(np.asarray(xs, dtype=np.float64).reshape(1, self.nx))
        obs, kind = self._obs(obs, 1)
        if z0 is not None:
            z0 = np.ascontiguousarray(np.asarray(z0, dtype=np.float64).reshape(1, self.nz))
        z = np.empty((1, self.nz)); st = np.empty(1, np.int32); it = np.empty(1, np.int32); tr = np.zeros((self.cfg.max_iter + 1, 8))
        check(lib().mpcb_solve_trace(self._h, dptr(x0), dptr(xs), dptr(obs), kind, dptr(z0), dptr(z), iptr(st), iptr(it), dptr(tr)), self._h)
        return dict(z=z[0], status=int(st[0]), iters=int(it[0]), trace=tr[: int(it[0]) + 1])

    def closed_loop(self, x0, xs, obs_state=None, steps=80, obs_motion=_abi.OBSMOVE_STATIC, hold_on_failure=False,
                    advance_first_only=False, aa=0.0, params=None):
        """Receding-horizon loop on the device (main_cbf_kin_c_sim.py:87-123).  obs_motion: OBSMOVE_STATIC (obstacles fixed,
        main_cbf_kin_c_sim.py), OBSMOVE_PREDICTED (constant-velocity obstacles predicted per solve and advanced per step,
        main_cbf_kin_c_sim_pre.py), OBSMOVE_CURRENT (advanced, no prediction).
        hold_on_failure: a step whose solve fails applies the previous plan (hold-and-shift) instead of the failed iterate.
        advance_first_only: only obstacle 0 moves between steps (main_cbf_kin_c_sim_pre.py:106).
        aa: blend weight of the path window in the stage cost (kin.py:194-199, mpcb_closed_loop_ref); 0 = the set-point loop.
        params: a ParamSet of B rows: solve and plant step of instance b under row b (mpcb_closed_loop_params); not with aa != 0.
        Returns dict(x_hist, u_hist, status, iters, obs_state)."""
        x0 = np.ascontiguousarray(np.atleast_2d(np.asarray(x0, dtype=np.float64)))
        xs = np.ascontiguousarray(np.atleast_2d(np.asarray(xs, dtype=np.float64)))
        B = x0.shape[0]
        aa = float(aa)
        if params is not None and aa != 0.0:
            raise ValueError("params and aa != 0 cannot be combined: the parameter sets have no tracking kernels")
        if aa != 0.0:
            if x0.shape != (B, self.nx) or xs.shape != (B, self.nx):
                raise ValueError("x0 and xs must be [B,%d]" % self.nx)
        ob = None
        if self.cfg.n_obs:
            ob = np.array(obs_state, dtype=np.float64).reshape(B, self.cfg.n_obs, 6).copy()
        xh = np.empty((B, steps + 1, self.nx)); uh = np.empty((B, steps, 2))
        st = np.empty((B, steps), np.int32); it = np.empty((B, steps), np.int32)
        flags = (_abi.CL_HOLD_ON_FAILURE if hold_on_failure else 0) | (_abi.CL_ADVANCE_FIRST_ONLY if advance_first_only else 0)
        if params is not None:
            check(lib().mpcb_closed_loop_params(self._h, B, steps, params.ptr, dptr(x0), dptr(xs), dptr(ob), int(obs_motion), flags, dptr(xh),
                                                dptr(uh), iptr(st), iptr(it)), self._h)
        elif aa == 0.0:
            check(lib().mpcb_closed_loop(self._h, B, steps, dptr(x0), dptr(xs), dptr(ob), int(obs_motion), flags, dptr(xh), dptr(uh),
                                         iptr(st), iptr(it)), self._h)
        else:
            check(lib().mpcb_closed_loop_ref(self._h, B, steps, dptr(x0), dptr(xs), dptr(ob), int(obs_motion), flags, aa, dptr(xh),
                                             dptr(uh), iptr(st), iptr(it)), self._h)
        return dict(x_hist=xh, u_hist=uh, status=st, iters=it, obs_state=ob)

    # ----- scene generation on the device (include/mpcbatch.h, "scene generation") ----------------------------------
    def sample_scenes(self, kind, B, seed, first_index=0):
        """B scenes of distribution `kind` (_abi.SCENES_C2 / C3 / C4) drawn on the device with the counter-based generator;
        scene i of a population is the same whichever call or GPU draws it (global index first_index + i).  Downloads
        (x0 [B,nx], xs [B,nx], obs [B,n_obs,6])."""
        no = self.cfg.n_obs
        d_x0 = self.device_array((B, self.nx)); d_xs = self.device_array((B, self.nx)); d_ob = self.device_array((B, max(no, 1), 6))
        check(lib().mpcb_sample_scenes(self._h, int(kind), int(B), int(seed), int(first_index), d_x0.ptr, d_xs.ptr, d_ob.ptr), self._h)
        self.sync()
        out = d_x0.download(), d_xs.download(), d_ob.download()[:, :no]
        for d in (d_x0, d_xs, d_ob):
            d.free()
        return out

    def closed_loop_sampled(self, kind, B, seed, first_index=0, steps=80, obs_motion=_abi.OBSMOVE_STATIC, hold_on_failure=False,
                            advance_first_only=False):
        """closed_loop on scenes drawn on the device; also returns the scenes (x0, obs0)."""
        no = self.cfg.n_obs
        x0 = np.empty((B, self.nx)); ob = np.empty((B, no, 6)) if no else None
        xh = np.empty((B, steps + 1, self.nx)); uh = np.empty((B, steps, 2))
        st = np.empty((B, steps), np.int32); it = np.empty((B, steps), np.int32)
        flags = (_abi.CL_HOLD_ON_FAILURE if hold_on_failure else 0) | (_abi.CL_ADVANCE_FIRST_ONLY if advance_first_only else 0)
        check(lib().mpcb_closed_loop_sampled(self._h, int(kind), int(B), int(seed), int(first_index), int(steps), int(obs_motion), flags,
                                             dptr(x0), dptr(ob), dptr(xh), dptr(uh), iptr(st), iptr(it)), self._h)
        return dict(x0=x0, obs0=ob, x_hist=xh, u_hist=uh, status=st, iters=it)

    def predict_obstacles(self, obs, dt, N):
        """Device twin of Obs_prediction.obs_prediction: obs [n,6] -> [n,N+1,6]."""
        obs = np.ascontiguousarray(np.asarray(obs, dtype=np.float64).reshape(-1, 6))
        out = np.empty((len(obs), N + 1, 6))
        check(lib().mpcb_predict_obstacles(self._h, len(obs), int(N), float(dt), dptr(obs), dptr(out)), self._h)
        return out

    def ref_path_window(self, x_start, x0, xs, T_horizon, dt, last_idx):
        """Device twin of RefPathGenerator.define_ref_path + find_ref_traj for B instances: (window [B,N_p+1,4], min_idx [B])."""
        x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(-1, 4)); xs = np.ascontiguousarray(np.asarray(xs, dtype=np.float64).reshape(-1, 4))
        li = np.ascontiguousarray(np.asarray(last_idx, dtype=np.int32).reshape(-1))
        win = np.empty((len(x0), int(T_horizon / dt) + 1, 4))
        check(lib().mpcb_ref_path_window(self._h, len(x0), float(x_start), dptr(x0), dptr(xs), float(T_horizon), float(dt), iptr(li), dptr(win)), self._h)
        return win, li

    # ----- device-resident path (bench.py, multi-GPU plumbing) -------------------------------------------
    def device_array(self, shape, dtype=np.float64):
        return DeviceArray(self, shape, dtype)

    def solve_device(self, B, d_x0, d_xs, d_obs, obs_kind, d_z0, d_z, d_obj=None, d_status=None, d_iters=None, d_kkt=None,
                     d_lam_g=None, d_lam_x=None, sync=False, d_x_ref=None, params=None):
        """Raw device pointers (ints / c_void_p / DeviceArray).  Asynchronous on the handle's stream unless sync.
        d_x_ref [B,N,nx]: per-stage reference (mpcb_solve_device_ref).  params: a ParamSet of B rows (mpcb_solve_device_params)."""
        if params is not None and d_x_ref is not None:
            raise ValueError("params and d_x_ref cannot be combined: the parameter sets have no tracking kernels")
        def p(v):
            if v is None:
                return None
            if isinstance(v, DeviceArray):
                return v.ptr
            return C.c_void_p(int(v)) if not isinstance(v, C.c_void_p) else v
        if params is not None:
            check(lib().mpcb_solve_device_params(self._h, B, params.ptr, p(d_x0), p(d_xs), p(d_obs), obs_kind, p(d_z0), p(d_z), p(d_obj),
                                                 p(d_status), p(d_iters), p(d_kkt), p(d_lam_g), p(d_lam_x), 1 if sync else 0), self._h)
        elif d_x_ref is None:
            check(lib().mpcb_solve_device(self._h, B, p(d_x0), p(d_xs), p(d_obs), obs_kind, p(d_z0), p(d_z), p(d_obj), p(d_status),
                                          p(d_iters), p(d_kkt), p(d_lam_g), p(d_lam_x), 1 if sync else 0), self._h)
        else:
            check(lib().mpcb_solve_device_ref(self._h, B, p(d_x0), p(d_xs), p(d_x_ref), p(d_obs), obs_kind, p(d_z0), p(d_z), p(d_obj),
                                              p(d_status), p(d_iters), p(d_kkt), p(d_lam_g), p(d_lam_x), 1 if sync else 0), self._h)

    # ----- multi-start solve (include/mpcbatch_multi.h) ------------------------------------------------------
    @staticmethod
    def _controls(controls):
        """[K, 2] float64 rows of (steer, accel); None means turn_starts(3)."""
        if controls is None:
            return turn_starts(3)
        c = np.ascontiguousarray(np.asarray(controls, dtype=np.float64))
        if c.ndim != 2 or c.shape[1] != 2 or c.shape[0] < 1:
            raise ValueError("controls must be [K, 2] rows of (steer, accel), got %s" % (c.shape,))
        return c

    def solve_multi(self, x0, xs, obs=None, z0=None, controls=None, multipliers=False, obj_margin=1e-9, basin_tol=1e-4, want_all=False):
        """Every instance solved from K starts in one launch of K * B instances, the cheapest solution kept (mpcb_solve_multi).
        controls [K,2] rows of (steer, accel) held over the horizon, None = turn_starts(3); z0 [B,nz] | None: the caller's start of
        candidate 0, used verbatim.  A later candidate replaces the incumbent only if its objective is lower by more than
        obj_margin * max(1, |obj|); two solutions count as one when they differ by at most basin_tol in every entry of z.
        Returns the dict of solve_batch (the winner's z, obj, status, iters, kkt[, lam_g, lam_x]) plus which [B] (the winner's index),
        n_ok [B] (candidates that solved) and n_basins [B] (distinct solutions found); with want_all also z_all [B,K,nz], obj_all,
        status_all, iters_all [B,K]."""
        x0 = np.ascontiguousarray(np.atleast_2d(np.asarray(x0, dtype=np.float64)))
        xs = np.ascontiguousarray(np.atleast_2d(np.asarray(xs, dtype=np.float64)))
        B = x0.shape[0]
        if x0.shape != (B, self.nx) or xs.shape != (B, self.nx):
            raise ValueError("x0 and xs must be [B,%d]" % self.nx)
        obs, kind = self._obs(obs, B)
        if z0 is not None:
            z0 = np.ascontiguousarray(np.asarray(z0, dtype=np.float64).reshape(B, self.nz))
        c = self._controls(controls)
        K = c.shape[0]
        z = np.empty((B, self.nz)); obj = np.empty(B); st = np.empty(B, np.int32); it = np.empty(B, np.int32); kkt = np.empty((B, 4))
        lam_g = np.empty((B, self.ng)) if multipliers else None
        lam_x = np.empty((B, self.nz)) if multipliers else None
        which = np.empty(B, np.int32); n_ok = np.empty(B, np.int32); n_basins = np.empty(B, np.int32)
        z_all = np.empty((B, K, self.nz)) if want_all else None
        obj_all = np.empty((B, K)) if want_all else None
        st_all = np.empty((B, K), np.int32) if want_all else None
        it_all = np.empty((B, K), np.int32) if want_all else None
        check(lib().mpcb_solve_multi(self._h, B, K, dptr(x0), dptr(xs), dptr(obs), kind, dptr(z0), dptr(c), float(obj_margin), float(basin_tol),
                                     dptr(z), dptr(obj), iptr(st), iptr(it), dptr(kkt), dptr(lam_g), dptr(lam_x), iptr(which), iptr(n_ok),
                                     iptr(n_basins), dptr(z_all), dptr(obj_all), iptr(st_all), iptr(it_all)), self._h)
        out = dict(z=z, obj=obj, status=st, iters=it, kkt=kkt, which=which, n_ok=n_ok, n_basins=n_basins)
        if multipliers:
            out["lam_g"] = lam_g; out["lam_x"] = lam_x
        if want_all:
            out.update(z_all=z_all, obj_all=obj_all, status_all=st_all, iters_all=it_all)
        return out

    def solve_multi_device(self, B, d_x0, d_xs, d_obs, obs_kind, d_z0, d_z, controls=None, obj_margin=1e-9, basin_tol=1e-4, d_obj=None,
                           d_status=None, d_iters=None, d_kkt=None, d_lam_g=None, d_lam_x=None, d_which=None, d_n_ok=None, d_n_basins=None,
                           d_z_all=None, d_obj_all=None, d_status_all=None, d_iters_all=None, sync=False):
        """mpcb_solve_multi_device over raw device pointers (ints / c_void_p / DeviceArray), like solve_device; controls stays a host
        array [K,2] (None = turn_starts(3)).  Waits for the launch lanes and runs on the handle's own stream, asynchronous unless sync.
        d_*_all are [B,K,...] over the expanded batch, row b * K + k."""
        c = self._controls(controls)
        check(lib().mpcb_solve_multi_device(self._h, int(B), c.shape[0], _devptr(d_x0), _devptr(d_xs), _devptr(d_obs), int(obs_kind), _devptr(d_z0),
                                            dptr(c), float(obj_margin), float(basin_tol), _devptr(d_z), _devptr(d_obj), _devptr(d_status),
                                            _devptr(d_iters), _devptr(d_kkt), _devptr(d_lam_g), _devptr(d_lam_x), _devptr(d_which), _devptr(d_n_ok),
                                            _devptr(d_n_basins), _devptr(d_z_all), _devptr(d_obj_all), _devptr(d_status_all), _devptr(d_iters_all),
                                            1 if sync else 0), self._h)

    # ----- evaluate and certify a point (include/mpcbatch.h, "evaluate and certify any point") -------------------------
    def evaluate(self, x0, xs, obs, z, lam_g=None, lam_x=None, x_ref=None, params=None, want_g=True, want_grad=False):
        """What the NLP says about the points z [B,nz], solved or not (mpcb_evaluate): dict(obj [B], g [B,ng] | None, grad_lag [B,nz] | None,
        feas_g, feas_x, h_min, stationarity, compl, sign, lam_scale [B] each).  lam_g [B,ng] and lam_x [B,nz]: both or neither; without
        them stationarity, compl, sign and lam_scale are NaN and want_grad is refused by the library.  x_ref [B,N,nx]: the tracking
        objective (kinematic model).  params: a ParamSet of B rows, instance b is evaluated under row b."""
        x0 = np.ascontiguousarray(np.atleast_2d(np.asarray(x0, dtype=np.float64)))
        xs = np.ascontiguousarray(np.atleast_2d(np.asarray(xs, dtype=np.float64)))
        B = x0.shape[0]
        if x0.shape != (B, self.nx) or xs.shape != (B, self.nx):
            raise ValueError("x0 and xs must be [B,%d]" % self.nx)
        if x_ref is not None:
            x_ref = np.ascontiguousarray(np.asarray(x_ref, dtype=np.float64))
            if x_ref.shape != (B, self.N, self.nx):
                raise ValueError("x_ref must be [B,N,nx] = [%d,%d,%d], got %s" % (B, self.N, self.nx, x_ref.shape))
        obs, kind = self._obs(obs, B)
        z = np.ascontiguousarray(np.asarray(z, dtype=np.float64).reshape(B, self.nz))
        if lam_g is not None:
            lam_g = np.ascontiguousarray(np.asarray(lam_g, dtype=np.float64).reshape(B, self.ng))
        if lam_x is not None:
            lam_x = np.ascontiguousarray(np.asarray(lam_x, dtype=np.float64).reshape(B, self.nz))
        obj = np.empty(B); res = np.empty((B, _abi.EVAL_COLS))
        g = np.empty((B, self.ng)) if want_g else None
        grad = np.empty((B, self.nz)) if want_grad else None
        check(lib().mpcb_evaluate(self._h, B, params.ptr if params is not None else None, dptr(x0), dptr(xs), dptr(x_ref), dptr(obs), kind,
                                  dptr(z), dptr(lam_g), dptr(lam_x), dptr(obj), dptr(g), dptr(grad), dptr(res)), self._h)
        out = dict(obj=obj, g=g, grad_lag=grad)
        out.update({name: res[:, i].copy() for i, name in enumerate(_abi.EVAL_NAMES)})
        return out

    def evaluate_device(self, B, d_x0, d_xs, d_obs, obs_kind, d_z, d_lam_g=None, d_lam_x=None, d_obj=None, d_g=None, d_grad_lag=None,
                        d_res=None, sync=False, d_x_ref=None, params=None):
        """mpcb_evaluate_device over raw device pointers (ints / c_void_p / DeviceArray), like solve_device.  Queued behind the handle's most
        recent solve_device call, on its lane; d_res is [B, 7] in the order of _abi.EVAL_NAMES."""
        check(lib().mpcb_evaluate_device(self._h, B, params.ptr if params is not None else None, _devptr(d_x0), _devptr(d_xs), _devptr(d_x_ref),
                                         _devptr(d_obs), obs_kind, _devptr(d_z), _devptr(d_lam_g), _devptr(d_lam_x), _devptr(d_obj), _devptr(d_g),
                                         _devptr(d_grad_lag), _devptr(d_res), 1 if sync else 0), self._h)

    # ----- multi-GPU (include/mpcbatch.h, "multi-GPU") ------------------------------------------------------
    def set_devices(self, ids):
        """One process driving several devices: solve_batch then shards the batch over them and all-gathers z (RCCL)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        check(lib().mpcb_set_devices(self._h, iptr(ids), len(ids)), self._h)

    def comm_init(self, unique_id, rank, world):
        """One process per GPU: join the RCCL group identified by `unique_id` (comm_unique_id() of rank 0)."""
        buf = C.create_string_buffer(bytes(unique_id), _abi.UNIQUE_ID_BYTES)
        check(lib().mpcb_comm_init_rank(self._h, C.cast(buf, C.c_void_p), int(rank), int(world)), self._h)

    def comm_info(self):
        w, r = C.c_int32(), C.c_int32()
        check(lib().mpcb_comm_info(self._h, C.byref(w), C.byref(r)), self._h)
        return w.value, r.value

    def allgather(self, d_send, d_recv, count):
        p = lambda v: v.ptr if isinstance(v, DeviceArray) else C.c_void_p(int(v))   # noqa: E731
        check(lib().mpcb_allgather(self._h, p(d_send), p(d_recv), int(count)), self._h)

    def allreduce(self, values, op="sum"):
        """In-place over the ranks on a small float64 array; also a barrier."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        check(lib().mpcb_allreduce(self._h, dptr(v), v.size, 0 if op == "sum" else 1), self._h)
        return v

    def gathered_z(self, index, B):
        """(device group) the [B, nz] trajectories of the last solve_batch as device `index` of the group holds them after the
        all-gather, downloaded for inspection."""
        p = C.c_void_p()
        check(lib().mpcb_gathered_z(self._h, int(index), C.byref(p)), self._h)
        G = self.comm_info()[0]
        longest = max(hi - lo for lo, hi in (shard_bounds(B, G, g) for g in range(G)))
        raw = np.empty((G * longest, self.nz))
        check(lib().mpcb_dev_download(self._h, raw.ctypes.data_as(C.c_void_p), p, raw.nbytes), self._h)
        return np.concatenate([raw[g * longest: g * longest + (hi - lo)] for g, (lo, hi) in enumerate(shard_bounds(B, G, g) for g in range(G))])

    def sync(self):
        check(lib().mpcb_sync(self._h), self._h)

    def wait_for(self, other):
        """This handle's stream waits (on the device) for everything queued so far on `other`'s stream."""
        check(lib().mpcb_stream_wait(self._h, other._h), self._h)

    def record(self, slot):
        """Mark "everything queued so far on this handle" in event slot `slot` (mpcb_event_record)."""
        check(lib().mpcb_event_record(self._h, int(slot)), self._h)

    def wait_mark(self, other, slot):
        """This handle's later work waits for `other`'s mark `slot` (mpcb_event_wait); no-op if never recorded."""
        check(lib().mpcb_event_wait(self._h, other._h, int(slot)), self._h)

    def timing(self, reset=False):
        n = C.c_int32(); tot = C.c_double(); last = C.c_double()
        check(lib().mpcb_timing(self._h, 1 if reset else 0, C.byref(n), C.byref(tot), C.byref(last)), self._h)
        return dict(launches=n.value, total_ms=tot.value, last_ms=last.value)
