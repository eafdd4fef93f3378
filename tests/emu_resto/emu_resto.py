"""ctypes front-end of tests/emu_resto (CPU stepping of the restoration phase inside the lean launch).  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

from mpc_motion_planning_amd._abi import dptr, iptr, OBSIN_STATIC, OBSIN_PREDICTED
from tests.emu.emu import _rows

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        _LIB = C.CDLL(os.path.join(_HERE, "_build", "libmpcbemuresto.so"))
        _LIB.mpcb_emu_resto_solve.restype = C.c_int
        _LIB.mpcb_emu_resto_dispatch.restype = C.c_int
    return _LIB


def solve(cfg, x0, xs, obs=None, z0=None, x_ref=None, cfgs=None, resto_in_launch=None):
    """tests.emu.emu.solve with the wrapper of the kernels that restore in place -> dict(z, obj, status, iters, kkt, lam_g, lam_x).
    resto_in_launch: the restoration phase inside the lean launch, None by the rule of mpcb_dispatch.h, False never, True wherever the
    instantiation has it and a restoration pass follows (the rule without its LDS condition)."""
    x0 = np.ascontiguousarray(np.atleast_2d(x0), dtype=np.float64)
    xs = np.ascontiguousarray(np.atleast_2d(xs), dtype=np.float64)
    B = x0.shape[0]; N = cfg.N; nx = cfg.nx()
    nz = 2 * N + nx * (N + 1)
    nrate = sum(1 for i in range(2) if np.isfinite(cfg.du_lo[i]) or np.isfinite(cfg.du_hi[i]))
    ng = nx * (N + 1) + nrate * (N - 1) + cfg.n_obs * (N + 1 if cfg.obs_terminal else N)
    kind = OBSIN_STATIC
    if cfg.n_obs > 0:
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if obs.size == B * cfg.n_obs * (N + 1) * 6:
            kind = OBSIN_PREDICTED
    else:
        obs = None
    if z0 is not None:
        z0 = np.ascontiguousarray(z0, dtype=np.float64).reshape(B, nz)
    if x_ref is not None:
        x_ref = np.ascontiguousarray(np.asarray(x_ref, dtype=np.float64).reshape(B, N, 4))
    cfgs = _rows(cfgs)
    assert cfgs is None or len(cfgs) == B, "one config per instance"
    z = np.zeros((B, nz)); obj = np.zeros(B); st = np.zeros(B, np.int32); it = np.zeros(B, np.int32)
    kkt = np.zeros((B, 4)); lam_g = np.zeros((B, ng)); lam_x = np.zeros((B, nz))
    rc = lib().mpcb_emu_resto_solve(C.byref(cfg), C.c_int32(B), dptr(x0), dptr(xs), dptr(obs), C.c_int32(kind), dptr(z0),
                                    dptr(z), dptr(obj), iptr(st), iptr(it), dptr(kkt), dptr(lam_g), dptr(lam_x), dptr(x_ref), cfgs,
                                    C.c_int32(-1 if resto_in_launch is None else int(bool(resto_in_launch))))
    if rc != 0:
        raise RuntimeError("mpcb_emu_resto_solve failed with code %d" % rc)
    return dict(z=z, obj=obj, status=st, iters=it, kkt=kkt, lam_g=lam_g, lam_x=lam_x)


def dispatch(cfg, track=False, params=False, start_given=False, fused=None):
    """The rule for the first launch of one solve: dict(code) when no kernel is shipped for it, else dict(code=0, resto_in_launch, lds_first,
    passes): whether that launch runs the restoration phase of its instances itself, the LDS bytes it gets, and pass_plan's passes."""
    out = (C.c_int64 * 8)()
    rc = lib().mpcb_emu_resto_dispatch(C.byref(cfg), C.c_int32(track), C.c_int32(params), C.c_int32(start_given),
                                       C.c_int32(-1 if fused is None else int(fused)), out)
    if rc != 0:
        return dict(code=rc)
    o = list(out)
    return dict(code=0, resto_in_launch=bool(o[0]), lds_first=o[1], passes=o[3:3 + o[2]])
