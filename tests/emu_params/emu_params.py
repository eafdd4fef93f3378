"""ctypes front-end of tests/emu_params (CPU stepping of the PARAMS instantiations of the kernel source).  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

from mpc_motion_planning_amd._abi import MpcbConfig, dptr, iptr, OBSIN_STATIC, OBSIN_PREDICTED

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        _LIB = C.CDLL(os.path.join(_HERE, "_build", "libmpcbparams.so"))
        _LIB.mpcb_emu_params_solve.restype = C.c_int
    return _LIB


def solve(base, cfgs, x0, xs, obs=None, z0=None):
    """Instance b stepped under cfgs[b] (a ctypes array of MpcbConfig, e.g. from solver.vary, or a sequence of configs); `base` plays
    the handle's config.  -> dict(z, obj, status, iters, kkt, lam_g, lam_x)."""
    x0 = np.ascontiguousarray(np.atleast_2d(x0), dtype=np.float64)
    xs = np.ascontiguousarray(np.atleast_2d(xs), dtype=np.float64)
    B = x0.shape[0]; N = base.N; nx = base.nx()
    if not (isinstance(cfgs, C.Array) and cfgs._type_ is MpcbConfig):
        rows = list(cfgs)
        arr = (MpcbConfig * len(rows))()
        for b, r in enumerate(rows):
            C.memmove(C.byref(arr[b]), C.byref(r), C.sizeof(MpcbConfig))
        cfgs = arr
    assert len(cfgs) == B, "one config per instance"
    nz = 2 * N + nx * (N + 1)
    nrate = sum(1 for i in range(2) if np.isfinite(base.du_lo[i]) or np.isfinite(base.du_hi[i]))
    ng = nx * (N + 1) + nrate * (N - 1) + base.n_obs * (N + 1 if base.obs_terminal else N)
    kind = OBSIN_STATIC
    if base.n_obs > 0:
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if obs.size == B * base.n_obs * (N + 1) * 6:
            kind = OBSIN_PREDICTED
    else:
        obs = None
    if z0 is not None:
        z0 = np.ascontiguousarray(z0, dtype=np.float64).reshape(B, nz)
    z = np.zeros((B, nz)); obj = np.zeros(B); st = np.zeros(B, np.int32); it = np.zeros(B, np.int32)
    kkt = np.zeros((B, 4)); lam_g = np.zeros((B, ng)); lam_x = np.zeros((B, nz))
    rc = lib().mpcb_emu_params_solve(C.byref(base), cfgs, C.c_int32(B), dptr(x0), dptr(xs), dptr(obs), C.c_int32(kind), dptr(z0),
                                     dptr(z), dptr(obj), iptr(st), iptr(it), dptr(kkt), dptr(lam_g), dptr(lam_x))
    if rc != 0:
        raise RuntimeError("mpcb_emu_params_solve failed with code %d" % rc)
    return dict(z=z, obj=obj, status=st, iters=it, kkt=kkt, lam_g=lam_g, lam_x=lam_x)
