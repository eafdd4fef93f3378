"""ctypes front-end of tests/emu_eval (CPU stepping of mpcb_eval.h).  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

from mpc_motion_planning_amd import _abi
from mpc_motion_planning_amd._abi import MpcbConfig, dptr, OBSIN_STATIC, OBSIN_PREDICTED

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        _LIB = C.CDLL(os.path.join(_HERE, "_build", "libmpcbevalemu.so"))
        _LIB.mpcb_emu_evaluate.restype = C.c_int
    return _LIB


def dims(cfg):
    """nx, nz, ng of a config, as mpcb_dims counts them (a rate row per control with a finite du bound)."""
    N, nx = cfg.N, cfg.nx()
    nrate = sum(1 for i in range(2) if np.isfinite(cfg.du_lo[i]) or np.isfinite(cfg.du_hi[i]))
    return nx, 2 * N + nx * (N + 1), nx * (N + 1) + nrate * (N - 1) + cfg.n_obs * (N + 1 if cfg.obs_terminal else N)


def evaluate(cfg, x0, xs, obs, z, lam_g=None, lam_x=None, x_ref=None, cfgs=None, want_g=True, want_grad=False):
    """BatchSolver.evaluate stepped on the CPU: the same arguments behind a config, the same dict back.  cfgs: instance b under cfgs[b]."""
    x0 = np.ascontiguousarray(np.atleast_2d(x0), dtype=np.float64)
    xs = np.ascontiguousarray(np.atleast_2d(xs), dtype=np.float64)
    B = x0.shape[0]; N = cfg.N
    nx, nz, ng = dims(cfg)
    kind = OBSIN_STATIC
    if cfg.n_obs > 0:
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if obs.size == B * cfg.n_obs * (N + 1) * 6:
            kind = OBSIN_PREDICTED
        else:
            assert obs.size == B * cfg.n_obs * 6
    else:
        obs = None
    z = np.ascontiguousarray(np.asarray(z, dtype=np.float64).reshape(B, nz))
    if lam_g is not None:
        lam_g = np.ascontiguousarray(np.asarray(lam_g, dtype=np.float64).reshape(B, ng))
    if lam_x is not None:
        lam_x = np.ascontiguousarray(np.asarray(lam_x, dtype=np.float64).reshape(B, nz))
    if x_ref is not None:
        x_ref = np.ascontiguousarray(np.asarray(x_ref, dtype=np.float64).reshape(B, N, nx))
    if cfgs is not None and not (isinstance(cfgs, C.Array) and cfgs._type_ is MpcbConfig):
        rows = list(cfgs)
        cfgs = (MpcbConfig * len(rows))()
        for b, r in enumerate(rows):
            C.memmove(C.byref(cfgs[b]), C.byref(r), C.sizeof(MpcbConfig))
    assert cfgs is None or len(cfgs) == B, "one config per instance"
    obj = np.full(B, np.nan); res = np.full((B, _abi.EVAL_COLS), np.nan)
    g = np.full((B, ng), np.nan) if want_g else None
    grad = np.full((B, nz), np.nan) if want_grad else None
    rc = lib().mpcb_emu_evaluate(C.byref(cfg), C.c_int32(B), cfgs, C.c_int32(nz), C.c_int32(ng), dptr(x0), dptr(xs), dptr(x_ref), dptr(obs),
                                 C.c_int32(kind), dptr(z), dptr(lam_g), dptr(lam_x), dptr(obj), dptr(g), dptr(grad), dptr(res))
    if rc != 0:
        raise RuntimeError("mpcb_emu_evaluate failed with code %d" % rc)
    out = dict(obj=obj, g=g, grad_lag=grad)
    out.update({name: res[:, i].copy() for i, name in enumerate(_abi.EVAL_NAMES)})
    return out
