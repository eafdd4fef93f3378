"""ctypes front-end of tests/emu_multi (CPU stepping of mpcb_multi.h).  Test infrastructure only.

Every output array is allocated with a tail of GUARD sentinel words behind it, which the stepped kernels must leave alone."""
import ctypes as C
import os
import subprocess

import numpy as np

from mpc_motion_planning_amd._abi import dptr, iptr

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
GUARD = 64


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        _LIB = C.CDLL(os.path.join(_HERE, "_build", "libmpcbmultiemu.so"))
        _LIB.mpcb_emu_multi_expand.restype = C.c_int
        _LIB.mpcb_emu_multi_select.restype = C.c_int
    return _LIB


class _Guarded:
    """A flat output buffer of `shape` followed by GUARD words of a sentinel."""

    def __init__(self, shape, dtype):
        self.shape, self.n = shape, int(np.prod(shape))
        self.sentinel = np.nan if dtype == np.float64 else -123456
        self.buf = np.full(self.n + GUARD, self.sentinel, dtype=dtype)

    def ptr(self):
        return dptr(self.buf) if self.buf.dtype == np.float64 else iptr(self.buf)

    def take(self, what):
        tail = self.buf[self.n:]
        clean = np.isnan(tail).all() if self.buf.dtype == np.float64 else (tail == self.sentinel).all()
        assert clean, "%s: the kernel wrote behind its output" % what
        return self.buf[:self.n].reshape(self.shape).copy()


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def expand(N, nx, x0, xs, obs, controls, z0=None):
    """mpcb_multi_expand stepped on the CPU.  x0, xs [B,nx]; obs [B, ...] | None (any row length); controls [K,2] | None (K = 1 with z0);
    z0 [B,nz] | None.  Returns (x0_e [B*K,nx], xs_e [B*K,nx], obs_e [B*K, row] | None, z0_e [B*K,nz])."""
    x0 = _c(x0); xs = _c(xs); z0 = _c(z0); controls = _c(controls)
    B = x0.shape[0]; K = 1 if controls is None else controls.shape[0]
    nz = 2 * N + nx * (N + 1)
    obs_row = 0
    if obs is not None:
        obs = _c(obs).reshape(B, -1); obs_row = obs.shape[1]
    E = B * K
    o_x0 = _Guarded((E, nx), np.float64); o_xs = _Guarded((E, nx), np.float64); o_z0 = _Guarded((E, nz), np.float64)
    o_obs = _Guarded((E, obs_row), np.float64) if obs_row else None
    rc = lib().mpcb_emu_multi_expand(C.c_int32(B), C.c_int32(K), C.c_int32(N), C.c_int32(nx), C.c_int32(nz), C.c_int32(obs_row), dptr(x0), dptr(xs),
                                     dptr(obs), dptr(z0), dptr(controls), o_x0.ptr(), o_xs.ptr(), o_obs.ptr() if o_obs else None, o_z0.ptr())
    if rc != 0:
        raise RuntimeError("mpcb_emu_multi_expand failed with code %d" % rc)
    return o_x0.take("x0_e"), o_xs.take("xs_e"), (o_obs.take("obs_e") if o_obs else None), o_z0.take("z0_e")


def select(z_all, obj_all, status_all, iters_all=None, kkt_all=None, lam_g_all=None, lam_x_all=None, obj_margin=1e-9, basin_tol=1e-4):
    """mpcb_multi_select stepped on the CPU over [B,K,...] tables.  Returns dict(z, obj, status, which, n_ok, n_basins[, iters, kkt, lam_g,
    lam_x]): the optional outputs where their table is given."""
    z_all = _c(z_all); obj_all = _c(obj_all)
    B, K, nz = z_all.shape
    status_all = np.ascontiguousarray(status_all, dtype=np.int32).reshape(B, K)
    iters_all = None if iters_all is None else np.ascontiguousarray(iters_all, dtype=np.int32).reshape(B, K)
    kkt_all = _c(kkt_all); lam_g_all = _c(lam_g_all); lam_x_all = _c(lam_x_all)
    ng = 0 if lam_g_all is None else lam_g_all.shape[2]
    out = dict(z=_Guarded((B, nz), np.float64), obj=_Guarded((B,), np.float64), status=_Guarded((B,), np.int32),
               which=_Guarded((B,), np.int32), n_ok=_Guarded((B,), np.int32), n_basins=_Guarded((B,), np.int32),
               iters=_Guarded((B,), np.int32) if iters_all is not None else None,
               kkt=_Guarded((B, 4), np.float64) if kkt_all is not None else None,
               lam_g=_Guarded((B, ng), np.float64) if lam_g_all is not None else None,
               lam_x=_Guarded((B, nz), np.float64) if lam_x_all is not None else None)
    p = lambda k: out[k].ptr() if out[k] is not None else None      # noqa: E731
    rc = lib().mpcb_emu_multi_select(C.c_int32(B), C.c_int32(K), C.c_int32(nz), C.c_int32(ng), C.c_double(obj_margin), C.c_double(basin_tol),
                                     dptr(z_all), dptr(obj_all), dptr(kkt_all), dptr(lam_g_all), dptr(lam_x_all), iptr(status_all), iptr(iters_all),
                                     p("z"), p("obj"), p("kkt"), p("lam_g"), p("lam_x"), p("status"), p("iters"), p("which"), p("n_ok"),
                                     p("n_basins"))
    if rc != 0:
        raise RuntimeError("mpcb_emu_multi_select failed with code %d" % rc)
    return {k: v.take(k) for k, v in out.items() if v is not None}
