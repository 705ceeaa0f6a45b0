"""ctypes calls of the C ABI with numpy arrays (tests/test_gpu_c64.py, tests/test_gpu_std_parity.py): column-major staging of
(batch, R, C) arrays and proposed_algorithm through its _c32 / _c64 entry points in host memory."""
import ctypes as C

import numpy as np

from jstsp19_amd import _lib

HOST = 0


def _f(a):                       # column-major bytes of a (batch, R, C) / (R, C) array: trial index slowest
    a = np.asarray(a)
    if a.ndim == 3:
        return np.ascontiguousarray(np.transpose(a, (0, 2, 1)))
    return np.ascontiguousarray(a.T)


def _unf(buf, shape):            # inverse of _f
    if len(shape) == 3:
        b, R, Cc = shape
        return np.transpose(buf.reshape(b, Cc, R), (0, 2, 1))
    R, Cc = shape
    return buf.reshape(Cc, R).T


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _proposed(lib, ctx, suffix, A, B, Om, subY, Imax, tY, tS, rho, type_, indx=None, want_ce=True):
    batch, N, M = subY.shape
    Gr, G2 = A.shape[1], B.shape[1]
    cdt, rdt = (np.complex128, np.float64) if suffix == "c64" else (np.complex64, np.float32)
    a, b, om, sy = _f(A.astype(cdt)), _f(B.astype(cdt)), _f(Om.astype(rdt)), _f(subY.astype(cdt))
    S = np.empty(batch * Gr * G2, cdt)
    Y = np.empty(batch * N * M, cdt)
    ce = np.empty(batch * 3 * Imax, np.float64) if want_ce else None
    ty, ts, rh = (np.full(batch, v, np.float64) for v in (tY, tS, rho))
    ix = np.ascontiguousarray(indx, np.int32) if indx is not None else None
    fn = getattr(lib, "jstsp_proposed_algorithm_" + suffix)
    _lib.check(fn(ctx.handle, N, M, Gr, G2, batch, _p(sy), _p(om), _p(a), 0, _p(b), G2 * M, Imax, _dp(ty), _dp(ts), _dp(rh),
                  type_, _p(ix), _p(S), _p(Y), _p(ce), HOST), "proposed_" + suffix)
    return (_unf(S, (batch, Gr, G2)), _unf(Y, (batch, N, M)),
            np.transpose(ce.reshape(batch, 3, Imax), (0, 2, 1)) if want_ce else None)
