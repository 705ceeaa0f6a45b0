"""Every float64 entry point refuses a batch whose workspace would pass the family's 24 GiB limit with JSTSP_E_UNSUPPORTED and
names the largest batch that fits (include/jstsp.h), before it allocates or copies anything; the context then still works.

The shapes are the largest each entry point admits at batch 65535: the need is hundreds of GiB to PiB, several times the card's
memory, so a refusal that did not fire would end in an allocation error code, never in a copy from the one-element arrays passed
here.  That the batch named in the message really fits is not tested - it would mean allocating 24 GiB on a shared card - and holds
by construction: the search and the allocation run the same layout function (csrc/ws64.h: ws64_open)."""
import ctypes as C
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HOST, DEVICE = 0, 1
BIG = 65535
ONES = np.ones(BIG)                                             # tau, rho: read on the host at full length


def _lib_ctx():
    from jstsp19_amd import _lib
    return _lib.load(), _lib.default_context(0)


def _p(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def _d(x):
    return x.ctypes.data_as(C.POINTER(C.c_double))


def _c(*shape, seed=0):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.standard_normal(shape) + 1j * rng.standard_normal(shape))


def _z(n, dtype=np.complex128):
    return np.zeros(n, dtype)


DUMMY = _z(1)                                                   # stands for every matrix of a refused call: never read or written


def _svt(lib, h, mem, big):
    if big:
        return lib.jstsp_svt_f64(h, 512, 512, BIG, _p(DUMMY), _d(ONES), _p(DUMMY), mem)
    Y, X = _c(1, 4, 3), _z(12)
    return lib.jstsp_svt_f64(h, 3, 4, 1, _p(Y), _d(ONES), _p(X), mem)


def _mc_svt(lib, h, mem, big):
    if big:
        return lib.jstsp_mc_svt_f64(h, 512, 512, BIG, _p(DUMMY), _p(DUMMY), 3, _d(ONES), _d(ONES), _p(DUMMY), mem)
    OH, Om, X = _c(1, 4, 3), np.ones(12), _z(12)
    return lib.jstsp_mc_svt_f64(h, 3, 4, 1, _p(OH), _p(Om), 2, _d(ONES), _d(ONES), _p(X), mem)


def _mc_admm(lib, h, mem, big):
    if big:
        return lib.jstsp_mc_admm_f64(h, 512, 512, BIG, _p(DUMMY), _p(DUMMY), _p(DUMMY), 3, _d(ONES), _d(ONES), _p(DUMMY), _p(DUMMY), mem)
    Ht, OH, Om, X, ce = _c(1, 4, 3), _c(1, 4, 3, seed=1), np.ones(12), _z(12), _z(2, np.float64)
    return lib.jstsp_mc_admm_f64(h, 3, 4, 1, _p(Ht), _p(OH), _p(Om), 2, _d(ONES), _d(ONES), _p(X), _p(ce), mem)


def _sparse_admm(lib, h, mem, big):
    if big:
        return lib.jstsp_sparse_admm_f64(h, 512, 512, 512, 512, BIG, _p(DUMMY), _p(DUMMY), _p(DUMMY), _p(DUMMY), 3, _p(DUMMY), _p(DUMMY), mem)
    Ht, OH, Dr, Dt, S, ce = _c(1, 4, 3), _c(1, 4, 3, seed=1), _c(3, 3, seed=2), _c(4, 4, seed=3), _z(12), _z(2, np.float64)
    return lib.jstsp_sparse_admm_f64(h, 3, 4, 3, 4, 1, _p(Ht), _p(OH), _p(Dr), _p(Dt), 2, _p(S), _p(ce), mem)


def _proposed(lib, h, mem, big):
    if big:
        return lib.jstsp_proposed_algorithm_f64(h, 512, 512, 512, 512, BIG, _p(DUMMY), _p(DUMMY), _p(DUMMY), 512 * 512, _p(DUMMY), 512 * 512, 3,
                                                _d(ONES), _d(ONES), _d(ONES), 0, None, _p(DUMMY), _p(DUMMY), _p(DUMMY), mem)
    N, M, Gr, G2 = 3, 4, 5, 6
    subY, Om, A, B = _c(1, M, N), np.ones(N * M), _c(Gr, N, seed=1), _c(M, G2, seed=2)
    S, Y, ce = _z(Gr * G2), _z(N * M), _z(3 * 2, np.float64)
    return lib.jstsp_proposed_algorithm_f64(h, N, M, Gr, G2, 1, _p(subY), _p(Om), _p(A), 0, _p(B), 0, 2, _d(ONES), _d(ONES), _d(ONES), 0, None,
                                            _p(S), _p(Y), _p(ce), mem)


def _pinv(lib, h, mem, big):
    if big:
        return lib.jstsp_pinv_f64(h, 512, 8192, BIG, _p(DUMMY), _p(DUMMY), None, None, mem)
    A, P, rc, rk = _c(1, 3, 5), _z(15), _z(1, np.float64), _z(1, np.int32)
    return lib.jstsp_pinv_f64(h, 5, 3, 1, _p(A), _p(P), _p(rc), _p(rk), mem)


def _ls(lib, h, mem, big):
    if big:                                                     # A 8192 x 512 and B 512 x 8192, one factor per trial
        return lib.jstsp_ls_f64(h, 8192, 8192, 512, 512, BIG, _p(DUMMY), _p(DUMMY), 8192 * 512, _p(DUMMY), 512 * 8192, _p(DUMMY), None, mem)
    N, M, Gr, G2 = 5, 6, 3, 4
    Y, A, B, S, rc = _c(1, M, N), _c(Gr, N, seed=1), _c(M, G2, seed=2), _z(Gr * G2), _z(2, np.float64)
    return lib.jstsp_ls_f64(h, N, M, Gr, G2, 1, _p(Y), _p(A), 0, _p(B), 0, _p(S), _p(rc), mem)


def _omp(lib, h, mem, big):
    if big:
        return lib.jstsp_omp_f64(h, 65536, 2048, BIG, _p(DUMMY), 0, _p(DUMMY), 1024, _p(DUMMY), _p(DUMMY), _p(DUMMY), mem)
    A, v, x, idx, tg = _c(9, 6), _c(1, 6, seed=1), _z(9), _z(3, np.int32), _z(18)
    return lib.jstsp_omp_f64(h, 6, 9, 1, _p(A), 0, _p(v), 3, _p(x), _p(idx), _p(tg), mem)


def _omp_kron(lib, h, mem, big):
    if big:
        return lib.jstsp_omp_kron_f64(h, 256, 256, 32, 32, BIG, _p(DUMMY), 0, _p(DUMMY), 0, _p(DUMMY), 1024, _p(DUMMY), _p(DUMMY), mem)
    Af, Bf, y, x, idx = _c(4, 3), _c(2, 5, seed=1), _c(1, 6, seed=2), _z(20), _z(3, np.int32)
    return lib.jstsp_omp_kron_f64(h, 3, 2, 4, 5, 1, _p(Af), 0, _p(Bf), 0, _p(y), 3, _p(x), _p(idx), mem)


ENTRIES = {"svt_f64": _svt, "mc_svt_f64": _mc_svt, "mc_admm_f64": _mc_admm, "sparse_admm_f64": _sparse_admm,
           "proposed_algorithm_f64": _proposed, "pinv_f64": _pinv, "ls_f64": _ls, "omp_f64": _omp, "omp_kron_f64": _omp_kron}


@pytest.mark.parametrize("memspace", [HOST, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_a_batch_past_the_limit_is_refused_with_the_batch_that_fits_and_the_context_goes_on(name, memspace):
    lib, ctx = _lib_ctx()
    rc = ENTRIES[name](lib, ctx.handle, memspace, True)
    msg = lib.jstsp_last_error().decode()
    assert rc == -3, (rc, msg)                                  # JSTSP_E_UNSUPPORTED
    m = re.search(r"largest batch that fits is about (\d+)", msg)
    assert m, msg
    assert 1 <= int(m.group(1)) < BIG, msg
    rc = ENTRIES[name](lib, ctx.handle, HOST, False)            # the same entry point, batch 1 on a tiny shape
    assert rc == 0, (rc, lib.jstsp_last_error().decode())
