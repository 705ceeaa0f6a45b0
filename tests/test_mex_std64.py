"""The MEX command 'proposed_algorithm_std_f64' (mex/jstsp_mex.cpp) without a GPU: the gateway compiles with -Wall -Wextra
-Werror against the stand-in MEX API (tests/mex_stub/), and the command hands the reference's argument list, the optional
indx_S / PA / PB ([] = not given), the strides and the optional outputs to jstsp_proposed_std_f64 unchanged.  The library side
is a recording stand-in for that entry (and for context creation), linked in front of the real library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_mex_gateway import MexError, call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RECORDER = r"""
#include <cstdint>
#include <cstring>
#include "jstsp.h"
struct Rec { int dims[6], memspace, has_PA, has_PB, has_idx, has_Y, has_ce, has_rc, idx0; long long sA, sB; double tY1, tS1, rho1, sum_PA, sum_PB; };
static Rec g_rec;
static int g_ctx_store;
extern "C" {
int jstsp_create(int, jstsp_ctx **out) { *out = reinterpret_cast<jstsp_ctx *>(&g_ctx_store); return 0; }
int jstsp_destroy(jstsp_ctx *) { return 0; }
const char *jstsp_last_error(void) { return "recorder"; }
int jstsp_proposed_std_f64(jstsp_ctx *, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *, const double *, const jstsp_c64 *, long long sA,
                           const jstsp_c64 *, long long sB, const jstsp_c64 *PA, const jstsp_c64 *PB, int Imax, const double *tY, const double *tS,
                           const double *rho, const int32_t *idx, jstsp_c64 *S, jstsp_c64 *Y, double *ce, double *rc, int memspace)
{
    std::memset(&g_rec, 0, sizeof(g_rec));
    const int d[6] = {N, M, Gr, G2, batch, Imax};
    std::memcpy(g_rec.dims, d, sizeof(d));
    g_rec.sA = sA; g_rec.sB = sB; g_rec.memspace = memspace;
    g_rec.has_PA = PA != nullptr; g_rec.has_PB = PB != nullptr; g_rec.has_idx = idx != nullptr;
    g_rec.has_Y = Y != nullptr; g_rec.has_ce = ce != nullptr; g_rec.has_rc = rc != nullptr;
    g_rec.idx0 = idx ? idx[0] : 0;
    g_rec.tY1 = tY[batch - 1]; g_rec.tS1 = tS[batch - 1]; g_rec.rho1 = rho[batch - 1];
    if (PA) for (long long i = 0; i < (long long)Gr * N * (sA ? batch : 1); ++i) g_rec.sum_PA += PA[i].re;
    if (PB) for (long long i = 0; i < (long long)M * G2 * (sB ? batch : 1); ++i) g_rec.sum_PB += PB[i].im;
    for (long long i = 0; i < (long long)Gr * G2 * batch; ++i) S[i] = jstsp_c64{(double)i, -(double)i};
    if (Y) for (long long i = 0; i < (long long)N * M * batch; ++i) Y[i] = jstsp_c64{1.0, 2.0};
    if (ce) for (long long i = 0; i < 3ll * Imax * batch; ++i) ce[i] = (double)i;
    if (rc) { rc[0] = 0.25; rc[1] = 0.125; }
    return N == 3 ? JSTSP_E_ILLCOND : 0;
}
const Rec *recorder_last(void) { return &g_rec; }
}
"""


class Rec(C.Structure):
    _fields_ = [("dims", C.c_int * 6)] + [(n, C.c_int) for n in ("memspace", "has_PA", "has_PB", "has_idx", "has_Y", "has_ce", "has_rc", "idx0")] + \
               [("sA", C.c_longlong), ("sB", C.c_longlong)] + [(n, C.c_double) for n in ("tY1", "tS1", "rho1", "sum_PA", "sum_PB")]


@pytest.fixture(scope="module")
def mex(tmp_path_factory):
    from jstsp19_amd import build as B
    lib = B.build()
    d = tmp_path_factory.mktemp("mexstd64")
    src, rec, out = str(d / "recorder.cpp"), str(d / "libjstsp_recorder_std64.so"), str(d / "jstsp_mex_stub_std64.so")
    open(src, "w").write(RECORDER)
    r = subprocess.run(["g++", "-O1", "-Wall", "-Wextra", "-Werror", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), src, "-o", rec],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cmd = ["g++", "-O1", "-Wall", "-Wextra", "-Werror", "-std=c++17", "-shared", "-fPIC", "-DMATLAB_MEX_FILE",
           "-I" + os.path.join(ROOT, "tests", "mex_stub"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "mex", "jstsp_mex.cpp"), os.path.join(ROOT, "tests", "mex_stub", "stub.cpp"), "-o", out,
           "-Wl,--no-as-needed", "-L" + str(d), "-ljstsp_recorder_std64", "-L" + os.path.dirname(lib), "-ljstsp_mi355x",
           "-Wl,-rpath," + str(d), "-Wl,-rpath," + os.path.dirname(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy first, as jstsp19_amd._lib does)
    m = C.CDLL(out)
    vp = C.c_void_p
    m.mxCreateNumericArray.restype = vp
    m.mxCreateNumericArray.argtypes = [C.c_size_t, C.POINTER(C.c_size_t), C.c_int, C.c_int]
    m.mxCreateString.restype = vp
    m.mxCreateString.argtypes = [C.c_char_p]
    m.mxCreateDoubleScalar.restype = vp
    m.mxCreateDoubleScalar.argtypes = [C.c_double]
    m.mxGetData.restype = vp
    m.mxGetData.argtypes = [vp]
    m.mxGetCell.restype = vp
    m.mxGetCell.argtypes = [vp, C.c_size_t]
    m.mxGetNumberOfDimensions.restype = C.c_size_t
    m.mxGetNumberOfDimensions.argtypes = [vp]
    m.mxGetDimensions.restype = C.POINTER(C.c_size_t)
    m.mxGetDimensions.argtypes = [vp]
    m.mxIsComplex.argtypes = [vp]
    m.mxGetClassID.argtypes = [vp]
    m.stub_call.argtypes = [C.c_int, C.POINTER(vp), C.c_int, C.POINTER(vp)]
    m.stub_error_id.restype = C.c_char_p
    m.stub_error_message.restype = C.c_char_p
    r = C.CDLL(rec)
    r.recorder_last.restype = C.POINTER(Rec)
    m.last = lambda: r.recorder_last().contents
    yield m
    m.stub_run_at_exit()


def _c(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def _problem(rng, batch=3):
    N, M, Gr, G2 = 6, 9, 4, 5
    return _c(rng, N, M, batch), np.ones((N, M, batch)), _c(rng, N, Gr), _c(rng, G2, M, batch)      # shared A, per-page B


def test_the_reference_argument_list_and_the_optional_outputs_pass_through(mex):
    rng = np.random.default_rng(3)
    subY, Om, A, B = _problem(rng)
    tY = np.array([0.1, 0.2, 0.3])
    S, = call(mex, 1, "proposed_algorithm_std_f64", subY, Om, A, B, 7, tY, 0.5, 0.25, "std")
    rec = mex.last()
    assert list(rec.dims) == [6, 9, 4, 5, 3, 7] and (rec.sA, rec.sB, rec.memspace) == (0, 45, 0)
    assert (rec.has_PA, rec.has_PB, rec.has_idx, rec.has_Y, rec.has_ce, rec.has_rc) == (0, 0, 0, 0, 0, 0)
    assert (rec.tY1, rec.tS1, rec.rho1) == (0.3, 0.5, 0.25)
    k = np.arange(60, dtype=np.float64)
    assert S.shape == (4, 5, 3) and np.array_equal(S.reshape(-1, order="F"), k - 1j * k)
    S, Y, ce, rc = call(mex, 4, "proposed_algorithm_std_f64", subY, Om, A, B, 7, tY, 0.5, 0.25, "std")
    rec = mex.last()
    assert (rec.has_Y, rec.has_ce, rec.has_rc) == (1, 1, 1)
    assert Y.shape == (6, 9, 3) and np.all(Y == 1 + 2j) and ce.shape == (7, 3, 3) and np.array_equal(ce.reshape(-1, order="F"), np.arange(63.0))
    assert rc.shape == (1, 2) and np.array_equal(rc[0], [0.25, 0.125])


def test_indx_S_and_the_factors_are_optional_and_may_be_empty(mex):
    rng = np.random.default_rng(4)
    subY, Om, A, B = _problem(rng)
    idx = np.stack([rng.permutation(20) + 1 for _ in range(3)], axis=1).astype(float)            # Gr G2 x pages
    PA, PB = _c(rng, 4, 6), _c(rng, 9, 5, 3)
    call(mex, 1, "proposed_algorithm_std_f64", subY, Om, A, B, 2, 0.1, 0.5, 0.25, "std", idx)
    rec = mex.last()
    assert (rec.has_idx, rec.idx0, rec.has_PA, rec.has_PB) == (1, int(idx[0, 0]), 0, 0)
    call(mex, 1, "proposed_algorithm_std_f64", subY, Om, A, B, 2, 0.1, 0.5, 0.25, "std", np.zeros((0, 0)), PA, PB)
    rec = mex.last()
    assert (rec.has_idx, rec.has_PA, rec.has_PB) == (0, 1, 1)
    assert abs(rec.sum_PA - PA.real.sum()) < 1e-12 and abs(rec.sum_PB - PB.imag.sum()) < 1e-12
    call(mex, 1, "proposed_algorithm_std_f64", subY, Om, A, B, 2, 0.1, 0.5, 0.25, "std", idx, np.zeros((0, 0)), PB)
    rec = mex.last()
    assert (rec.has_idx, rec.has_PA, rec.has_PB) == (1, 0, 1)


def test_bad_calls_are_refused_before_the_library_and_a_library_error_is_reported(mex):
    rng = np.random.default_rng(5)
    subY, Om, A, B = _problem(rng)
    good = (subY, Om, A, B, 2, 0.1, 0.5, 0.25, "std")
    PA, PB = _c(rng, 4, 6), _c(rng, 9, 5, 3)
    e0 = np.zeros((0, 0))
    for args, nlhs, ident in ((good[:8], 1, "jstsp:args"), (good, 5, "jstsp:args"), (good + (e0, PA, PB, PB), 1, "jstsp:args"),
                              (good[:8] + ("approximate",), 1, "jstsp:args"), (good[:4] + (0,) + good[5:], 1, "jstsp:args"),
                              ((subY, Om, A[:-1], B) + good[4:], 1, "jstsp:shape"), ((subY, Om[:, :-1], A, B) + good[4:], 1, "jstsp:shape"),
                              (good + (np.arange(1.0, 20.0),), 1, "jstsp:shape"),                 # numel(indx_S) != Gr G2 per page
                              (good + (e0, PA.T, PB), 1, "jstsp:shape"), (good + (e0, PA, PB[:, :, 0]), 1, "jstsp:shape"),
                              (good + (e0, np.stack([PA] * 3, axis=2), PB), 1, "jstsp:shape")):  # PA paged, A shared
        with pytest.raises(MexError) as e:
            call(mex, nlhs, "proposed_algorithm_std_f64", *args)
        assert e.value.ident == ident, str(e.value)
    with pytest.raises(MexError) as e:                                     # the recorder refuses N = 3 with JSTSP_E_ILLCOND
        call(mex, 1, "proposed_algorithm_std_f64", subY[:3], Om[:3], A[:3], B, 2, 0.1, 0.5, 0.25, "std")
    assert e.value.ident == "jstsp:call" and "jstsp_proposed_std_f64" in str(e.value) and "(-6)" in str(e.value)
    assert "'proposed_algorithm_std_f64'" in open(os.path.join(ROOT, "mex", "proposed_algorithm_std_f64.m")).read()
