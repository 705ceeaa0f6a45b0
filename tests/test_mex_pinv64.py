"""The MEX commands 'pinv_f64' and 'ls_f64' (mex/jstsp_mex.cpp) without a GPU: the gateway compiles with -Wall -Wextra -Werror
against the stand-in MEX API (tests/mex_stub/), and the two commands hand their arguments, the batch dimension and the optional
outputs to the library unchanged.  The library side is a recording stand-in for the two entries (and for context creation),
linked in front of the real library, which still resolves every other symbol of the gateway."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import check_below
from test_mex_gateway import MexError, call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RECORDER = r"""
#include <cstdint>
#include <cstring>
#include "jstsp.h"
struct Rec { int which, dims[6], memspace, has_rc, has_rk; long long sA, sB; double sum_re, sum_im; };
static Rec g_rec;
static int g_ctx_store;
static double sum_of(const jstsp_c64 *p, long long n, double *im) { double r = 0; *im = 0; for (long long i = 0; i < n; ++i) { r += p[i].re; *im += p[i].im; } return r; }
extern "C" {
int jstsp_create(int, jstsp_ctx **out) { *out = reinterpret_cast<jstsp_ctx *>(&g_ctx_store); return 0; }
int jstsp_destroy(jstsp_ctx *) { return 0; }
const char *jstsp_last_error(void) { return "recorder"; }
int jstsp_pinv_f64(jstsp_ctx *, int rows, int cols, int batch, const jstsp_c64 *A, jstsp_c64 *P, double *rc, int32_t *rk, int memspace)
{
    std::memset(&g_rec, 0, sizeof(g_rec));
    g_rec.which = 1; g_rec.dims[0] = rows; g_rec.dims[1] = cols; g_rec.dims[2] = batch; g_rec.memspace = memspace;
    g_rec.has_rc = rc != nullptr; g_rec.has_rk = rk != nullptr;
    g_rec.sum_re = sum_of(A, (long long)rows * cols * batch, &g_rec.sum_im);
    for (int t = 0; t < batch; ++t)                     /* P(c, r, t) = conj(A(r, c, t)): shows the layout arrives as it is */
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) {
                const jstsp_c64 a = A[((long long)t * cols + c) * rows + r];
                P[((long long)t * rows + r) * cols + c] = jstsp_c64{a.re, -a.im};
            }
    for (int t = 0; t < batch; ++t) { if (rc) rc[t] = 0.5 + t; if (rk) rk[t] = 7 + t; }
    return rows == 3 ? JSTSP_E_UNSUPPORTED : 0;
}
int jstsp_ls_f64(jstsp_ctx *, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *Y, const jstsp_c64 *, long long sA, const jstsp_c64 *,
                 long long sB, jstsp_c64 *S, double *rc, int memspace)
{
    std::memset(&g_rec, 0, sizeof(g_rec));
    g_rec.which = 2; g_rec.dims[0] = N; g_rec.dims[1] = M; g_rec.dims[2] = Gr; g_rec.dims[3] = G2; g_rec.dims[4] = batch;
    g_rec.sA = sA; g_rec.sB = sB; g_rec.memspace = memspace; g_rec.has_rc = rc != nullptr;
    g_rec.sum_re = sum_of(Y, (long long)N * M * batch, &g_rec.sum_im);
    for (long long i = 0; i < (long long)Gr * G2 * batch; ++i) S[i] = jstsp_c64{(double)i, -(double)i};
    if (rc) { rc[0] = 0.25; rc[1] = 0.125; }
    return 0;
}
const Rec *recorder_last(void) { return &g_rec; }
}
"""


class Rec(C.Structure):
    _fields_ = [("which", C.c_int), ("dims", C.c_int * 6), ("memspace", C.c_int), ("has_rc", C.c_int), ("has_rk", C.c_int),
                ("sA", C.c_longlong), ("sB", C.c_longlong), ("sum_re", C.c_double), ("sum_im", C.c_double)]


@pytest.fixture(scope="module")
def mex(tmp_path_factory):
    from jstsp19_amd import build as B
    lib = B.build()
    d = tmp_path_factory.mktemp("mexpinv64")
    src, rec, out = str(d / "recorder.cpp"), str(d / "libjstsp_recorder.so"), str(d / "jstsp_mex_stub.so")
    open(src, "w").write(RECORDER)
    r = subprocess.run(["g++", "-O1", "-Wall", "-Wextra", "-Werror", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), src, "-o", rec],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cmd = ["g++", "-O1", "-Wall", "-Wextra", "-Werror", "-std=c++17", "-shared", "-fPIC", "-DMATLAB_MEX_FILE",
           "-I" + os.path.join(ROOT, "tests", "mex_stub"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "mex", "jstsp_mex.cpp"), os.path.join(ROOT, "tests", "mex_stub", "stub.cpp"), "-o", out,
           "-Wl,--no-as-needed", "-L" + str(d), "-ljstsp_recorder", "-L" + os.path.dirname(lib), "-ljstsp_mi355x",
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


def test_pinv_f64_passes_shape_batch_and_optional_outputs_through(mex):
    rng = np.random.default_rng(3)
    A = _c(rng, 6, 4, 5)                                                   # rows x cols x pages
    P, = call(mex, 1, "pinv_f64", A)
    rec = mex.last()
    assert (rec.which, list(rec.dims[:3]), rec.memspace, rec.has_rc, rec.has_rk) == (1, [6, 4, 5], 0, 0, 0)
    check_below("mex_pinv64/input_sum", abs(rec.sum_re - A.real.sum()) + abs(rec.sum_im - A.imag.sum()), 1e-12)
    assert P.shape == (4, 6, 5)
    check_below("mex_pinv64/output_mismatch", np.abs(P - np.conj(np.swapaxes(A, 0, 1))).max(), 1e-300)
    P, rc, rk = call(mex, 3, "pinv_f64", A)
    rec = mex.last()
    assert (rec.has_rc, rec.has_rk) == (1, 1)
    assert rc.shape == (5, 1) and rk.shape == (5, 1) and rk.dtype == np.int32
    assert np.array_equal(rc[:, 0], 0.5 + np.arange(5)) and np.array_equal(rk[:, 0], 7 + np.arange(5))
    P, rc = call(mex, 2, "pinv_f64", A[:, :, 0])                           # 2-D: batch 1; a real matrix is widened
    rec = mex.last()
    assert (list(rec.dims[:3]), rec.has_rc, rec.has_rk) == ([6, 4, 1], 1, 0) and P.shape == (4, 6)
    call(mex, 1, "pinv_f64", A[:, :, 0].real)
    check_below("mex_pinv64/input_sum", abs(mex.last().sum_re - A[:, :, 0].real.sum()) + abs(mex.last().sum_im), 1e-12)


def test_ls_f64_passes_strides_batch_and_rcond_through(mex):
    rng = np.random.default_rng(4)
    Y, A, B = _c(rng, 6, 9, 3), _c(rng, 6, 4), _c(rng, 5, 9, 3)            # shared A, per-page B
    S, = call(mex, 1, "ls_f64", Y, A, B)
    rec = mex.last()
    assert (rec.which, list(rec.dims[:5]), rec.sA, rec.sB, rec.memspace, rec.has_rc) == (2, [6, 9, 4, 5, 3], 0, 45, 0, 0)
    check_below("mex_pinv64/input_sum", abs(rec.sum_re - Y.real.sum()) + abs(rec.sum_im - Y.imag.sum()), 1e-12)
    assert S.shape == (4, 5, 3)
    k = np.arange(60, dtype=np.float64)
    check_below("mex_pinv64/output_mismatch", np.abs(S.reshape(-1, order="F") - (k - 1j * k)).max(), 1e-300)
    S, rc = call(mex, 2, "ls_f64", Y, np.stack([A] * 3, axis=2), B[:, :, 0])
    rec = mex.last()
    assert (rec.sA, rec.sB, rec.has_rc) == (24, 0, 1) and np.array_equal(rc[:, 0], [0.25, 0.125])


def test_bad_calls_are_refused_before_the_library_and_a_library_error_is_reported(mex):
    rng = np.random.default_rng(5)
    Y, A, B = _c(rng, 6, 9), _c(rng, 6, 4), _c(rng, 5, 9)
    for args, nlhs, ident in ((("pinv_f64",), 1, "jstsp:args"), (("pinv_f64", A, A), 1, "jstsp:args"), (("pinv_f64", A), 4, "jstsp:args"),
                              (("ls_f64", Y, A), 1, "jstsp:args"), (("ls_f64", Y, A, B), 3, "jstsp:args"),
                              (("ls_f64", Y, A[:-1], B), 1, "jstsp:shape"), (("ls_f64", Y, A, B[:, :-1]), 1, "jstsp:shape"),
                              (("ls_f64", np.stack([Y] * 2, axis=2), np.stack([A] * 3, axis=2), B), 1, "jstsp:shape")):
        with pytest.raises(MexError) as e:
            call(mex, nlhs, *args)
        assert e.value.ident == ident, (args[0], str(e.value))
    with pytest.raises(MexError) as e:                                     # the recorder refuses 3 rows with JSTSP_E_UNSUPPORTED
        call(mex, 1, "pinv_f64", _c(rng, 3, 2))
    assert e.value.ident == "jstsp:call" and "jstsp_pinv_f64" in str(e.value) and "(-3)" in str(e.value)
    for f, cmd in (("pinv_f64.m", "'pinv_f64'"), ("ls_estimate_f64.m", "'ls_f64'")):
        assert cmd in open(os.path.join(ROOT, "mex", f)).read()
