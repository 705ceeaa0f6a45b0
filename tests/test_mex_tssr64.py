"""The MEX commands 'mmv_omp_f64', 'mc_svt_f64' and 'mc_admm_f64' (mex/jstsp_mex.cpp) without a GPU: the gateway compiles with
-Wall -Wextra -Werror against the stand-in MEX API (tests/mex_stub/), and the three commands hand shapes, the batch dimension,
strides, pnorm, K, Imax, the per-page scalars and the NULL-able outputs to the library unchanged.  The library side is a
recording stand-in for the three entries (and for context creation), linked in front of the real library, which still resolves
every other symbol of the gateway."""
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
struct Rec { int which, dims[6], memspace, has_a, has_b; long long sA, sB; double sum_re, sum_im; };
static Rec g_rec;
static int g_ctx_store;
static double sum_of(const jstsp_c64 *p, long long n, double *im) { double r = 0; *im = 0; for (long long i = 0; i < n; ++i) { r += p[i].re; *im += p[i].im; } return r; }
extern "C" {
int jstsp_create(int, jstsp_ctx **out) { *out = reinterpret_cast<jstsp_ctx *>(&g_ctx_store); return 0; }
int jstsp_destroy(jstsp_ctx *) { return 0; }
const char *jstsp_last_error(void) { return "recorder"; }
int jstsp_mmv_omp_f64(jstsp_ctx *, int N, int Gr, int S, int batch, const jstsp_c64 *, long long sA, const jstsp_c64 *Y, int K, int pnorm,
                      jstsp_c64 *Z, int32_t *idx, int32_t *cnt, int memspace)
{
    std::memset(&g_rec, 0, sizeof(g_rec));
    g_rec.which = 1; g_rec.dims[0] = N; g_rec.dims[1] = Gr; g_rec.dims[2] = S; g_rec.dims[3] = batch; g_rec.dims[4] = K; g_rec.dims[5] = pnorm;
    g_rec.sA = sA; g_rec.memspace = memspace; g_rec.has_a = idx != nullptr; g_rec.has_b = cnt != nullptr;
    g_rec.sum_re = sum_of(Y, (long long)N * S * batch, &g_rec.sum_im);
    for (long long i = 0; i < (long long)Gr * S * batch; ++i) Z[i] = jstsp_c64{(double)i, -(double)i};
    for (int i = 0; idx && i < K * batch; ++i) idx[i] = i + 1;
    for (int t = 0; cnt && t < batch; ++t) cnt[t] = 2 + t;
    return N == 3 ? JSTSP_E_UNSUPPORTED : 0;
}
int jstsp_mc_svt_f64(jstsp_ctx *, int Mr, int Mt, int batch, const jstsp_c64 *OH, const double *Om, int Imax, const double *tau, const double *rho,
                     jstsp_c64 *X, int memspace)
{
    std::memset(&g_rec, 0, sizeof(g_rec));
    g_rec.which = 2; g_rec.dims[0] = Mr; g_rec.dims[1] = Mt; g_rec.dims[2] = batch; g_rec.dims[3] = Imax; g_rec.memspace = memspace;
    g_rec.sum_re = sum_of(OH, (long long)Mr * Mt * batch, &g_rec.sum_im);
    for (long long i = 0; i < (long long)Mr * Mt * batch; ++i) g_rec.sum_im += Om[i];
    for (long long i = 0; i < (long long)Mr * Mt * batch; ++i) X[i] = jstsp_c64{tau[i / ((long long)Mr * Mt)], rho[i / ((long long)Mr * Mt)]};
    return 0;
}
int jstsp_mc_admm_f64(jstsp_ctx *, int Mr, int Mt, int batch, const jstsp_c64 *H, const jstsp_c64 *OH, const double *, int Imax, const double *tau,
                      const double *rho, jstsp_c64 *X, double *ce, int memspace)
{
    std::memset(&g_rec, 0, sizeof(g_rec));
    g_rec.which = 3; g_rec.dims[0] = Mr; g_rec.dims[1] = Mt; g_rec.dims[2] = batch; g_rec.dims[3] = Imax; g_rec.memspace = memspace;
    g_rec.has_a = H != nullptr; g_rec.has_b = ce != nullptr;
    g_rec.sum_re = sum_of(OH, (long long)Mr * Mt * batch, &g_rec.sum_im);
    for (long long i = 0; i < (long long)Mr * Mt * batch; ++i) X[i] = jstsp_c64{tau[i / ((long long)Mr * Mt)], rho[i / ((long long)Mr * Mt)]};
    for (int i = 0; ce && i < Imax * batch; ++i) ce[i] = 0.5 * i;
    return 0;
}
const Rec *recorder_last(void) { return &g_rec; }
}
"""


class Rec(C.Structure):
    _fields_ = [("which", C.c_int), ("dims", C.c_int * 6), ("memspace", C.c_int), ("has_a", C.c_int), ("has_b", C.c_int),
                ("sA", C.c_longlong), ("sB", C.c_longlong), ("sum_re", C.c_double), ("sum_im", C.c_double)]


@pytest.fixture(scope="module")
def mex(tmp_path_factory):
    from jstsp19_amd import build as B
    lib = B.build()
    d = tmp_path_factory.mktemp("mextssr64")
    src, rec, out = str(d / "recorder.cpp"), str(d / "libjstsp_recorder_tssr64.so"), str(d / "jstsp_mex_stub_tssr64.so")
    open(src, "w").write(RECORDER)
    r = subprocess.run(["g++", "-O1", "-Wall", "-Wextra", "-Werror", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), src, "-o", rec],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cmd = ["g++", "-O1", "-Wall", "-Wextra", "-Werror", "-std=c++17", "-shared", "-fPIC", "-DMATLAB_MEX_FILE",
           "-I" + os.path.join(ROOT, "tests", "mex_stub"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "mex", "jstsp_mex.cpp"), os.path.join(ROOT, "tests", "mex_stub", "stub.cpp"), "-o", out,
           "-Wl,--no-as-needed", "-L" + str(d), "-ljstsp_recorder_tssr64", "-L" + os.path.dirname(lib), "-ljstsp_mi355x",
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


def test_mmv_omp_f64_passes_shapes_strides_k_pnorm_and_optional_outputs_through(mex):
    rng = np.random.default_rng(3)
    A, Y = _c(rng, 6, 4), _c(rng, 6, 5, 3)                                 # shared A; N x S x pages
    Z, = call(mex, 1, "mmv_omp_f64", A, 2, Y)
    rec = mex.last()
    assert (rec.which, list(rec.dims), rec.sA, rec.memspace, rec.has_a, rec.has_b) == (1, [6, 4, 5, 3, 2, 2], 0, 0, 0, 0)
    check_below("mex_tssr64/input_sum", abs(rec.sum_re - Y.real.sum()) + abs(rec.sum_im - Y.imag.sum()), 1e-12)
    assert Z.shape == (4, 5, 3)
    k = np.arange(60, dtype=np.float64)
    check_below("mex_tssr64/output_mismatch", np.abs(Z.reshape(-1, order="F") - (k - 1j * k)).max(), 1e-300)
    Z, sup, cnt = call(mex, 3, "mmv_omp_f64", np.stack([A] * 3, axis=2), 2, Y, 1)
    rec = mex.last()
    assert (list(rec.dims), rec.sA, rec.has_a, rec.has_b) == ([6, 4, 5, 3, 2, 1], 24, 1, 1)
    assert sup.shape == (2, 3) and sup.dtype == np.int32 and np.array_equal(sup.reshape(-1, order="F"), np.arange(1, 7))
    assert cnt.shape == (3, 1) and cnt.dtype == np.int32 and np.array_equal(cnt[:, 0], [2, 3, 4])
    Z, sup = call(mex, 2, "mmv_omp_f64", A, 3, Y[:, :, 0])                 # 2-D Y: batch 1
    rec = mex.last()
    assert (list(rec.dims), rec.has_a, rec.has_b) == ([6, 4, 5, 1, 3, 2], 1, 0) and Z.shape == (4, 5)


def test_mc_svt_f64_and_mc_admm_f64_pass_batch_imax_scalars_and_null_outputs_through(mex):
    rng = np.random.default_rng(4)
    OH, H = _c(rng, 5, 7, 3), _c(rng, 5, 7, 3)
    Om = (rng.random((5, 7, 3)) < 0.5).astype(float)
    tau, rho = np.array([0.1, 0.2, 0.3]), 0.5
    X, = call(mex, 1, "mc_svt_f64", OH, Om, 9, tau, rho)
    rec = mex.last()
    assert (rec.which, list(rec.dims[:4]), rec.memspace) == (2, [5, 7, 3, 9], 0)
    check_below("mex_tssr64/input_sum", abs(rec.sum_re - OH.real.sum()) + abs(rec.sum_im - OH.imag.sum() - Om.sum()), 1e-12)
    assert X.shape == (5, 7, 3)
    for t in range(3):                                                     # one tau per page, the scalar rho for every page
        assert np.all(X[:, :, t] == tau[t] + 0.5j)
    X, ce = call(mex, 2, "mc_admm_f64", H, OH, Om, 4, tau, rho)
    rec = mex.last()
    assert (rec.which, list(rec.dims[:4]), rec.has_a, rec.has_b) == (3, [5, 7, 3, 4], 1, 1)
    assert X.shape == (5, 7, 3) and np.array_equal(ce.reshape(-1, order="F"), 0.5 * np.arange(12))
    X, = call(mex, 1, "mc_admm_f64", np.zeros((0, 0)), OH, Om, 4, tau, rho)   # one output: no error curve, Htrue may be []
    rec = mex.last()
    assert (rec.has_a, rec.has_b) == (0, 0) and np.all(X[:, :, 2] == tau[2] + 0.5j)
    X, = call(mex, 1, "mc_svt_f64", OH[:, :, 0], Om[:, :, 0], 0, 0.1, 0.2)  # 2-D: batch 1; Imax = 0 is allowed
    assert list(mex.last().dims[:4]) == [5, 7, 1, 0] and X.shape == (5, 7)


def test_bad_calls_are_refused_before_the_library_and_a_library_error_is_reported(mex):
    rng = np.random.default_rng(5)
    A, Y = _c(rng, 6, 4), _c(rng, 6, 5)
    OH, Om = _c(rng, 5, 7), np.ones((5, 7))
    for args, nlhs, ident in ((("mmv_omp_f64", A, 2), 1, "jstsp:args"), (("mmv_omp_f64", A, 2, Y, 2, 1), 1, "jstsp:args"),
                              (("mmv_omp_f64", A, 2, Y), 4, "jstsp:args"), (("mmv_omp_f64", A, 0, Y), 1, "jstsp:args"),
                              (("mmv_omp_f64", A, 2, Y, 3), 1, "jstsp:args"), (("mmv_omp_f64", A[:-1], 2, Y), 1, "jstsp:shape"),
                              (("mmv_omp_f64", np.stack([A] * 3, axis=2), 2, np.stack([Y] * 2, axis=2)), 1, "jstsp:shape"),
                              (("mc_svt_f64", OH, Om, 3, 0.1), 1, "jstsp:args"), (("mc_svt_f64", OH, Om, 3, 0.1, 0.1), 2, "jstsp:args"),
                              (("mc_svt_f64", OH, Om[:, :-1], 3, 0.1, 0.1), 1, "jstsp:shape"), (("mc_svt_f64", OH, Om, -1, 0.1, 0.1), 1, "jstsp:args"),
                              (("mc_admm_f64", OH, OH, Om, 3, 0.1), 1, "jstsp:args"), (("mc_admm_f64", OH, OH, Om, 3, 0.1, 0.1), 3, "jstsp:args"),
                              (("mc_admm_f64", OH[:-1], OH, Om, 3, 0.1, 0.1), 2, "jstsp:shape"), (("mc_admm_f64", OH, OH, Om[:-1], 3, 0.1, 0.1), 1, "jstsp:shape"),
                              (("mc_admm_f64", OH, OH, Om, 0, 0.1, 0.1), 1, "jstsp:args")):
        with pytest.raises(MexError) as e:
            call(mex, nlhs, *args)
        assert e.value.ident == ident, (args[0], str(e.value))
    with pytest.raises(MexError) as e:                                     # the recorder refuses 3 rows with JSTSP_E_UNSUPPORTED
        call(mex, 1, "mmv_omp_f64", _c(rng, 3, 2), 1, _c(rng, 3, 2))
    assert e.value.ident == "jstsp:call" and "jstsp_mmv_omp_f64" in str(e.value) and "(-3)" in str(e.value)
    for f, cmd in (("mmv_omp_f64.m", "'mmv_omp_f64'"), ("mc_svt_f64.m", "'mc_svt_f64'"), ("mc_admm_f64.m", "'mc_admm_f64'")):
        assert cmd in open(os.path.join(ROOT, "mex", f)).read()
