"""The MEX command 'proposed_algorithm_resume' (mex/jstsp_mex.cpp) without a GPU: the gateway compiles with -Wall -Wextra -Werror
against the stand-in MEX API (tests/mex_stub/), and the command hands the reference's argument list, the type, the optional
indx_S / state / it0 ([] = not given) and the optional outputs - the state among them - to jstsp_proposed_resume_c64 unchanged.
The library side is a recording stand-in for that entry (and for context creation), linked in front of the real library;
jstsp_admm_state_elems is the real one."""
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
struct Rec { int dims[6], memspace, std1, it0, has_idx, has_Y, has_ce, has_in, has_out, idx0; long long sA, sB; double tY1, rho1, sum_in; };
static Rec g_rec;
static int g_ctx_store;
extern "C" {
int jstsp_create(int, jstsp_ctx **out) { *out = reinterpret_cast<jstsp_ctx *>(&g_ctx_store); return 0; }
int jstsp_destroy(jstsp_ctx *) { return 0; }
const char *jstsp_last_error(void) { return "recorder"; }
int jstsp_proposed_resume_c64(jstsp_ctx *, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *, const double *, const jstsp_c64 *, long long sA,
                              const jstsp_c64 *, long long sB, int Imax, const double *tY, const double *, const double *rho, int type, const int32_t *idx,
                              jstsp_c64 *S, jstsp_c64 *Y, double *ce, int it0, const jstsp_c64 *in, jstsp_c64 *out, int memspace)
{
    std::memset(&g_rec, 0, sizeof(g_rec));
    const int d[6] = {N, M, Gr, G2, batch, Imax};
    std::memcpy(g_rec.dims, d, sizeof(d));
    g_rec.sA = sA; g_rec.sB = sB; g_rec.memspace = memspace; g_rec.std1 = type == JSTSP_TYPE_STD; g_rec.it0 = it0;
    g_rec.has_idx = idx != nullptr; g_rec.has_Y = Y != nullptr; g_rec.has_ce = ce != nullptr; g_rec.has_in = in != nullptr; g_rec.has_out = out != nullptr;
    g_rec.idx0 = idx ? idx[0] : 0;
    g_rec.tY1 = tY[batch - 1]; g_rec.rho1 = rho[batch - 1];
    const long long ne = 4ll * N * M + 2ll * Gr * G2;
    if (in) for (long long i = 0; i < ne * batch; ++i) g_rec.sum_in += in[i].re - in[i].im;
    for (long long i = 0; i < (long long)Gr * G2 * batch; ++i) S[i] = jstsp_c64{(double)i, -(double)i};
    if (Y) for (long long i = 0; i < (long long)N * M * batch; ++i) Y[i] = jstsp_c64{1.0, 2.0};
    if (ce) for (long long i = 0; i < 3ll * Imax * batch; ++i) ce[i] = (double)i;
    if (out) for (long long i = 0; i < ne * batch; ++i) out[i] = jstsp_c64{(double)(i % ne), (double)(i / ne)};
    return N == 3 ? JSTSP_E_ARG : 0;
}
const Rec *recorder_last(void) { return &g_rec; }
}
"""


class Rec(C.Structure):
    _fields_ = [("dims", C.c_int * 6)] + \
               [(n, C.c_int) for n in ("memspace", "std1", "it0", "has_idx", "has_Y", "has_ce", "has_in", "has_out", "idx0")] + \
               [("sA", C.c_longlong), ("sB", C.c_longlong)] + [(n, C.c_double) for n in ("tY1", "rho1", "sum_in")]


@pytest.fixture(scope="module")
def mex(tmp_path_factory):
    from jstsp19_amd import build as B
    lib = B.build()
    d = tmp_path_factory.mktemp("mexresume32")
    src, rec, out = str(d / "recorder.cpp"), str(d / "libjstsp_recorder_resume32.so"), str(d / "jstsp_mex_stub_resume32.so")
    open(src, "w").write(RECORDER)
    r = subprocess.run(["g++", "-O1", "-Wall", "-Wextra", "-Werror", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), src, "-o", rec],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cmd = ["g++", "-O1", "-Wall", "-Wextra", "-Werror", "-std=c++17", "-shared", "-fPIC", "-DMATLAB_MEX_FILE",
           "-I" + os.path.join(ROOT, "tests", "mex_stub"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "mex", "jstsp_mex.cpp"), os.path.join(ROOT, "tests", "mex_stub", "stub.cpp"), "-o", out,
           "-Wl,--no-as-needed", "-L" + str(d), "-ljstsp_recorder_resume32", "-L" + os.path.dirname(lib), "-ljstsp_mi355x",
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


N, M, GR, G2, NB = 6, 9, 4, 5, 3
NE = 4 * N * M + 2 * GR * G2
FN = "proposed_algorithm_resume"


def _problem(rng):
    return _c(rng, N, M, NB), np.ones((N, M, NB)), _c(rng, N, GR), _c(rng, G2, M, NB)      # shared A, per-page B


def test_from_zero_the_argument_list_and_the_optional_outputs_pass_through(mex):
    rng = np.random.default_rng(3)
    subY, Om, A, B = _problem(rng)
    tY = np.array([0.1, 0.2, 0.3])
    S, = call(mex, 1, FN, subY, Om, A, B, 7, tY, 0.5, 0.25, "approximate")
    rec = mex.last()
    assert list(rec.dims) == [N, M, GR, G2, NB, 7] and (rec.sA, rec.sB, rec.memspace, rec.std1, rec.it0) == (0, G2 * M, 0, 0, 0)
    assert (rec.has_idx, rec.has_Y, rec.has_ce, rec.has_in, rec.has_out) == (0, 0, 0, 0, 0) and (rec.tY1, rec.rho1) == (0.3, 0.25)
    k = np.arange(GR * G2 * NB, dtype=np.float64)
    assert S.shape == (GR, G2, NB) and np.array_equal(S.reshape(-1, order="F"), k - 1j * k)
    S, Y, ce, st = call(mex, 4, FN, subY, Om, A, B, 7, tY, 0.5, 0.25, "std")
    rec = mex.last()
    assert (rec.std1, rec.has_Y, rec.has_ce, rec.has_in, rec.has_out) == (1, 1, 1, 0, 1)
    assert Y.shape == (N, M, NB) and np.all(Y == 1 + 2j) and ce.shape == (7, 3, NB)
    assert st.shape == (NE, NB)                                             # one column per problem: the stride of the C ABI
    for t in range(NB):
        assert np.array_equal(st[:, t], np.arange(NE) + 1j * t)


def test_a_state_it0_and_indx_S_pass_through_and_may_be_empty(mex):
    rng = np.random.default_rng(4)
    subY, Om, A, B = _problem(rng)
    idx = np.stack([rng.permutation(GR * G2) + 1 for _ in range(NB)], axis=1).astype(float)
    st = _c(rng, NE, NB)
    e0 = np.zeros((0, 0))
    for typ in ("approximate", "std"):
        call(mex, 4, FN, subY, Om, A, B, 2, 0.1, 0.5, 0.25, typ, idx, st, 11)
        rec = mex.last()
        assert (rec.std1, rec.has_idx, rec.idx0, rec.has_in, rec.has_out, rec.it0) == (int(typ == "std"), 1, int(idx[0, 0]), 1, 1, 11)
        assert abs(rec.sum_in - (st.real - st.imag).sum()) < 1e-10
        call(mex, 1, FN, subY, Om, A, B, 2, 0.1, 0.5, 0.25, typ, e0, st, 4)
        rec = mex.last()
        assert (rec.has_idx, rec.has_in, rec.has_out, rec.it0) == (0, 1, 0, 4)
        call(mex, 1, FN, subY, Om, A, B, 2, 0.1, 0.5, 0.25, typ, idx, e0)
        rec = mex.last()
        assert (rec.has_idx, rec.has_in, rec.it0) == (1, 0, 0)
    call(mex, 1, FN, subY, Om, A, B, 2, 0.1, 0.5, 0.25, "approximate", e0, st.real, 1)          # a real state is widened
    assert abs(mex.last().sum_in - st.real.sum()) < 1e-10


def test_bad_calls_are_refused_before_the_library_and_a_library_error_is_reported(mex):
    rng = np.random.default_rng(5)
    subY, Om, A, B = _problem(rng)
    good = (subY, Om, A, B, 2, 0.1, 0.5, 0.25, "approximate")
    st, e0 = _c(rng, NE, NB), np.zeros((0, 0))
    for args, nlhs, ident in ((good[:8], 1, "jstsp:args"), (good, 5, "jstsp:args"), (good + (e0, st, 1, 2), 1, "jstsp:args"),
                              (good[:8] + ("exact",), 1, "jstsp:args"), (good[:4] + (0,) + good[5:], 1, "jstsp:args"),
                              (good + (e0, st, -1), 1, "jstsp:args"), (good + (e0, e0, 3), 1, "jstsp:args"),      # it0 < 0; it0 without a state
                              ((subY, Om, A[:-1], B) + good[4:], 1, "jstsp:shape"), ((subY, Om[:, :-1], A, B) + good[4:], 1, "jstsp:shape"),
                              (good + (np.arange(1.0, 20.0),), 1, "jstsp:shape"),                 # numel(indx_S) != Gr G2 per page
                              (good + (e0, st[:-1]), 1, "jstsp:shape"), (good + (e0, st[:, :2]), 1, "jstsp:shape")):
        with pytest.raises(MexError) as e:
            call(mex, nlhs, FN, *args)
        assert e.value.ident == ident, str(e.value)
    with pytest.raises(MexError) as e:                                     # the recorder refuses N = 3 with JSTSP_E_ARG
        call(mex, 1, FN, subY[:3], Om[:3], A[:3], B, 2, 0.1, 0.5, 0.25, "approximate")
    assert e.value.ident == "jstsp:call" and "jstsp_proposed_resume_c64" in str(e.value) and "(-4)" in str(e.value)
    assert "'%s'" % FN in open(os.path.join(ROOT, "mex", FN + ".m")).read()
