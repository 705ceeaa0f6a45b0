"""The MEX commands 'omp_f64' and 'sparse_admm_f64' (mex/jstsp_mex.cpp) without a GPU: the gateway compiles with -Wall -Wextra
-Werror against the stand-in MEX API (tests/mex_stub/), knows both commands, reports a wrong argument count as jstsp:args and
inconsistent dimensions as jstsp:shape, and the wrappers mex/OMP_f64.m and mex/sparse_admm_f64.m name their command."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def call(tmp_path_factory):
    from jstsp19_amd import build as B
    lib = B.build()
    out = str(tmp_path_factory.mktemp("mexomp64") / "jstsp_mex_stub_omp64.so")
    cmd = ["g++", "-O1", "-Wall", "-Wextra", "-Werror", "-std=c++17", "-shared", "-fPIC", "-DMATLAB_MEX_FILE",
           "-I" + os.path.join(ROOT, "tests", "mex_stub"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "mex", "jstsp_mex.cpp"), os.path.join(ROOT, "tests", "mex_stub", "stub.cpp"), "-o", out,
           "-L" + os.path.dirname(lib), "-ljstsp_mi355x", "-Wl,-rpath," + os.path.dirname(lib)]
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
    m.stub_call.argtypes = [C.c_int, C.POINTER(vp), C.c_int, C.POINTER(vp)]
    m.stub_error_id.restype = C.c_char_p
    m.stub_error_message.restype = C.c_char_p

    def to_mx(x):
        if isinstance(x, str):
            return m.mxCreateString(x.encode())
        if np.isscalar(x):
            return m.mxCreateDoubleScalar(float(x))
        x = np.asarray(x)
        cplx = np.iscomplexobj(x)
        dims = (C.c_size_t * x.ndim)(*x.shape)
        a = m.mxCreateNumericArray(x.ndim, dims, 6, 1 if cplx else 0)
        buf = np.ascontiguousarray(x.astype(np.complex128 if cplx else np.float64).reshape(-1, order="F"))
        C.memmove(m.mxGetData(a), buf.ctypes.data, buf.nbytes)
        return a

    def call_(nlhs, *args):
        prhs = (vp * len(args))(*[to_mx(a) for a in args])
        plhs = (vp * max(nlhs, 1))()
        if m.stub_call(nlhs, plhs, len(args), prhs):
            return m.stub_error_id().decode(), m.stub_error_message().decode()
        return None, None

    yield call_
    m.stub_run_at_exit()


def _c(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def test_omp_f64_is_known_and_checks_counts_and_shapes(call):
    rng = np.random.default_rng(5)
    A, v = _c(rng, 6, 9), _c(rng, 6, 1)
    ident, msg = call(1, "omp_f64", A, v)                                     # OMP.m:1 takes A, v, m (, snr)
    assert ident == "jstsp:args" and "omp_f64" in msg and "unknown function" not in msg
    ident, msg = call(5, "omp_f64", A, v, 3)
    assert ident == "jstsp:args" and "output" in msg
    ident, msg = call(1, "omp_f64", A, v[:-1], 3)
    assert ident == "jstsp:shape" and "omp_f64" in msg
    ident, msg = call(1, "omp_f64", A, v, 0)
    assert ident == "jstsp:args" and "m must be" in msg
    ident, msg = call(1, "omp_f65", A, v, 3)
    assert ident == "jstsp:args" and "unknown function" in msg
    import torch
    if not torch.cuda.is_available():           # known command, good arguments, no GPU: the failing jstsp_create, loudly
        ident, msg = call(1, "omp_f64", A, v, 3, 10.0)
        assert ident == "jstsp:call" and "jstsp_create" in msg


def test_sparse_admm_f64_is_known_and_checks_counts_and_shapes(call):
    rng = np.random.default_rng(6)
    H, OH, Dr, Dt = _c(rng, 4, 3), _c(rng, 4, 3), _c(rng, 4, 4), _c(rng, 3, 3)
    ident, msg = call(1, "sparse_admm_f64", H, OH, Dr, Dt)                    # sparse_admm.m:1 takes five inputs
    assert ident == "jstsp:args" and "sparse_admm_f64" in msg and "unknown function" not in msg
    ident, msg = call(3, "sparse_admm_f64", H, OH, Dr, Dt, 5)
    assert ident == "jstsp:args" and "output" in msg
    ident, msg = call(1, "sparse_admm_f64", H[:-1], OH, Dr, Dt, 5)
    assert ident == "jstsp:shape" and "sparse_admm_f64" in msg
    ident, msg = call(1, "sparse_admm_f64", H, OH, Dr[:-1], Dt, 5)
    assert ident == "jstsp:shape"
    ident, msg = call(1, "sparse_admm_f64", H, OH, Dr, Dt, 0)
    assert ident == "jstsp:args" and "Imax" in msg
    import torch
    if not torch.cuda.is_available():
        ident, msg = call(2, "sparse_admm_f64", H, OH, Dr, Dt, 5)
        assert ident == "jstsp:call" and "jstsp_create" in msg


def test_the_wrappers_name_their_command_and_keep_the_reference_signatures():
    omp = open(os.path.join(ROOT, "mex", "OMP_f64.m")).read()
    assert "'omp_f64'" in omp and "function [x_hat, indexSet, v, targetMatrix] = OMP_f64(A, v, m, snr)" in omp
    sa = open(os.path.join(ROOT, "mex", "sparse_admm_f64.m")).read()
    assert "'sparse_admm_f64'" in sa and "function [S, convergence_error] = sparse_admm_f64(Htrue, OH, Dr, Dt, Imax)" in sa
    # the fp32 commands are still there, unchanged in name
    src = open(os.path.join(ROOT, "mex", "jstsp_mex.cpp")).read()
    for name in ('"OMP"', '"omp_f64"', '"sparse_admm"', '"sparse_admm_f64"', "jstsp_omp_c64", "jstsp_sparse_admm_c64"):
        assert name in src
