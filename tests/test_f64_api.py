"""The float64 solver's public surface without a GPU: the five Python names exist and fail loudly (no fallback), and the MEX
gateway built against tests/mex_stub knows the 'proposed_algorithm_f64' command and checks its argument count."""
import os
import subprocess

import numpy as np
import pytest

import jstsp19_amd as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("proposed_algorithm_f64", "proposed_algorithm_angles_f64", "svt_f64", "correlate_f64", "synthesize_f64")


def test_the_five_names_are_exported():
    from jstsp19_amd import solvers
    for n in NAMES:
        assert callable(getattr(J, n)) and n in solvers.__all__
    lib = J.load()
    for n in ("jstsp_proposed_algorithm_f64", "jstsp_svt_f64", "jstsp_correlate_f64", "jstsp_synthesize_f64"):
        assert hasattr(lib, n)


def test_they_raise_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rng = np.random.default_rng(0)
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    A, B, K, S = c(4, 3), c(5, 6), c(4, 6), c(3, 5)
    Om = np.ones((4, 6))
    calls = [lambda: J.proposed_algorithm_f64(K, Om, A, B, 3, 0.1, 0.1, 0.5),
             lambda: J.proposed_algorithm_angles_f64(K, Om, np.arange(1, 16), A, B, 3, 0.1, 0.1, 0.5),
             lambda: J.svt_f64(K, 0.1), lambda: J.correlate_f64(K, A, B), lambda: J.synthesize_f64(S, A, B)]
    for f in calls:
        with pytest.raises(J.JstspError):
            f()


def test_bad_shapes_raise_value_error_before_any_device_work():
    A, B, K = np.zeros((4, 3), complex), np.zeros((5, 6), complex), np.zeros((4, 6), complex)
    with pytest.raises(ValueError):
        J.proposed_algorithm_f64(K, np.ones((4, 5)), A, B, 3, 0.1, 0.1, 0.5)
    with pytest.raises(ValueError):
        J.proposed_algorithm_f64(K, np.ones((4, 6)), A[:-1], B, 3, 0.1, 0.1, 0.5)
    with pytest.raises(ValueError):
        J.correlate_f64(K, A, B[:, :-1])


def test_mex_gateway_knows_the_f64_command_and_checks_its_argument_count(tmp_path):
    import ctypes as C
    from jstsp19_amd import build as B
    lib = B.build()
    out = str(tmp_path / "jstsp_mex_stub.so")
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
        dims = (C.c_size_t * 2)(*x.shape)
        a = m.mxCreateNumericArray(2, dims, 6, 1 if cplx else 0)
        buf = np.ascontiguousarray(x.astype(np.complex128 if cplx else np.float64).reshape(-1, order="F"))
        C.memmove(m.mxGetData(a), buf.ctypes.data, buf.nbytes)
        return a

    def call(nlhs, *args):
        prhs = (vp * len(args))(*[to_mx(a) for a in args])
        plhs = (vp * max(nlhs, 1))()
        if m.stub_call(nlhs, plhs, len(args), prhs):
            return m.stub_error_id().decode(), m.stub_error_message().decode()
        return None, None

    rng = np.random.default_rng(1)
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    subY, Om, A, Bm = c(12, 20), np.ones((12, 20)), c(12, 9), c(10, 20)
    ident, msg = call(1, "proposed_algorithm_f64", subY, Om, A, Bm)                    # nine inputs, as proposed_algorithm.m:1
    assert ident == "jstsp:args" and "proposed_algorithm_f64" in msg and "9 to 10" in msg
    ident, msg = call(4, "proposed_algorithm_f64", subY, Om, A, Bm, 5, 1.0, 1.0, 0.2, "approximate")
    assert ident == "jstsp:args" and "output" in msg
    ident, msg = call(1, "proposed_algorithm_f64", subY, Om, A[:-1], Bm, 5, 1.0, 1.0, 0.2, "approximate")
    assert ident == "jstsp:shape"
    ident, msg = call(1, "proposed_algorithm_f65", subY)
    assert ident == "jstsp:args" and "unknown function" in msg
    if not torch.cuda.is_available():           # known command, good arguments, no GPU: the failing jstsp_create, loudly
        ident, msg = call(1, "proposed_algorithm_f64", subY, Om, A, Bm, 5, 1.0, 1.0, 0.2, "approximate")
        assert ident == "jstsp:call" and "jstsp_create" in msg
    for f in ("proposed_algorithm_f64.m", "proposed_algorithm_angles_f64.m"):
        assert "'proposed_algorithm_f64'" in open(os.path.join(ROOT, "mex", f)).read()
    m.stub_run_at_exit()
