"""Alg. 1 in float64 - the public surface without a GPU: the symbol is declared in include/jstsp.h and exported, the ctypes
prototype matches the declaration, the Python names exist, check their arguments before any device work and fail loudly without
a GPU (no fallback), and the MATLAB wrapper names the MEX command."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import jstsp19_amd as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declaration():
    h = open(os.path.join(ROOT, "include", "jstsp.h")).read()
    m = re.search(r"\bint\s+jstsp_proposed_std_f64\s*\(([^;]*)\)\s*;", h)
    assert m, "jstsp_proposed_std_f64 is not declared in include/jstsp.h"
    return h, [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def test_the_symbol_is_declared_exported_and_its_prototype_matches():
    from jstsp19_amd import _lib
    h, args = _declaration()
    res, proto = _lib.SIGNATURES["jstsp_proposed_std_f64"]
    assert res is C.c_int and len(proto) == len(args) == 24
    for a, p in zip(args, proto):
        if "*" in a:
            assert p in (C.c_void_p, _lib.c_dp), a
        elif a.startswith("long long"):
            assert p is C.c_longlong, a
        else:
            assert a.startswith("int ") and p is C.c_int, a
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names == ["ctx", "N", "M", "Gr", "G2", "batch", "subY", "Omega", "A", "strideA", "B", "strideB", "PA", "PB", "Imax", "tau_Y", "tau_S",
                     "rho", "indx_S", "S_out", "Y_out", "ce_out", "rcond_out", "memspace"]
    assert hasattr(J.load(), "jstsp_proposed_std_f64")
    # the refusing entry keeps its text and points here
    assert "jstsp_proposed_std_f64 below" in h
    assert "'std' has no float64 path" in open(os.path.join(ROOT, "jstsp19_amd", "csrc", "proposed64.hip")).read()


def test_the_python_names_and_their_signatures():
    from jstsp19_amd import solvers
    for n in ("proposed_algorithm_std_f64", "proposed_algorithm_angles_std_f64"):
        assert callable(getattr(J, n)) and n in solvers.__all__
    p = inspect.signature(J.proposed_algorithm_std_f64).parameters
    assert list(p)[:8] == ["subY", "Omega", "A", "B", "Imax", "tau_Y", "tau_S", "rho"]
    for k, d in (("indx_S", None), ("PA", None), ("PB", None), ("want_ce", True), ("info", False), ("ctx", None)):
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is d
    assert list(inspect.signature(J.proposed_algorithm_angles_std_f64).parameters)[:3] == ["subY", "Omega", "indx_S"]
    from jstsp19_amd import montecarlo
    assert inspect.signature(montecarlo.run_approx_sweep).parameters["precision"].default == "f32"


def test_bad_arguments_raise_value_error_before_any_device_work():
    A, B, K, Om = np.zeros((6, 3), complex), np.zeros((4, 8), complex), np.zeros((6, 8), complex), np.ones((6, 8))
    f = J.proposed_algorithm_std_f64
    with pytest.raises(ValueError):
        f(K, np.ones((6, 7)), A, B, 3, 0.1, 0.1, 0.5)
    with pytest.raises(ValueError):
        f(K, Om, A[:-1], B, 3, 0.1, 0.1, 0.5)
    with pytest.raises(ValueError):
        f(K, Om, A, B, 3, 0.1, 0.1, 0.5, PA=np.zeros((6, 3), complex))                 # pinv(A) is Gr x N
    with pytest.raises(ValueError):
        f(K, Om, A, B, 3, 0.1, 0.1, 0.5, PB=np.zeros((2, 8, 4), complex))              # B is shared, PB is not
    with pytest.raises(ValueError):
        f(K, Om, A, B, 3, np.ones(2), 0.1, 0.5)
    from jstsp19_amd import montecarlo
    from jstsp19_amd.system_model import TrainingParams
    with pytest.raises(ValueError):
        montecarlo.run_approx_sweep(TrainingParams(), [0.0], [10], 1, precision="f16", device="cpu")
    with pytest.raises(ValueError):
        montecarlo.run_approx_sweep(TrainingParams(), [0.0], [10], 1, precision="f64", solve_fn=lambda i, k: (0, 0), device="cpu")


def test_they_raise_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rng = np.random.default_rng(0)
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    A, B, K, Om = c(6, 3), c(4, 8), c(6, 8), np.ones((6, 8))
    for f in (lambda: J.proposed_algorithm_std_f64(K, Om, A, B, 3, 0.1, 0.1, 0.5),
              lambda: J.proposed_algorithm_std_f64(K, Om, A, B, 3, 0.1, 0.1, 0.5, PA=np.linalg.pinv(A), PB=np.linalg.pinv(B), info=True),
              lambda: J.proposed_algorithm_angles_std_f64(K, Om, np.arange(1, 13), A, B, 3, 0.1, 0.1, 0.5)):
        with pytest.raises(J.JstspError):
            f()


def test_the_matlab_wrapper_and_the_tools_name_the_feature():
    assert "'proposed_algorithm_std_f64'" in open(os.path.join(ROOT, "mex", "proposed_algorithm_std_f64.m")).read()
    assert '"proposed_algorithm_std_f64"' in open(os.path.join(ROOT, "mex", "jstsp_mex.cpp")).read()
    assert "--f64" in open(os.path.join(ROOT, "tools", "run_errorVSsnr_approx.py")).read()
    assert "--std" in open(os.path.join(ROOT, "tools", "float64_reference.py")).read()
