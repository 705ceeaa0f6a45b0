"""The interface of the float64 SVD with vectors without a GPU: the two prototypes in include/jstsp.h argument by argument, the
ctypes table and the built library, the Python wrappers (exported, refusing bad arguments before any device call, raising
without a device - there is no CPU fallback) and the MATLAB wrappers."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import jstsp19_amd as J
from jstsp19_amd import _lib, solvers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "jstsp_svd_f64": ["jstsp_ctx *ctx", "int rows", "int cols", "int batch", "const jstsp_c64 *A", "int n_keep", "jstsp_c64 *U", "double *sv",
                      "jstsp_c64 *V", "int32_t *rank_out", "int32_t *conv_out", "int memspace"],
    "jstsp_lowrank_f64": ["jstsp_ctx *ctx", "int rows", "int cols", "int batch", "const jstsp_c64 *A", "int R", "jstsp_c64 *X",
                          "double *tail_out", "int memspace"],
}
CTYPES = {"int": C.c_int}


def test_prototypes_argument_by_argument():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jstsp.h")).read(), flags=re.S)
    for name, want in PROTOTYPES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name
        got = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
        assert got == want, (name, got)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(want)
        for a, decl in zip(args, want):
            assert a is (C.c_void_p if "*" in decl else CTYPES[decl.split()[0]]), (name, decl)


def test_the_library_exports_both_entries():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in PROTOTYPES:
        assert hasattr(lib, name), name
        assert hasattr(J.load(), name)


def test_wrappers_are_exported_and_refuse_bad_arguments_before_any_device_call():
    for n in ("svd_f64", "lowrank_f64"):
        assert n in solvers.__all__ and getattr(J, n) is getattr(solvers, n)
    A = np.zeros((2, 4, 6), dtype=np.complex128)
    for bad in (lambda: J.svd_f64(np.zeros((2, 2, 4, 6))), lambda: J.lowrank_f64(np.zeros((2, 2, 4, 6)), 1), lambda: J.svd_f64(np.zeros(4)),
                lambda: J.svd_f64(A, 0), lambda: J.svd_f64(A, 5), lambda: J.lowrank_f64(A, 0), lambda: J.lowrank_f64(A, 5),
                lambda: J.svd_f64(torch.zeros(4, 6, dtype=torch.complex128)), lambda: J.lowrank_f64(torch.zeros(4, 6, dtype=torch.complex128), 2)):
        with pytest.raises(ValueError):
            bad()


def test_no_cpu_fallback():
    calls = (lambda: J.svd_f64(np.eye(3, dtype=complex)), lambda: J.lowrank_f64(np.eye(3, dtype=complex), 1))
    if torch.cuda.is_available():                        # with a device the same calls answer
        assert np.array_equal(calls[0]()[1], np.ones(3)) and np.array_equal(calls[1](), np.diag([1.0 + 0j, 0, 0]))
        return
    for call in calls:
        with pytest.raises(J.JstspError):
            call()


def test_matlab_wrappers_exist_and_name_their_commands():
    for f, cmd in (("svd_f64.m", "'svd_f64'"), ("lowrank_f64.m", "'lowrank_f64'")):
        src = open(os.path.join(ROOT, "mex", f)).read()
        assert cmd in src and "jstsp_mex(" in src
    gw = open(os.path.join(ROOT, "mex", "jstsp_mex.cpp")).read()
    assert '"svd_f64"' in gw and '"lowrank_f64"' in gw and "jstsp_svd_f64(" in gw and "jstsp_lowrank_f64(" in gw
