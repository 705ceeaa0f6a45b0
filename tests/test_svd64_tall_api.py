"""The interface of the float64 SVD with vectors on the QR route without a GPU: the two prototypes in include/jstsp.h argument by
argument, the ctypes table and the built library, the Python wrappers (exported, refusing bad arguments before any device call,
raising without a device - there is no CPU fallback), the per-matrix workspace figure the wrappers chunk a batch by, and the MATLAB
wrappers and gateway commands."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import jstsp19_amd as J
import svd64_tall_problems as T
from jstsp19_amd import _lib, solvers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "jstsp_svd_tall_f64": ["jstsp_ctx *ctx", "int rows", "int cols", "int batch", "const jstsp_c64 *A", "int n_keep", "jstsp_c64 *U",
                           "double *sv", "jstsp_c64 *V", "int32_t *rank_out", "int32_t *conv_out", "int memspace"],
    "jstsp_lowrank_tall_f64": ["jstsp_ctx *ctx", "int rows", "int cols", "int batch", "const jstsp_c64 *A", "int R", "jstsp_c64 *X",
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
    # the arguments of the entries they stand beside
    for name in PROTOTYPES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt), re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name.replace("_tall", ""), txt)
        assert re.sub(r"\s+", " ", m[0].group(1)) == re.sub(r"\s+", " ", m[1].group(1)), name


def test_the_library_exports_both_entries():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in PROTOTYPES:
        assert hasattr(lib, name), name
        assert hasattr(J.load(), name)


def test_wrappers_are_exported_and_refuse_bad_arguments_before_any_device_call():
    for n in ("svd_tall_f64", "lowrank_tall_f64"):
        assert n in solvers.__all__ and getattr(J, n) is getattr(solvers, n)
    A = np.zeros((2, 4, 6), dtype=np.complex128)
    for bad in (lambda: J.svd_tall_f64(np.zeros((2, 2, 4, 6))), lambda: J.lowrank_tall_f64(np.zeros((2, 2, 4, 6)), 1),
                lambda: J.svd_tall_f64(np.zeros(4)), lambda: J.svd_tall_f64(A, 0), lambda: J.svd_tall_f64(A, 5),
                lambda: J.lowrank_tall_f64(A, 0), lambda: J.lowrank_tall_f64(A, 5),
                lambda: J.svd_tall_f64(torch.zeros(4, 6, dtype=torch.complex128)),
                lambda: J.lowrank_tall_f64(torch.zeros(4, 6, dtype=torch.complex128), 2)):
        with pytest.raises(ValueError):
            bad()


def test_the_chunking_figure_covers_the_reflector_store():
    """the wrappers cut a batch by a per-matrix figure that has to cover what tall_layout (csrc/svd64.hip) takes, every array
    rounded up to 256 bytes: the restated figure plus five roundings, and for a host call the staged operand and outputs"""
    for rows, cols, keep in ((64, 65536, 64), (65536, 64, 1), (9000, 33, 7), (1, 7, 1), (5, 3, 3)):
        a = solvers._Arg(np.zeros((1, rows, cols), dtype=np.complex128), np.complex128, "A")
        dev = solvers._svd_tall_per_matrix(a, keep, _lib.DEVICE)
        assert dev >= T.workspace_bytes(rows, cols, keep) + 5 * 255, (rows, cols, keep)
        host = solvers._svd_tall_per_matrix(a, keep, _lib.HOST)
        assert host >= dev + 16 * (rows * cols + (rows + cols) * keep) + 8 * keep + 8
    a = solvers._Arg(np.zeros((1, 64, 65536), dtype=np.complex128), np.complex128, "A")
    assert (24 << 30) // solvers._svd_tall_per_matrix(a, 64, _lib.DEVICE) < 400     # (the batch the C entry refuses in the GPU test)


def test_no_cpu_fallback():
    calls = (lambda: J.svd_tall_f64(np.eye(3, dtype=complex)), lambda: J.lowrank_tall_f64(np.eye(3, dtype=complex), 1))
    if torch.cuda.is_available():                        # with a device the same calls answer
        assert np.array_equal(calls[0]()[1], np.ones(3)) and np.array_equal(calls[1](), np.diag([1.0 + 0j, 0, 0]))
        return
    for call in calls:
        with pytest.raises(J.JstspError):
            call()


def test_matlab_wrappers_exist_and_name_their_commands():
    for f, cmd in (("svd_tall_f64.m", "'svd_tall_f64'"), ("lowrank_tall_f64.m", "'lowrank_tall_f64'")):
        src = open(os.path.join(ROOT, "mex", f)).read()
        assert cmd in src and "jstsp_mex(" in src
    gw = open(os.path.join(ROOT, "mex", "jstsp_mex.cpp")).read()
    assert '"svd_tall_f64"' in gw and '"lowrank_tall_f64"' in gw and "jstsp_svd_tall_f64(" in gw and "jstsp_lowrank_tall_f64(" in gw
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "'svd_tall_f64'" in doc and "'lowrank_tall_f64'" in doc
