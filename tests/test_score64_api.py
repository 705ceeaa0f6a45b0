"""The interface of the device scoring of float64 estimates without a GPU: the two prototypes in include/jstsp.h argument by
argument, the ctypes table and the built library, the Python wrappers (exported, refusing bad arguments before any device call,
raising without a device - there is no CPU fallback) and the ``score`` keyword of the sweep runner (default "host", validated
before any device work)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import jstsp19_amd as J
from jstsp19_amd import _lib, montecarlo as mc, solvers
from jstsp19_amd.system_model import TrainingParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "jstsp_nmse_spectral_f64": ["jstsp_ctx *ctx", "int R", "int C", "int batch", "const jstsp_c64 *S", "const jstsp_c64 *Zbar", "double *nmse",
                                "int memspace"],
    "jstsp_rate_f64": ["jstsp_ctx *ctx", "int R", "int C", "int batch", "const jstsp_c64 *S", "const jstsp_c64 *Zbar", "double noise_var",
                       "double *rate", "int memspace"],
}
CTYPES = {"int": C.c_int, "double": C.c_double}


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
    for n in ("nmse_spectral_f64", "rate_f64"):
        assert n in solvers.__all__ and getattr(J, n) is getattr(solvers, n)
    Z = np.zeros((2, 4, 6), dtype=np.complex128)
    for bad in (lambda: J.nmse_spectral_f64(Z, Z[:, :3]), lambda: J.rate_f64(Z, Z[:1], 0.1), lambda: J.nmse_spectral_f64(np.zeros(4), np.zeros(4)),
                lambda: J.nmse_spectral_f64(torch.zeros(4, 6, dtype=torch.complex128), torch.zeros(4, 6, dtype=torch.complex128)),
                lambda: J.rate_f64(Z, torch.zeros(2, 4, 6, dtype=torch.complex64), 0.1)):
        with pytest.raises(ValueError):
            bad()


def test_no_cpu_fallback():
    Z = np.eye(3, dtype=complex)
    calls = (lambda: J.nmse_spectral_f64(3 * Z, Z), lambda: J.rate_f64(Z, Z, 1.0 / 3.0))
    if torch.cuda.is_available():                        # with a device the same calls answer
        assert calls[0]() == 1.0 and abs(calls[1]() - 3.0) < 1e-14
        return
    for call in calls:
        with pytest.raises(J.JstspError):
            call()


def test_score_defaults_to_host_and_is_validated_before_any_device_work():
    for f in (mc.run_points, mc._hip_baselines, mc.run_approx_sweep, mc._hip_alg12_f64):
        assert inspect.signature(f).parameters["score"].default == "host", f.__name__
    base = TrainingParams(Nt=4, Nr=32, L=4, T=140, ratio=0.75)
    for bad in ("gpu", "f64"):
        with pytest.raises(ValueError, match="score"):
            mc.run_points([], 1, score=bad, device="cpu", builder=lambda *a: None)
        with pytest.raises(ValueError, match="score"):
            mc._hip_baselines({}, 100, ls_precision="f64", mmv_precision="f64", score=bad)
        with pytest.raises(ValueError, match="score"):
            mc.run_approx_sweep(base, [10.0], [10], 2, precision="f64", score=bad, device="cpu", builder=lambda *a: None)
        with pytest.raises(ValueError, match="score"):
            mc._hip_alg12_f64({}, [10], score=bad)
    # the accepted values pass the check: an empty sweep on the CPU-side hook does no device work and returns
    for ok in ("host", "device"):
        assert mc.run_points([], 1, score=ok, device="cpu", builder=lambda *a: None).shape == (0, 2)


def test_matlab_wrappers_exist_and_name_their_commands():
    for f, cmd in (("nmse_spectral_f64.m", "'nmse_spectral_f64'"), ("rate_f64.m", "'rate_f64'")):
        src = open(os.path.join(ROOT, "mex", f)).read()
        assert cmd in src and "jstsp_mex(" in src
    gw = open(os.path.join(ROOT, "mex", "jstsp_mex.cpp")).read()
    assert '"nmse_spectral_f64"' in gw and '"rate_f64"' in gw and "jstsp_nmse_spectral_f64(" in gw and "jstsp_rate_f64(" in gw
