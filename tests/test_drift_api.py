"""The public surface of the drifting tracked channel and of the support order without a GPU: the header declares the three
entries with their argument lists, the ctypes table binds them, the built library exports them, build_trials takes drift=, the
solvers module exports support_order / support_order_f64, and run_tracking takes drift= and the three PAI modes."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import jstsp19_amd as J
from jstsp19_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIFT = "jstsp_build_trials_tracked_drift_c32"
ORDER32, ORDER64 = "jstsp_support_order_c32", "jstsp_support_order_f64"


def _prototype(name):
    h = open(os.path.join(ROOT, "include", "jstsp.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, h)
    assert m, "no prototype of %s" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")], h[:m.start()].rsplit("/*", 1)[1]


def test_header_declares_the_drift_entry_with_its_13_arguments():
    args, doc = _prototype(DRIFT)
    assert args == ["jstsp_ctx *ctx", "const jstsp_model *model", "uint64_t seed", "int sweep_idx", "long long trial0", "int batch",
                    "int frame", "double corr", "double drift", "const jstsp_trials *out", "double *dphi_r", "double *dphi_t",
                    "int memspace"]
    for word in ("wideband_mmwave_channel.m:56-62", "O(frame)", "JSTSP_E_ARG", "build_trials_tracked", "drift == 0", "dphi_r"):
        assert word in doc, word


def test_header_declares_the_support_order_entries():
    a32, _ = _prototype(ORDER32)
    a64, doc = _prototype(ORDER64)
    assert a32 == ["jstsp_ctx *ctx", "int Gr", "int G2", "int batch", "const jstsp_c32 *S", "int32_t *indx_S", "int memspace"]
    assert a64 == ["jstsp_ctx *ctx", "int Gr", "int G2", "int batch", "const double *S", "int32_t *indx_S", "int memspace"]
    for word in ("plot_errorVSsnr.m:143", "ascending index", "NaN", "JSTSP_E_SHAPE", "JSTSP_E_NULL"):
        assert word in doc, word


def test_signature_table_has_them():
    res, args = _lib.SIGNATURES[DRIFT]
    tracked = _lib.SIGNATURES["jstsp_build_trials_tracked_c32"][1]
    assert res is _lib.c_int and len(args) == 13
    assert args[:8] == tracked[:8] and args[8] is C.c_double and args[9] == tracked[8] and args[12] == tracked[9]
    for n in (ORDER32, ORDER64):
        res, args = _lib.SIGNATURES[n]
        assert res is _lib.c_int and len(args) == 7 and args[1:4] == [_lib.c_int] * 3 and args[6] is _lib.c_int


def test_the_built_library_exports_them():
    lib = J.load()
    for n in (DRIFT, ORDER32, ORDER64):
        assert hasattr(lib, n), n
        assert getattr(lib, n).argtypes == _lib.SIGNATURES[n][1]


def test_build_trials_takes_drift():
    from jstsp19_amd.system_model import SweepParams, build_trials
    sig = inspect.signature(build_trials).parameters
    assert sig["drift"].kind is inspect.Parameter.KEYWORD_ONLY and sig["drift"].default is None
    p = SweepParams(Nt=2, Nr=8, L=2, T=4, Mr=2)
    for kw in (dict(drift=0.1), dict(drift=0.1, frame=2), dict(drift=-0.1, corr=0.5), dict(drift=float("nan"), corr=0.5),
               dict(drift=float("inf"), corr=0.5, frame=1),
               dict(drift=0.1, corr=0.5, channel=np.zeros((8, 2, 2), dtype=np.complex64))):
        with pytest.raises(ValueError):                          # refused before anything touches a device
            build_trials(p, 0, 1, **kw)


def test_support_order_is_public():
    from jstsp19_amd import solvers
    for n in ("support_order", "support_order_f64"):
        assert n in solvers.__all__ and getattr(J, n) is getattr(solvers, n)
        sig = inspect.signature(getattr(solvers, n)).parameters
        assert list(sig) == ["S", "ctx"] and sig["ctx"].kind is inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(ValueError):                              # a vector is not a (Gr, G2) matrix: refused on the Python side
        solvers.support_order(np.zeros(4, dtype=np.complex64))


def test_run_tracking_takes_drift_and_the_pai_modes():
    from jstsp19_amd import montecarlo
    from jstsp19_amd.system_model import SweepParams
    sig = inspect.signature(montecarlo.run_tracking).parameters
    assert sig["drift"].kind is inspect.Parameter.KEYWORD_ONLY and sig["drift"].default is None
    assert sig["modes"].default == ("cold", "warm", "warm_vs")
    p = SweepParams(Nt=2, Nr=8, L=2, T=4, Mr=2)
    # the argument check accepts the new modes: with one of them the call gets past it and fails on the check that follows
    for mode in ("pai", "pai_prev", "warm_pai_prev"):
        with pytest.raises(ValueError, match="drift must be"):
            montecarlo.run_tracking(p, 2, 3, 0.5, modes=(mode,), drift=-1.0)
    with pytest.raises(ValueError, match="warm_pai_prev"):
        montecarlo.run_tracking(p, 2, 3, 0.5, modes=("hot",))
    with pytest.raises(ValueError, match="modes"):
        montecarlo.run_tracking(p, 2, 3, 0.5, modes=("cold", "hot"), drift=0.1)
    for bad in (float("nan"), float("inf"), -0.5):
        with pytest.raises(ValueError, match="drift"):
            montecarlo.run_tracking(p, 2, 3, 0.5, drift=bad)
