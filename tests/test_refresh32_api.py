"""The public surface of the fp32 refreshed support without a GPU: jstsp_support_top_c32, jstsp_proposed_refresh_c32 and
jstsp_proposed_refresh_c64 in the header, the ctypes table and the built library; support_top and proposed_algorithm_refresh
exported with their signatures; what the Python side refuses before anything touches a device; run_tracking's refresh_f32 and the
tool's flag."""
import inspect
import os
import re

import numpy as np
import pytest

import jstsp19_amd as J
from jstsp19_amd import _lib, solvers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP, REFRESH, REFRESH64 = "jstsp_support_top_c32", "jstsp_proposed_refresh_c32", "jstsp_proposed_refresh_c64"


def _prototype(name):
    h = open(os.path.join(ROOT, "include", "jstsp.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, h)
    assert m, "no prototype of %s" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")], h[:m.start()].rsplit("/*", 1)[1]


def test_header_declares_the_three_entries():
    args, doc = _prototype(TOP)
    assert args == ["jstsp_ctx *ctx", "int Gr", "int G2", "int batch", "const jstsp_c32 *S", "int count", "int32_t *indx_top", "int memspace"]
    assert "tests/test_gpu_support_top32.py" in doc and "jstsp_support_order_c32" in doc and "32 KiB" in doc
    for name, cx, re_t in ((REFRESH, "jstsp_c32", "float"), (REFRESH64, "jstsp_c64", "double")):
        args, doc = _prototype(name)
        assert args[6:8] == ["const %s *subY" % cx, "const %s *Omega" % re_t]
        assert args[12:21] == ["int Imax", "const double *tau_Y", "const double *tau_S", "const double *rho", "int type", "const int32_t *indx_S",
                               "int n_indx", "int refresh_start", "int refresh_period"]
        assert args[21:] == ["%s *S_out" % cx, "%s *Y_out" % cx, "double *ce_out", "int it0", "const %s *state_in" % cx, "%s *state_out" % cx,
                             "int32_t *indx_out", "int memspace"]
        assert "tests/test_gpu_refresh32.py" in doc and "JSTSP_E_UNSUPPORTED" in doc and "JSTSP_E_ARG" in doc


def test_signature_table_and_library_have_them():
    lib = J.load()
    assert _lib.SIGNATURES[TOP] == _lib.SIGNATURES["jstsp_support_top_f64"]
    sib = _lib.SIGNATURES["jstsp_proposed_resume_c32"][1]
    for n in (REFRESH, REFRESH64):
        res, args = _lib.SIGNATURES[n]
        assert res is _lib.c_int and len(args) == 29
        # the resumed entry's list with n_indx, start, period after indx_S and indx_out before memspace
        assert args[:18] == sib[:18] and args[18:21] == [_lib.c_int] * 3 and args[21:27] == sib[18:24]
        assert args[27] is _lib.c_void_p and args[28] is _lib.c_int
    for n in (TOP, REFRESH, REFRESH64):
        assert hasattr(lib, n) and getattr(lib, n).argtypes == _lib.SIGNATURES[n][1]


def test_the_functions_are_public():
    for n in ("support_top", "proposed_algorithm_refresh"):
        assert n in solvers.__all__ and getattr(J, n) is getattr(solvers, n)
    sig = inspect.signature(solvers.support_top).parameters
    assert list(sig) == ["S", "count", "ctx"] and sig["ctx"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(solvers.proposed_algorithm_refresh).parameters
    assert list(sig) == list(inspect.signature(solvers.proposed_algorithm_refresh_f64).parameters)
    assert list(sig) == ["subY", "Omega", "A", "B", "Imax", "tau_Y", "tau_S", "rho", "start", "period", "indx_S", "want_ce", "ctx", "state",
                         "it0", "return_state"]
    for name, default in (("start", 0), ("period", 1), ("indx_S", None), ("want_ce", True), ("ctx", None), ("state", None), ("it0", 0),
                          ("return_state", True)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default, name


def test_python_side_refusals_come_before_the_device():
    rng = np.random.default_rng(0)
    c = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)
    subY, Om, A, B = c(2, 6, 7), np.ones((2, 6, 7), np.float32), c(6, 4), c(3, 7)          # batch 2, g = 12
    f = lambda **kw: solvers.proposed_algorithm_refresh(subY, Om, A, B, 3, 0.1, 0.1, 0.5, **kw)
    for kw in (dict(start=-1), dict(period=-1), dict(start=-2, period=0)):
        with pytest.raises(ValueError, match="start and period"):
            f(**kw)
    for bad in (np.zeros((2, 13), np.int32), np.zeros((2, 0), np.int32), np.zeros((3, 4), np.int32), np.zeros(5, np.int32),
                np.zeros((), np.int32)):
        with pytest.raises(ValueError, match="indx_S"):
            f(indx_S=bad)
    with pytest.raises(ValueError, match="it0"):
        f(it0=2)
    with pytest.raises(ValueError, match="it0"):
        f(it0=-1, state=np.zeros((2, solvers.admm_state_elems(6, 7, 4, 3)), np.complex64))
    with pytest.raises(ValueError, match="state"):
        f(it0=1, state=np.zeros((2, 5), np.complex64))


class _Reached(Exception):
    pass


def test_run_tracking_takes_refresh_f32(monkeypatch):
    from jstsp19_amd import montecarlo

    def reached(*a, **kw):
        raise _Reached()
    monkeypatch.setattr(montecarlo, "build_trials", reached)    # the first thing run_tracking does after its argument checks
    from jstsp19_amd.system_model import SweepParams
    sig = inspect.signature(montecarlo.run_tracking).parameters
    assert sig["refresh_f32"].kind is inspect.Parameter.KEYWORD_ONLY and sig["refresh_f32"].default is False
    p = SweepParams(Nt=2, Nr=8, L=2, T=4, Mr=2)
    for mode in ("refresh", "warm_refresh", "pai_prev_refresh"):
        # the default keeps the refusal, word for word
        with pytest.raises(ValueError, match=re.escape("refresh the support inside the float64 solver: precision must be 'f64'")):
            montecarlo.run_tracking(p, 2, 3, 0.5, modes=("cold", mode), precision="f32")
        # with the keyword the call gets past every argument check
        with pytest.raises(_Reached):
            montecarlo.run_tracking(p, 2, 3, 0.5, modes=(mode,), precision="f32", refresh_f32=True, device="cpu")
    for modes in (("refresh",), ("cold",)):                     # the keyword belongs to the fp32 solver
        with pytest.raises(ValueError, match="refresh_f32"):
            montecarlo.run_tracking(p, 2, 3, 0.5, modes=modes, precision="f64", refresh_f32=True)


def test_the_tool_takes_the_flag():
    src = open(os.path.join(ROOT, "tools", "run_tracking.py")).read()
    assert '"--refresh-f32"' in src and 'kw["refresh_f32"] = True' in src
