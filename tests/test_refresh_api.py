"""The public surface of the refreshed support without a GPU: jstsp_support_top_f64 and jstsp_proposed_refresh_f64 in the header,
the ctypes table and the built library; support_top_f64 and proposed_algorithm_refresh_f64 exported with their signatures; what the
Python side refuses before anything touches a device; the chunking estimate unchanged for the entries that were there; and the
new modes of run_tracking."""
import inspect
import os
import re

import numpy as np
import pytest

import jstsp19_amd as J
from jstsp19_amd import _lib, solvers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP, REFRESH = "jstsp_support_top_f64", "jstsp_proposed_refresh_f64"


def _prototype(name):
    h = open(os.path.join(ROOT, "include", "jstsp.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, h)
    assert m, "no prototype of %s" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")], h[:m.start()].rsplit("/*", 1)[1], h


def test_header_declares_the_two_entries():
    args, doc, h = _prototype(TOP)
    assert args == ["jstsp_ctx *ctx", "int Gr", "int G2", "int batch", "const double *V", "int count", "int32_t *indx_top", "int memspace"]
    assert re.search(r"#define\s+JSTSP_SUPPORT_TOP_MAX\s+4096\b", h)
    assert "tests/test_gpu_support_top.py" in doc and "JSTSP_E_ARG" in doc
    args, doc, _ = _prototype(REFRESH)
    assert args[12:20] == ["int Imax", "const double *tau_Y", "const double *tau_S", "const double *rho", "const int32_t *indx_S", "int n_indx",
                           "int refresh_start", "int refresh_period"]
    assert args[20:] == ["jstsp_c64 *S_out", "jstsp_c64 *Y_out", "double *ce_out", "int it0", "const jstsp_c64 *state_in",
                         "jstsp_c64 *state_out", "int32_t *indx_out", "int memspace"]
    assert "tests/test_gpu_refresh64.py" in doc and "818" in doc and "JSTSP_E_ARG" in doc


def test_signature_table_and_library_have_them():
    lib = J.load()
    assert _lib.SUPPORT_TOP_MAX == 4096
    res, args = _lib.SIGNATURES[TOP]
    assert res is _lib.c_int and [a is _lib.c_int for a in args] == [False, True, True, True, False, True, False, True]
    res, args = _lib.SIGNATURES[REFRESH]
    sib = _lib.SIGNATURES["jstsp_proposed_resume_f64"][1]
    assert res is _lib.c_int and len(args) == 28
    # the resumed entry's list without `type`, with n_indx, start, period after indx_S and indx_out before memspace
    assert args[:16] == sib[:16] and args[16] is sib[17] and args[17:20] == [_lib.c_int] * 3 and args[20:26] == sib[18:24]
    assert args[26] is _lib.c_void_p and args[27] is _lib.c_int
    for n in (TOP, REFRESH):
        assert hasattr(lib, n) and getattr(lib, n).argtypes == _lib.SIGNATURES[n][1]


def test_the_functions_are_public():
    for n in ("support_top_f64", "proposed_algorithm_refresh_f64"):
        assert n in solvers.__all__ and getattr(J, n) is getattr(solvers, n)
    sig = inspect.signature(solvers.support_top_f64).parameters
    assert list(sig) == ["S", "count", "ctx"] and sig["ctx"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(solvers.proposed_algorithm_refresh_f64).parameters
    assert list(sig) == ["subY", "Omega", "A", "B", "Imax", "tau_Y", "tau_S", "rho", "start", "period", "indx_S", "want_ce", "ctx", "state",
                         "it0", "return_state"]
    for name, default in (("start", 0), ("period", 1), ("indx_S", None), ("want_ce", True), ("ctx", None), ("state", None), ("it0", 0),
                          ("return_state", True)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default, name


def test_python_side_refusals_come_before_the_device():
    rng = np.random.default_rng(0)
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    subY, Om, A, B = c(2, 6, 7), np.ones((2, 6, 7)), c(6, 4), c(3, 7)          # batch 2, g = 12
    f = lambda **kw: solvers.proposed_algorithm_refresh_f64(subY, Om, A, B, 3, 0.1, 0.1, 0.5, **kw)
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
        f(it0=-1, state=np.zeros((2, solvers.admm_state_elems(6, 7, 4, 3)), complex))
    with pytest.raises(ValueError, match="state"):
        f(it0=1, state=np.zeros((2, 5), complex))


def test_the_chunking_estimate_of_the_other_entries_is_unchanged():
    sig = inspect.signature(solvers._f64_admm_bytes).parameters
    assert list(sig) == ["N", "M", "Gr", "G2", "sA", "sB", "std", "own_PA", "own_PB", "host", "resumed", "refresh"]
    assert sig["refresh"].kind is inspect.Parameter.KEYWORD_ONLY and sig["refresh"].default is False
    f = solvers._f64_admm_bytes
    assert f(32, 140, 32, 16, 0, 2240, False, True, True, True, True) == 1891328
    assert f(64, 64, 64, 512, 0, 0, False, True, True, False, False) == 5046272
    assert f(72, 80, 24, 20, 1728, 1600, True, True, False, True, False) == 2892800
    # the new entry: the rank array (4 bytes an entry), and for a host call the staged order in and the staged list out
    dev = f(64, 64, 64, 512, 0, 0, False, True, True, False, True, refresh=True) - f(64, 64, 64, 512, 0, 0, False, True, True, False, True)
    host = f(64, 64, 64, 512, 0, 0, False, True, True, True, True, refresh=True) - f(64, 64, 64, 512, 0, 0, False, True, True, True, True)
    assert dev == 4 * 32768 and host == dev + 4 * (32768 + 4096)


def test_run_tracking_takes_the_refresh_modes_and_their_keyword():
    from jstsp19_amd import montecarlo
    from jstsp19_amd.system_model import SweepParams
    sig = inspect.signature(montecarlo.run_tracking).parameters
    assert sig["refresh"].kind is inspect.Parameter.KEYWORD_ONLY and tuple(sig["refresh"].default) == (0, 1)
    modes = ("refresh", "warm_refresh", "pai_prev_refresh")
    assert montecarlo.TRACKING_PAI_MODES[:3] == ("pai", "pai_prev", "warm_pai_prev") and montecarlo.TRACKING_PAI_MODES[-3:] == modes
    p = SweepParams(Nt=2, Nr=8, L=2, T=4, Mr=2)
    # the argument check accepts the new modes: with one of them the call gets past it and fails on the check that follows
    for mode in modes:
        with pytest.raises(ValueError, match="drift must be"):
            montecarlo.run_tracking(p, 2, 3, 0.5, modes=(mode,), drift=-1.0)
        with pytest.raises(ValueError, match="precision must be 'f64'"):
            montecarlo.run_tracking(p, 2, 3, 0.5, modes=("cold", mode), precision="f32")
    with pytest.raises(ValueError, match="pai_prev_refresh"):
        montecarlo.run_tracking(p, 2, 3, 0.5, modes=("hot",))
    for bad in ((-1, 0), (0, -2), 3, (1, 1, 1), ("a", 1), None):
        with pytest.raises(ValueError, match="refresh"):
            montecarlo.run_tracking(p, 2, 3, 0.5, modes=("refresh",), refresh=bad)


def test_the_tool_takes_the_flag():
    src = open(os.path.join(ROOT, "tools", "run_tracking.py")).read()
    assert '"--refresh"' in src and "START,PERIOD" in src
    for mode in ("refresh", "warm_refresh", "pai_prev_refresh"):
        assert '"%s"' % mode in src
