"""proposed_algorithm_until (fp32) and run_tracking(until_f32=True) without a GPU: the prototype of the C entries and what is refused
before any device call."""
import ctypes as C

import numpy as np
import pytest

import jstsp19_amd
from jstsp19_amd import _lib, solvers
from jstsp19_amd.montecarlo import run_tracking
from jstsp19_amd.system_model import SweepParams


def _problem():
    rng = np.random.default_rng(5)
    c = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)
    return c(2, 6, 7), np.ones((2, 6, 7), np.float32), c(6, 4), c(3, 7)       # batch 2, g = 12


def test_the_prototype_is_the_refreshed_entrys_with_the_rule():
    sib = _lib.SIGNATURES["jstsp_proposed_refresh_c32"][1]
    for name in ("jstsp_proposed_until_c32", "jstsp_proposed_until_c64"):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(sib) + 5
        assert args[:21] == sib[:21] and args[24:-3] == sib[21:-1] and args[-1] is C.c_int
        assert args[21:24] == [C.POINTER(C.c_double), C.c_int, C.c_int] and args[-3:-1] == [C.c_void_p, C.c_void_p]
        assert args[16] is C.c_int                              # `type` after rho, as in the sibling
    assert hasattr(C.CDLL(_lib.LIB_PATH), "jstsp_proposed_until_c32")
    assert jstsp19_amd.proposed_algorithm_until is solvers.proposed_algorithm_until
    assert solvers.UNTIL_CHECK_F32 >= 1


def test_arguments_are_refused_before_any_device_call():
    f = lambda **kw: solvers.proposed_algorithm_until(*_problem(), 3, 0.1, 0.1, 0.5, **{"tol": 1e-3, **kw})
    for kw in (dict(min_iters=0), dict(check=0), dict(min_iters=-2, check=-1)):
        with pytest.raises(ValueError, match="min_iters and check"):
            f(**kw)
    with pytest.raises(ValueError, match="approximate"):
        f(type="std")
    for kw in (dict(refresh=(-1, 1)), dict(refresh=(0, -1))):
        with pytest.raises(ValueError, match="start and period"):
            f(**kw)
    with pytest.raises(ValueError, match="indx_S"):
        f(indx_S=np.zeros((2, 13), np.int32))
    with pytest.raises(ValueError, match="it0"):
        f(it0=2)
    with pytest.raises(ValueError, match="tol"):
        f(tol=(1e-3, 1e-3, 1e-3))
    with pytest.raises(TypeError):
        solvers.proposed_algorithm_until(*_problem(), 3, 0.1, 0.1, 0.5)       # tol is required


def test_until_f32_needs_the_fp32_precision_and_a_rule():
    p = SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4, snr_db=5.0)
    with pytest.raises(ValueError, match="until_f32 .* precision must be 'f32'"):
        run_tracking(p, 2, 2, 0.9, modes=("cold_until",), stop=(1e-4, 2), until_f32=True)
    with pytest.raises(ValueError, match="until_f32 needs stop"):
        run_tracking(p, 2, 2, 0.9, modes=("cold_until",), precision="f32", until_f32=True)
    with pytest.raises(ValueError, match="precision must be 'f64'"):        # opt-in: stop= alone still refuses the modes in fp32
        run_tracking(p, 2, 2, 0.9, modes=("cold_until",), precision="f32", stop=(1e-4, 2))
    for bad in ((0.0, 2), (1e-4, 0)):
        with pytest.raises(ValueError, match="stop"):
            run_tracking(p, 2, 2, 0.9, modes=("cold_until",), precision="f32", stop=bad, until_f32=True)
