"""proposed_algorithm_until_f64 and the *_until modes of run_tracking without a GPU: what is refused before any device call, the
prototype of the C entry, and the chunking estimate of the new entry."""
import ctypes as C

import numpy as np
import pytest

from jstsp19_amd import _lib, solvers
from jstsp19_amd.montecarlo import TRACKING_UNTIL_MODES, run_tracking
from jstsp19_amd.system_model import SweepParams


def _problem():
    rng = np.random.default_rng(5)
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    return c(2, 6, 7), np.ones((2, 6, 7)), c(6, 4), c(3, 7)                    # batch 2, g = 12


def test_arguments_are_refused_before_any_device_call():
    f = lambda **kw: solvers.proposed_algorithm_until_f64(*_problem(), 3, 0.1, 0.1, 0.5, **{"tol": 1e-3, **kw})
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
    with pytest.raises(ValueError, match="state"):
        f(it0=1, state=np.zeros((2, 5), complex))
    with pytest.raises(TypeError):
        solvers.proposed_algorithm_until_f64(*_problem(), 3, 0.1, 0.1, 0.5)    # tol is required


def test_the_prototype_is_the_refreshed_entrys_with_the_rule():
    res, args = _lib.SIGNATURES["jstsp_proposed_until_f64"]
    sib = _lib.SIGNATURES["jstsp_proposed_refresh_f64"][1]
    assert res is C.c_int and len(args) == len(sib) + 5
    assert args[:20] == sib[:20] and args[23:-3] == sib[20:-1] and args[-1] is C.c_int
    assert args[20:23] == [C.POINTER(C.c_double), C.c_int, C.c_int] and args[-3:-1] == [C.c_void_p, C.c_void_p]


def test_the_chunking_estimate_covers_the_shadow_set():
    sib = lambda host, sA=0, sB=0: solvers._f64_admm_bytes(64, 64, 64, 512, sA, sB, False, True, True, host, True, refresh=True)
    new = lambda host, sA=0, sB=0: solvers._f64_until_bytes(64, 64, 64, 512, sA, sB, host)
    nm, g = 64 * 64, 64 * 512
    assert new(True) - sib(True) == 16 * (5 * nm + 2 * g) + 24 * nm + 4 * g + 8 * 4096 + 1024
    assert new(False) - new(True) - (sib(False) - sib(True)) == 24 * nm                        # a device call: two buffers for subY, Omega
    assert new(True, 0, g) - sib(True, 0, g) - (new(True) - sib(True)) == 16 * (512 * 64 + 512 * 512)


def test_the_until_modes_of_run_tracking_are_refused_without_a_rule_and_in_fp32():
    p = SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4, snr_db=5.0)
    assert TRACKING_UNTIL_MODES == ("cold_until", "warm_until", "refresh_until", "warm_refresh_until")
    with pytest.raises(ValueError, match="precision must be 'f64'"):
        run_tracking(p, 2, 2, 0.9, modes=("warm_until",), precision="f32", stop=(1e-4, 2))
    with pytest.raises(ValueError, match="need stop"):
        run_tracking(p, 2, 2, 0.9, modes=("cold_until",))
    for bad in ((0.0, 2), (1e-4, 0), ("x", 2), -1.0):
        with pytest.raises(ValueError, match="stop"):
            run_tracking(p, 2, 2, 0.9, modes=("cold_until",), stop=bad)
