"""refit_f64 and run_tracking(refit=...): what the Python side refuses, before anything touches a device (no GPU here: a call that
got as far as the library would raise JstspError, not ValueError)."""
import numpy as np
import pytest

import jstsp19_amd as J
from jstsp19_amd import _lib, montecarlo as MC
from jstsp19_amd.system_model import SweepParams

N, M, Gr, G2 = 6, 7, 5, 4
G = Gr * G2


def _args(batch=None):
    rng = np.random.default_rng(0)
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    b = () if batch is None else (batch,)
    return [c(*b, N, M), np.ones(b + (N, M)), c(N, Gr), c(G2, M), c(*b, Gr, G2)]


def test_the_entry_is_exported_and_bound():
    assert J.refit_f64 is J.solvers.refit_f64 and "refit_f64" in J.solvers.__all__
    res, args = _lib.SIGNATURES["jstsp_refit_f64"]
    assert len(args) == 23 and hasattr(J.load(), "jstsp_refit_f64")


@pytest.mark.parametrize("kw", [dict(K=0), dict(K=G + 1), dict(K=-3), dict(iters=0), dict(iters=-1), dict(lam=-1e-3), dict(lam=float("nan")),
                                dict(tol=-1.0), dict(tol=float("nan"))])
def test_bad_scalars_are_refused(kw):
    v = dict(K=3, iters=2, lam=0.0, tol=0.0)
    v.update(kw)
    with pytest.raises(ValueError):
        J.refit_f64(*_args(), v["K"], v["iters"], v["lam"], v["tol"])
    with pytest.raises(ValueError):
        J.refit_f64(*_args(2), v["K"], v["iters"], v["lam"], v["tol"])


def test_bad_shapes_are_refused():
    a = _args(2)
    for k, bad in ((4, a[4][:, :-1]), (4, a[4][0]), (4, a[4][:1]), (1, a[1][:, :-1]), (2, a[2][:-1]), (3, a[3][:, :-1])):
        b = list(a)
        b[k] = bad
        with pytest.raises(ValueError):
            J.refit_f64(*b, 3, 2)


def test_bad_support_lists_are_refused():
    a = _args(2)
    ix = np.tile(np.arange(1, G + 1, dtype=np.int32), (2, 1))
    for bad in (ix[:, :2], np.concatenate([ix, ix], axis=1), ix[:1], ix[0], ix[None]):
        with pytest.raises(ValueError):
            J.refit_f64(*a, 3, 2, indx_S=bad)
    # without a list the selection kernel's limit holds, except for K = Gr*G2
    rng = np.random.default_rng(1)
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    big = [c(4, 5), np.ones((4, 5)), c(4, 80), c(70, 5), c(80, 70)]
    with pytest.raises(ValueError, match="selection kernel"):
        J.refit_f64(*big, _lib.SUPPORT_TOP_MAX + 1, 2)


def test_run_tracking_validates_refit():
    p = SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4, snr_db=5.0)
    g = p.solver_shape[2] * p.solver_shape[3]
    for bad in (5, (5,), (5, 2, 1), ("a", 2), (0, 2), (g + 1, 2), (5, 0), (5, -1)):
        with pytest.raises(ValueError, match="refit"):
            MC.run_tracking(p, 2, 3, 0.9, imax=(3,), refit=bad)
    with pytest.raises(ValueError, match="precision must be 'f64'"):
        MC.run_tracking(p, 2, 3, 0.9, imax=(3,), precision="f32", refit=(5, 2))
    big = SweepParams(Nt=64, Nr=64, L=8, T=64, Mr=8, snr_db=5.0)
    with pytest.raises(ValueError, match="refit"):
        MC.run_tracking(big, 2, 3, 0.9, imax=(3,), refit=(4097, 2))
    # the pinned mode lists are what they were
    assert MC.TRACKING_UNTIL_MODES == ("cold_until", "warm_until", "refresh_until", "warm_refresh_until")
    assert "refit" not in MC.TRACKING_PAI_MODES + MC.TRACKING_MODES
