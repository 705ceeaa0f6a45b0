"""CPU tier of CoSaMP: the float64 restatement (tests/cosamp_ref.py), the fixture tests/golden/cosamp.npz and the promise
the GPU test leans on, and the declared surface (header, library exports, ctypes table, MEX wrapper and command)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import cosamp_problems as P  # noqa: E402
import cosamp_ref as R  # noqa: E402
from test_mex_gateway import MexError, call, mex  # noqa: E402,F401  (the gateway built against the first-party mex.h stand-in)

ENTRIES = ("jstsp_cosamp_c32", "jstsp_cosamp_c64", "jstsp_cosamp_kron_c32", "jstsp_cosamp_kron_c64")


def test_restatement_recovers_planted_signals_exactly():
    """class (a) with y formed in float64 from the complex64 dictionary and signal: support equal, x to 1e-12"""
    for g in P.groups(with_driver=False):
        if g["cls"] != "a":
            continue
        for t in range(P.n_problems(g)):
            op, x0 = P.operator(g, t), g["x0"][t].astype(np.complex128)
            r = R.cosamp(op, op.Phi @ x0, g["K"], g["iters"], g["tol"])
            assert np.array_equal(r["support"], np.nonzero(x0)[0] + 1) and r["status"] == 0
            assert np.max(np.abs(r["x"] - x0)) / np.max(np.abs(x0)) < 1e-12 and r["resid"] <= g["tol"]


def test_dense_and_kronecker_forms_of_the_restatement_agree():
    for g in P.groups(with_driver=False):
        if g["kind"] != "kron":
            continue
        for t in range(P.n_problems(g)):
            op = P.operator(g, t)
            rk = R.cosamp(op, g["y"][t], g["K"], g["iters"], g["tol"])
            rd = R.cosamp(R.Dense(np.kron(op.Bf.T, op.Af)), g["y"][t], g["K"], g["iters"], g["tol"])
            assert np.array_equal(rk["support"], rd["support"]) and rk["iters"] == rd["iters"]
            assert np.max(np.abs(rk["x"] - rd["x"])) / np.max(np.abs(rd["x"])) < 1e-12


def test_edges_of_the_restatement():
    g = P.groups(with_driver=False)[2]
    op = P.operator(g, 0)
    r = R.cosamp(op, np.zeros(op.meas), g["K"], 5, 1e-5)
    assert r["iters"] == 0 and not r["x"].any() and r["status"] == 0 and r["resid"] == 0.0
    Phi = op.Phi.copy()
    j = int(np.nonzero(g["x0"][0])[0][0])
    Phi[:, (j + 7) % op.size_d] = Phi[:, j]                  # a repeated column: both copies tie and enter T together
    r = R.cosamp(R.Dense(Phi), g["y"][0], g["K"], 5, 1e-5)
    assert r["status"] == 1 and r["iters"] == 0 and not r["x"].any() and r["resid"] == 1.0


def test_fixture_is_reproduced_from_its_seeds(golden):
    import make_cosamp_fixture as M
    z, new = golden("cosamp"), M.build()
    assert sorted(z) == sorted(new)
    for k in z:
        if k.endswith((".support", ".iters", ".status", ".decided")):
            assert np.array_equal(z[k], new[k]), k
        elif k.endswith((".beta", ".selb", ".rmin", ".dref")):
            np.testing.assert_allclose(new[k], z[k], rtol=1e-3, atol=1e-9, err_msg=k)      # functions of sigma_min: conditioned as 1 / r
        else:
            np.testing.assert_allclose(new[k], z[k], rtol=1e-8, atol=1e-9 * np.max(np.abs(z[k])), err_msg=k)


def test_fixture_keeps_the_promise_the_gpu_test_leans_on(golden):
    """a condition on the inputs, checked against the reference alone: at most 10 % of classes (a)-(c) and 40 % of class (e)
    undecided; r = sigma_min / sigma_max of every least squares >= 1e-2 for (a)-(c), >= 1e-5 for (e)"""
    z = golden("cosamp")
    abc = [k[:-8] for k in z if k.endswith(".decided") and k[0] in "abc"]
    assert len(abc) == 6
    dec = np.concatenate([z[n + ".decided"] for n in abc])
    assert np.mean(~dec) <= 0.10 and min(z[n + ".rmin"].min() for n in abc) >= 1e-2
    assert z["e_driver.decided"].size == 64 and np.mean(~z["e_driver.decided"]) <= 0.40 and z["e_driver.rmin"].min() >= 1e-5
    assert np.all(z["e_driver.status"] == 0) and all(np.all(z[n + ".status"] == 0) for n in abc)


def test_cosamp_entries_are_declared_exported_and_bound():
    from jstsp19_amd import _lib
    import jstsp19_amd
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jstsp.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % n, header), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert len(_lib.SIGNATURES["jstsp_cosamp_c32"][1]) == 16 and len(_lib.SIGNATURES["jstsp_cosamp_kron_c32"][1]) == 20
    assert callable(jstsp19_amd.cosamp) and callable(jstsp19_amd.cosamp_kron)
    m = open(os.path.join(ROOT, "mex", "CoSaMP.m")).read()
    assert re.match(r"function x = CoSaMP\(Phi, y, K\)", m) and "jstsp_mex('CoSaMP', Phi, y, K)" in m


def test_gateway_refuses_a_malformed_cosamp_call_before_touching_the_gpu(mex):  # noqa: F811
    rng = np.random.default_rng(5)
    Phi = rng.standard_normal((30, 40)) + 1j * rng.standard_normal((30, 40))
    y = Phi[:, 0] * 2.0
    with pytest.raises(MexError) as e:
        call(mex, 1, "CoSaMP", Phi, y)                                   # CoSaMP(Phi, y, K): three inputs at least
    assert e.value.ident == "jstsp:args" and "3 to 5" in str(e.value)
    with pytest.raises(MexError) as e:
        call(mex, 1, "CoSaMP", Phi, y[:7], 4)
    assert e.value.ident == "jstsp:shape"
    for K in (0, 11, 21):                                                # K < 1; 3K > measures; 2K > size_d
        with pytest.raises(MexError) as e:
            call(mex, 1, "CoSaMP", Phi, y, K)
        assert e.value.ident == "jstsp:args" and "K" in str(e.value)
    with pytest.raises(MexError) as e:
        call(mex, 6, "CoSaMP", Phi, y, 4)
    assert e.value.ident == "jstsp:args" and "output" in str(e.value)
