"""tests/resume_ref.py - the state-carrying float64 restatement that the resumed solvers are tested against - and the public
surface of the resumed float64 entries without a GPU.

1. From the zero state it equals oracle/solvers.py proposed_algorithm on the committed small goldens, to the agreement the
   oracle's own two forms have there (tests/test_oracle.py: S, Y 1e-9 of max|ref|, convergence_error 1e-8 relative, the same
   Inf pattern).
2. Split a + b equals whole a + b to 0 ulp: the restatement carries nothing but the state.
3. The symbols are declared, exported and bound; jstsp_admm_state_elems counts 4 N M + 2 Gr G2; the Python names check their
   arguments before any device work and raise without a GPU (no fallback)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import resume_ref as R
from conftest import load_golden, rel_err
from oracle import solvers as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(g):
    return (g["subY"], g["Omega"], g["A"], g["B"]), (float(g["tau_Y"]), float(g["tau_Z"]), float(g["rho"]))


def _same(a, b):
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()           # 0 ulp, NaN and Inf included


@pytest.mark.parametrize("name,Imax", [("proposed_small", 20), ("proposed_refnative", 12)])
@pytest.mark.parametrize("typ,angles", [("approximate", False), ("approximate", True), ("std", False), ("std", True)])
def test_from_zero_it_is_the_oracle(name, Imax, typ, angles):
    g = load_golden(name)
    mats, prm = _args(g)
    N, Gr = g["A"].shape
    G2, M = g["B"].shape
    assert N >= Gr and M >= G2                                            # K2 of full column rank: 'std' is a least-squares solve
    ix = g["indx_S"] if angles else None
    So, Yo, ceo = O.proposed_algorithm(*mats, Imax, *prm, typ, indx_S=ix)
    S, Y, ce, state = R.solve(*mats, Imax, *prm, typ, indx_S=ix)
    assert rel_err(S, So) < 1e-9 and rel_err(Y, Yo) < 1e-9
    fin = np.isfinite(ceo)
    assert np.array_equal(fin, np.isfinite(ce)) and np.array_equal(np.isinf(ceo), np.isinf(ce))
    np.testing.assert_allclose(ce[fin], ceo[fin], rtol=1e-8, atol=1e-300)
    if typ == "approximate":
        assert np.isinf(ce[0, 2])                                         # :51 with v_prev = 0
    else:
        assert np.all(ce[:, 2] == 0)
    assert state.shape == (R.state_elems(N, M, Gr, G2),)
    assert np.array_equal(R.unpack_state(state, N, M, Gr, G2)[5], S)


@pytest.mark.parametrize("typ,angles", [("approximate", False), ("approximate", True), ("std", False), ("std", True)])
@pytest.mark.parametrize("legs", [(1, 5), (2, 4), (3, 1, 2), (7, 6)])
def test_split_equals_whole_to_the_bit(typ, angles, legs):
    g = load_golden("proposed_refnative")
    mats, prm = _args(g)
    ix = g["indx_S"] if angles else None
    whole = R.solve(*mats, sum(legs), *prm, typ, indx_S=ix)
    state, it0, rows = None, 0, []
    for n in legs:
        S, Y, ce, state = R.solve(*mats, n, *prm, typ, indx_S=ix, state=state, it0=it0)
        rows.append(ce)
        it0 += n
    _same((S, Y, np.concatenate(rows), state), whole)
    if angles:                                                            # it0 matters: the mask of the second leg restarts without it
        S0 = R.solve(*mats, legs[0], *prm, typ, indx_S=ix)[3]
        assert not np.array_equal(R.solve(*mats, legs[1], *prm, typ, indx_S=ix, state=S0, it0=0)[0],
                                  R.solve(*mats, legs[1], *prm, typ, indx_S=ix, state=S0, it0=legs[0])[0])


def test_first_row_of_a_resumed_leg_and_a_state_with_v_zero():
    g = load_golden("proposed_small")
    mats, prm = _args(g)
    N, Gr = g["A"].shape
    G2, M = g["B"].shape
    st = R.solve(*mats, 3, *prm)[3]
    ce = R.solve(*mats, 2, *prm, state=st, it0=3)[2]
    assert np.all(np.isfinite(ce))                                        # v != 0: row 1, column 3 is finite
    X, V1, V2, Cm, V, S = R.unpack_state(st, N, M, Gr, G2)
    ce0 = R.solve(*mats, 2, *prm, state=R.pack_state(X, V1, V2, Cm, 0 * V, S), it0=3)[2]
    assert np.isinf(ce0[0, 2]) and np.all(np.isfinite(ce0[1:]))           # v = 0 with X != 0: Inf as proposed_algorithm.m:51


# ---- the public surface without a GPU ----------------------------------------------------------------------------------------
def _declaration(name):
    h = open(os.path.join(ROOT, "include", "jstsp.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, h)
    assert m, "%s is not declared in include/jstsp.h" % name
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


@pytest.mark.parametrize("name,sibling", [("jstsp_proposed_resume_f64", "jstsp_proposed_algorithm_f64"),
                                          ("jstsp_proposed_std_resume_f64", "jstsp_proposed_std_f64")])
def test_the_symbols_are_declared_exported_and_their_prototypes_match(name, sibling):
    import jstsp19_amd as J
    from jstsp19_amd import _lib
    args, sib = _declaration(name), _declaration(sibling)
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names == [a.split()[-1].lstrip("*") for a in sib[:-1]] + ["it0", "state_in", "state_out", "memspace"]
    assert args[-3].startswith("const jstsp_c64") and args[-2].startswith("jstsp_c64") and args[-4] == "int it0"
    res, proto = _lib.SIGNATURES[name]
    assert res is C.c_int and len(proto) == len(args)
    for a, p in zip(args, proto):
        if "*" in a:
            assert p in (C.c_void_p, _lib.c_dp), a
        elif a.startswith("long long"):
            assert p is C.c_longlong, a
        else:
            assert a.startswith("int ") and p is C.c_int, a
    assert hasattr(J.load(), name)


def test_state_elems():
    import jstsp19_amd as J
    lib = J.load()
    for shp in ((32, 140, 32, 16), (72, 80, 24, 20), (1, 1, 1, 1), (512, 8192, 64, 4096)):
        N, M, Gr, G2 = shp
        assert lib.jstsp_admm_state_elems(*shp) == 4 * N * M + 2 * Gr * G2 == J.admm_state_elems(*shp) == R.state_elems(*shp)
    assert lib.jstsp_admm_state_elems(46341, 46341, 46341, 46341) == 6 * 46341 ** 2          # beyond 2^31: size_t, no int overflow
    for shp in ((0, 4, 4, 4), (4, -1, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0)):
        assert lib.jstsp_admm_state_elems(*shp) == 0


def test_the_python_names_their_signatures_and_argument_checks():
    import jstsp19_amd as J
    from jstsp19_amd import montecarlo, solvers
    for n in ("proposed_algorithm_resume_f64", "proposed_algorithm_std_resume_f64", "admm_state_elems"):
        assert callable(getattr(J, n)) and n in solvers.__all__
    for f, sib in ((J.proposed_algorithm_resume_f64, J.proposed_algorithm_f64), (J.proposed_algorithm_std_resume_f64, J.proposed_algorithm_std_f64)):
        p, ps = inspect.signature(f).parameters, inspect.signature(sib).parameters
        assert [k for k in ps if k != "info"] == list(p)[:-3] and list(p)[-3:] == ["state", "it0", "return_state"]
        for k, d in (("state", None), ("it0", 0), ("return_state", True)):
            assert p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is d
    assert inspect.signature(montecarlo.run_approx_sweep).parameters["resume"].default is False
    A, B, K, Om = np.zeros((6, 3), complex), np.zeros((4, 8), complex), np.zeros((6, 8), complex), np.ones((6, 8))
    ne = J.admm_state_elems(6, 8, 3, 4)
    for f in (J.proposed_algorithm_resume_f64, J.proposed_algorithm_std_resume_f64):
        with pytest.raises(ValueError):
            f(K, Om, A, B, 3, 0.1, 0.1, 0.5, it0=2)                                   # it0 without a state
        with pytest.raises(ValueError):
            f(K, Om, A, B, 3, 0.1, 0.1, 0.5, state=np.zeros((1, ne), complex), it0=-1)
        with pytest.raises(ValueError):
            f(K, Om, A, B, 3, 0.1, 0.1, 0.5, state=np.zeros((1, ne + 1), complex))
        with pytest.raises(ValueError):
            f(np.stack([K, K]), np.stack([Om, Om]), A, B, 3, 0.1, 0.1, 0.5, state=np.zeros((1, ne), complex))
        with pytest.raises(ValueError):
            f(K, np.ones((6, 7)), A, B, 3, 0.1, 0.1, 0.5)
    with pytest.raises(ValueError):
        J.proposed_algorithm_resume_f64(K, Om, A, B, 3, 0.1, 0.1, 0.5, "std")
    from jstsp19_amd.system_model import TrainingParams
    with pytest.raises(ValueError):
        montecarlo.run_approx_sweep(TrainingParams(), [0.0], [10], 1, resume=True, device="cpu")       # resume is the float64 sweep's


def test_the_fp32_entry_and_its_python_names():
    import jstsp19_amd as J
    from jstsp19_amd import _lib, solvers
    args, sib = _declaration("jstsp_proposed_resume_c32"), _declaration("jstsp_proposed_algorithm_c32")
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names == [a.split()[-1].lstrip("*") for a in sib[:-1]] + ["it0", "state_in", "state_out", "memspace"]
    assert args[-3].startswith("const jstsp_c32") and args[-2].startswith("jstsp_c32")
    assert len(_lib.SIGNATURES["jstsp_proposed_resume_c32"][1]) == len(args) and hasattr(J.load(), "jstsp_proposed_resume_c32")
    for n, sibn in (("proposed_algorithm_resume", "proposed_algorithm"), ("proposed_algorithm_angles_resume", "proposed_algorithm_angles")):
        assert callable(getattr(J, n)) and n in solvers.__all__
        p, ps = inspect.signature(getattr(J, n)).parameters, inspect.signature(getattr(J, sibn)).parameters
        assert list(ps) == list(p)[:-3] and list(p)[-3:] == ["state", "it0", "return_state"]
    A, B, K, Om = np.zeros((6, 3), np.complex64), np.zeros((4, 8), np.complex64), np.zeros((6, 8), np.complex64), np.ones((6, 8), np.float32)
    with pytest.raises(ValueError):
        J.proposed_algorithm_resume(K, Om, A, B, 3, 0.1, 0.1, 0.5, it0=2)
    with pytest.raises(ValueError):
        J.proposed_algorithm_resume(K, Om, A, B, 3, 0.1, 0.1, 0.5, state=np.zeros((1, 7), np.complex64))


def test_they_raise_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import jstsp19_amd as J
    rng = np.random.default_rng(0)
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    A, B, K, Om = c(6, 3), c(4, 8), c(6, 8), np.ones((6, 8))
    st = np.zeros((1, J.admm_state_elems(6, 8, 3, 4)), complex)
    for f in (lambda: J.proposed_algorithm_resume_f64(K, Om, A, B, 3, 0.1, 0.1, 0.5),
              lambda: J.proposed_algorithm_resume_f64(K, Om, A, B, 3, 0.1, 0.1, 0.5, state=st, it0=4),
              lambda: J.proposed_algorithm_std_resume_f64(K, Om, A, B, 3, 0.1, 0.1, 0.5, state=st, it0=4, return_state=False)):
        with pytest.raises(J.JstspError):
            f()
