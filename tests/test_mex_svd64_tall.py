"""The MEX commands 'svd_tall_f64' and 'lowrank_tall_f64' (mex/jstsp_mex.cpp) driven through the stand-in MEX API
(tests/mex_stub/): bad calls are refused before the library is touched (no GPU needed), and on the GPU [U,S,V] = svd_tall_f64(A)
and lowrank_tall_f64(A, R) on a 3 x 200 x 2 array reproduce the bits of the Python wrappers, with S the diagonal matrix of
svd(A,'econ')."""
import os

import numpy as np
import pytest

from test_mex_gateway import MexError, call, mex  # noqa: F401  (mex: the compiled gateway, a module-scoped fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def test_bad_calls_are_refused_before_the_library_and_the_wrappers_name_their_commands(mex):  # noqa: F811
    A = _c(np.random.default_rng(1), 3, 200)
    for args, nlhs in ((("svd_tall_f64",), 1), (("svd_tall_f64", A, 2, 3), 1), (("svd_tall_f64", A), 6), (("svd_tall_f64", A, 0), 3),
                       (("svd_tall_f64", A, 4), 3), (("lowrank_tall_f64", A), 1), (("lowrank_tall_f64", A, 1, 1), 1),
                       (("lowrank_tall_f64", A, 1), 3), (("lowrank_tall_f64", A, 0), 1), (("lowrank_tall_f64", A, 4), 1)):
        with pytest.raises(MexError) as e:
            call(mex, nlhs, *args)
        assert e.value.ident == "jstsp:args", (args[0], str(e.value))
        if len(args) == 3 and args[2] in (0, 4):
            assert args[0] in str(e.value)                                   # the message names the command that was called
    for f, cmd in (("svd_tall_f64.m", "'svd_tall_f64'"), ("lowrank_tall_f64.m", "'lowrank_tall_f64'")):
        assert cmd in open(os.path.join(ROOT, "mex", f)).read()


@pytest.mark.gpu
def test_svd_and_lowrank_reproduce_the_python_wrappers_bits(mex):  # noqa: F811
    import jstsp19_amd as J
    A = _c(np.random.default_rng(2), 3, 200, 2) * 0.3                       # rows x cols x pages
    Ab = np.ascontiguousarray(np.moveaxis(A, 2, 0))                          # (batch, rows, cols) for the Python wrapper
    Up, sp, Vp, rkp, cvp = J.svd_tall_f64(Ab, info=True)
    U, S, V, rk, cv = call(mex, 5, "svd_tall_f64", A)
    assert U.shape == (3, 3, 2) and S.shape == (3, 3, 2) and V.shape == (200, 3, 2) and rk.shape == (2, 1) and rk.dtype == np.int32
    for t in range(2):
        assert np.array_equal(U[:, :, t], Up[t]) and np.array_equal(V[:, :, t], Vp[t])
        assert np.array_equal(np.diag(S[:, :, t]), sp[t]) and np.count_nonzero(S[:, :, t] - np.diag(np.diag(S[:, :, t]))) == 0      # S is diagonal
        assert np.linalg.norm(A[:, :, t] - U[:, :, t] @ S[:, :, t] @ np.conj(V[:, :, t].T), 2) <= 1e-13 * sp[t, 0]
    assert np.array_equal(rk[:, 0], rkp) and np.array_equal(cv[:, 0], cvp) and np.all(rkp == 3) and np.all(cvp == 1)
    s, = call(mex, 1, "svd_tall_f64", A)                                     # one output: the column of values
    assert s.shape == (3, 1, 2) and np.array_equal(s[:, 0, :].T, sp)
    U2, S2, V2 = call(mex, 3, "svd_tall_f64", A[:, :, 0], 2)                 # 2-D, n_keep
    assert U2.shape == (3, 2) and S2.shape == (2, 2) and V2.shape == (200, 2)
    assert np.array_equal(U2, Up[0][:, :2]) and np.array_equal(np.diag(S2), sp[0][:2]) and np.array_equal(V2, Vp[0][:, :2])
    Xp, tp = J.lowrank_tall_f64(Ab, 2, info=True)
    X, tail = call(mex, 2, "lowrank_tall_f64", A, 2)
    assert X.shape == (3, 200, 2) and tail.shape == (2, 1)
    assert np.array_equal(np.moveaxis(X, 2, 0), Xp) and np.array_equal(tail[:, 0], tp) and np.array_equal(tp, sp[:, 2])
    X1, = call(mex, 1, "lowrank_tall_f64", A[:, :, 1].real, 3)               # a real matrix is widened
    assert np.array_equal(X1, J.lowrank_tall_f64(A[:, :, 1].real, 3))
