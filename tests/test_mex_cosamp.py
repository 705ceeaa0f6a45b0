"""The gateway's "CoSaMP" command (mex/CoSaMP.m: x = CoSaMP(Phi, y, K), plot_time_comparisions.m:96) returns what the _c64
entry returns, unbatched and with pages."""
import numpy as np
import pytest

from test_mex_gateway import call, mex  # noqa: F401


@pytest.mark.gpu
def test_gateway_cosamp_returns_what_the_c64_entry_returns(mex):  # noqa: F811
    import jstsp19_amd as J
    rng = np.random.default_rng(8)
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    meas, size_d, K, nb = 60, 90, 5, 3
    Phi = c(meas, size_d) / np.sqrt(meas)
    X0 = np.zeros((size_d, nb), complex)
    for t in range(nb):
        X0[rng.choice(size_d, K, replace=False), t] = 2 * c(K)
    Y = Phi @ X0 + 0.01 * c(meas, nb)
    xs, info = J.cosamp(Phi, Y.T.copy(), K, info=True)                     # the library's defaults, as CoSaMP.m runs them
    (x,) = call(mex, 1, "CoSaMP", Phi, Y[:, 0], K)
    assert x.shape == (size_d, 1) and np.array_equal(x[:, 0], xs[0])
    x, sup, it, rs, st = call(mex, 5, "CoSaMP", Phi, Y, K)
    assert x.shape == (size_d, nb) and np.array_equal(x.T, xs)
    assert np.array_equal(sup.T, info["support"]) and np.array_equal(it.reshape(-1), info["iters"])
    assert np.array_equal(rs.reshape(-1), info["resid"]) and not st.any()
    x7, _, it7, _, _ = call(mex, 5, "CoSaMP", np.stack([Phi] * nb, axis=2), Y, K, 2, 0.0)   # pages of Phi; iters, tol given
    assert list(it7.reshape(-1)) == [2] * nb and np.array_equal(x7.T, J.cosamp(Phi, Y.T.copy(), K, iters=2, tol=0.0))
