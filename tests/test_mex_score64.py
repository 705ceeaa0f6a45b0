"""The MEX commands 'nmse_spectral_f64' and 'rate_f64' (mex/jstsp_mex.cpp) driven through the stand-in MEX API (tests/mex_stub/):
bad calls are refused before the library is touched (no GPU needed), and on the GPU the two commands on a 32 x 16 x 3 array
(pages = batch) reproduce the bits of the Python wrappers."""
import os

import numpy as np
import pytest

from test_mex_gateway import MexError, call, mex  # noqa: F401  (mex: the compiled gateway, a module-scoped fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def test_bad_calls_are_refused_before_the_library_and_the_wrappers_name_their_commands(mex):  # noqa: F811
    Z = _c(np.random.default_rng(1), 4, 6)
    for args, nlhs in ((("nmse_spectral_f64",), 1), (("nmse_spectral_f64", Z), 1), (("nmse_spectral_f64", Z, Z, 0.1), 1), (("nmse_spectral_f64", Z, Z), 2),
                       (("rate_f64", Z, Z), 1), (("rate_f64", Z, Z, 0.1, 1), 1), (("rate_f64", Z, Z, 0.1), 2), (("rate_f64", Z, Z, -1.0), 1),
                       (("rate_f64", Z, Z, float("nan")), 1)):
        with pytest.raises(MexError) as e:
            call(mex, nlhs, *args)
        assert e.value.ident == "jstsp:args", (args[0], str(e.value))
    for args in (("nmse_spectral_f64", Z, Z[:3]), ("rate_f64", Z, np.stack([Z, Z], axis=2), 0.1)):
        with pytest.raises(MexError) as e:
            call(mex, 1, *args)
        assert e.value.ident == "jstsp:shape", (args[0], str(e.value))
    for f, cmd in (("nmse_spectral_f64.m", "'nmse_spectral_f64'"), ("rate_f64.m", "'rate_f64'")):
        assert cmd in open(os.path.join(ROOT, "mex", f)).read()


@pytest.mark.gpu
def test_the_two_commands_reproduce_the_python_wrappers_bits(mex):  # noqa: F811
    import jstsp19_amd as J
    rng = np.random.default_rng(2)
    Z = _c(rng, 32, 16, 3) * 0.3                                             # rows x cols x pages
    S = Z + 1e-3 * _c(rng, 32, 16, 3)
    Zb, Sb = (np.ascontiguousarray(np.moveaxis(x, 2, 0)) for x in (Z, S))    # (batch, rows, cols) for the Python wrappers
    e, = call(mex, 1, "nmse_spectral_f64", S, Z)
    assert e.shape == (3, 1) and e.dtype == np.float64 and np.array_equal(e[:, 0], J.nmse_spectral_f64(Sb, Zb))
    r, = call(mex, 1, "rate_f64", S, Z, 0.1)
    assert r.shape == (3, 1) and np.array_equal(r[:, 0], J.rate_f64(Sb, Zb, 0.1))
    e1, = call(mex, 1, "nmse_spectral_f64", S[:, :, 1], Z[:, :, 1])          # 2-D
    assert e1.shape == (1, 1) and e1[0, 0] == e[1, 0]
    er, = call(mex, 1, "nmse_spectral_f64", 3 * Z[:, :, 0].real, Z[:, :, 0].real)     # real matrices are widened
    assert er[0, 0] == 1.0
