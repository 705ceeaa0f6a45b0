"""tests/tracking_ref.py, the float64 restatement of the tracked channel's gain recursion, against the closed form the library
evaluates (include/jstsp.h: jstsp_build_trials_tracked_c32) - no GPU."""
import numpy as np
import pytest

import tracking_ref as R

CORRS = (0.0, 0.3, 0.5, 0.8, 0.95, 0.999, 1.0)


def _innovations(frames, shape=(3, 5), seed=7):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((frames,) + shape) + 1j * rng.standard_normal((frames,) + shape)) / np.sqrt(2.0)


@pytest.mark.parametrize("corr", CORRS)
def test_recursion_equals_closed_form(corr):
    w = _innovations(41)
    g = R.gains_recursion(w, corr)
    assert g.shape == w.shape and g.dtype == np.complex128
    for f in (0, 1, 2, 5, 17, 40):
        c = R.gains_closed_form(w, corr, f)
        assert np.max(np.abs(g[f] - c)) <= 1e-14, (corr, f)
        np.testing.assert_array_equal(R.gain_at(w, corr, f), g[f])


@pytest.mark.parametrize("corr", CORRS)
@pytest.mark.parametrize("frame", [0, 1, 2, 5, 100, 65535])
def test_coefficients_keep_the_variance(corr, frame):
    """corr^(2f) + (1 - corr^2) sum_{k=1..f} corr^(2(f-k)) = 1: every frame has the variance of a drawn gain."""
    c = R.coefficients(corr, frame)
    assert c.shape == (frame + 1,)
    assert abs(float(np.sum(c * c)) - 1.0) <= 1e-12


def test_exact_cases():
    """frame 0 is w_0 for any corr, corr = 1 keeps w_0 at every frame, corr = 0 returns w_f - on the bits."""
    w = _innovations(6)
    for corr in CORRS:
        np.testing.assert_array_equal(R.gains_recursion(w, corr)[0], w[0])
        np.testing.assert_array_equal(R.gains_closed_form(w, corr, 0), w[0])
    for f in range(6):
        np.testing.assert_array_equal(R.gains_recursion(w, 1.0)[f], w[0])
        np.testing.assert_array_equal(R.gains_closed_form(w, 1.0, f), w[0])
        np.testing.assert_array_equal(R.gains_recursion(w, 0.0)[f], w[f])
        np.testing.assert_array_equal(R.gains_closed_form(w, 0.0, f), w[f])


def test_lag_correlation_of_the_model():
    """E[g_f conj(g_{f-k})] = corr^k from the coefficients alone (unit-variance, independent innovations)."""
    corr = 0.8
    for f, k in ((1, 1), (3, 2), (3, 3), (9, 4)):
        a, b = R.coefficients(corr, f), R.coefficients(corr, f - k)
        assert abs(float(np.sum(a[:f - k + 1] * b)) - corr ** k) <= 1e-14


def test_real_innovations_and_bad_corr():
    w = np.arange(12, dtype=np.float32).reshape(4, 3)
    g = R.gains_recursion(w, 0.5)
    assert g.dtype == np.float64
    np.testing.assert_allclose(g[3], R.gains_closed_form(w, 0.5, 3), rtol=1e-14)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            R.gains_recursion(w, bad)
