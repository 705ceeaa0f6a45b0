"""CPU tier: the builders of tests/spectrum_problems.py do what they say, and the chunked-QR route restated in numpy
(qr(vstack([R, chunk]), mode='r') with chunks of 128 rows) stays within the cap of the GPU test on the six problems: measured
3e-16 .. 9e-16 of sigma_1, against the 1e-10 fixed beforehand (no Gram route meets it: sqrt(eps) = 1.5e-8 on the rank-deficient
cases)."""
import numpy as np

import spectrum_problems as P

CAP = 1e-10


def test_builders():
    rng = np.random.default_rng(1)
    q = P.orth(rng, 40, 7)
    assert np.allclose(q.conj().T @ q, np.eye(7), atol=1e-14)
    sigma = np.array([3.0, 2.0, 0.5, 1e-6])
    Y = P.usv(rng, 30, 50, sigma)
    assert Y.shape == (30, 50) and Y.dtype == np.complex128
    s = P.ref(Y)
    assert np.allclose(s[:4], sigma, rtol=1e-9) and np.all(s[4:] < 1e-14)
    assert P.err(s, s) == 0.0 and abs(P.err(s + 3e-3, s) - 1e-3) < 1e-12
    assert P.ordered(s) and not P.ordered(s[::-1]) and not P.ordered(-s)
    g = P.graded(64, 3.0)
    assert g[0] == 3.0 and abs(g[-1] / g[0] - 1e-12) < 1e-24
    for name, Ys in P.conditioning_cases(rng, 64, 100):
        assert Ys.shape == (2, 64, 100), name
    assert np.linalg.matrix_rank(P.conditioning_cases(rng, 64, 100)[0][1][0], tol=1e-9) == 6
    Y32 = P.rand(rng, 5, 9).astype(np.complex64)
    assert np.array_equal(P.ref(Y32), np.linalg.svd(Y32.astype(np.complex128), compute_uv=False))     # the values the device saw


def test_chunked_qr_route_in_numpy_meets_the_cap():
    rng = np.random.default_rng(2)
    cases = P.cpu_cases(rng)
    assert len(cases) == 6
    for name, Y in cases:
        e = P.err(P.chunked_qr_values(Y), P.ref(Y))
        print("chunked QR %s: %.3g" % (name, e))
        assert e < CAP, (name, e)
    # the adjoint orientation and a ragged last chunk
    Y = P.rand(rng, 33, 300)
    assert np.array_equal(P.chunked_qr_values(Y), P.chunked_qr_values(Y.conj().T))
    assert P.err(P.chunked_qr_values(Y, chunk=64), P.ref(Y)) < CAP
    assert np.array_equal(P.chunked_qr_values(np.zeros((40, 7))), np.zeros(7))
