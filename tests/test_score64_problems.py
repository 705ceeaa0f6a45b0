"""The float64 reference of tests/score64_problems.py pinned on closed-form cases (no GPU): _score_f64's two formulas."""
import numpy as np

import score64_problems as P


def _z(seed=1, batch=3, rows=6, cols=9):
    return P.rand(np.random.default_rng(seed), batch, rows, cols)


def test_equal_operands_give_zero_and_a_zero_estimate_gives_one():
    Z = _z()
    assert np.array_equal(P.ref_nmse(Z, Z), np.zeros(3))
    assert np.array_equal(P.ref_nmse(np.zeros_like(Z), Z), np.ones(3))


def test_three_times_zbar_is_four_raw_and_one_capped():
    Z = _z(2)
    for t in range(3):
        assert abs(P.ref_e(3 * Z[t], Z[t]) - 4.0) < 1e-14
    assert np.array_equal(P.ref_nmse(3 * Z, Z), np.ones(3))


def test_a_nan_stays_a_nan_and_the_zero_zbar_is_zero_over_zero():
    Z = _z(3)
    S = Z.copy()
    S[1, 2, 3] = np.nan
    e = P.ref_nmse(S, Z)
    assert np.isnan(e[1]) and e[0] == 0.0 and e[2] == 0.0
    assert np.isnan(P.ref_nmse(np.zeros_like(Z), np.zeros_like(Z))).all()
    assert np.array_equal(P.ref_nmse(Z, np.zeros_like(Z)), np.ones(3))         # x / 0 = Inf, capped


def test_the_rate_of_a_diagonal_zbar_in_closed_form():
    sigma = np.array([3.0, 2.0, 0.5, 0.0])
    Z = np.zeros((1, 4, 6), complex)
    Z[0, np.arange(4), np.arange(4)] = sigma * np.exp(1j * np.arange(4))
    for S, e in ((Z, 0.0), (3 * Z, 4.0), (np.zeros_like(Z), 1.0)):
        want = sum(np.log2(1.0 + s * s / (4 * (0.1 + e))) for s in sigma)
        assert abs(P.ref_rate(S, Z, 0.1)[0] - want) < 1e-13 * want
        assert abs(P.rate_from_sigma(sigma, 4, 0.1, e) - want) < 1e-13 * want


def test_the_rate_divides_by_the_rows_of_zbar_in_either_orientation():
    Z = _z(4, 2, 5, 11)
    Zh = np.ascontiguousarray(np.conj(np.swapaxes(Z, 1, 2)))
    S, Sh = 1.5 * Z, 1.5 * Zh
    for t in range(2):
        sig = np.linalg.svd(Z[t], compute_uv=False)
        e = P.ref_e(S[t], Z[t])
        assert abs(P.ref_rate(S, Z, 0.1)[t] - P.rate_from_sigma(sig, 5, 0.1, e)) < 1e-12      # det(I + c Z Z') over 5 rows
        assert abs(P.ref_rate(Sh, Zh, 0.1)[t] - P.rate_from_sigma(sig, 11, 0.1, e)) < 1e-12   # = det(I + c Z' Z), c with 11 rows
    assert not np.allclose(P.ref_rate(S, Z, 0.1), P.ref_rate(Sh, Zh, 0.1))


def test_the_shapes_cover_every_route_and_relative_error_uses_tiny():
    assert {P.route(*s) for s in P.LDS_SHAPES} == {"lds"} and {P.route(*s) for s in P.QR_SHAPES} == {"qr"}
    assert {P.route(*s) for s in P.GLOBAL_SHAPES} == {"global"}
    assert P.rel([0.0, 1.0], [0.0, 1.0]) == 0.0 and P.rel([P.TINY], [0.0]) == 1.0
