"""CPU tier of the plot_rankR.m restatement (tests/rank_ref.py): the receive signal is proposed_hbf.m's, the parameter sets
are the figure's, and on the reference's own samplers in float64 the spectrum drops to rounding level right after
min(Np, L*Nt) - the statement of the figure that the device sweep is later held to."""
import numpy as np
import pytest

import capacity_ref as C
import rank_ref as R
from oracle import system_model as OS

# sigma_{r+1} / sigma_1 of the float64 restatement, r = min(Np, L*Nt, Nr, T): the largest value over 20 realisations of each of
# the 18 points was 2.05e-16 (measured once with numpy's SVD; the values lie between 1.3e-16 and 2.1e-16 at every point).
TAIL_MEASURED = 2.05e-16


def test_received_is_proposed_hbf():
    rng = np.random.default_rng(3)
    Nr, Nt, L, Tf = 8, 3, 4, 10
    H = rng.standard_normal((Nr, Nt, L)) + 1j * rng.standard_normal((Nr, Nt, L))
    s = rng.standard_normal((Nt, Tf)) + 1j * rng.standard_normal((Nt, Tf))
    Y = R.received(H, s)
    # the oracle's proposed_hbf on the same operands (rows 1..L of each Toeplitz matrix), noise-free
    rows = np.stack([OS.toeplitz_rows(s[k], L) for k in range(Nt)], axis=2)
    W = OS.create_beamformer(Nr, "ZC")
    omega = np.tile(np.arange(2), (Tf, 1))
    Yo = OS.proposed_hbf(H, np.zeros((Nr, Tf), complex), rows, Tf, Nr, 2, W, omega)[4]
    assert np.max(np.abs(Y - Yo)) <= 1e-13 * np.max(np.abs(Yo))
    # the (Nr, Nt*L) layout of jstsp_build_trials_c32's H, and the capacity restatement of the same sum
    H2 = H.reshape(Nr, Nt * L, order="F")
    assert np.array_equal(R.received(H2, s), Y)
    assert np.max(np.abs(C.received(H2, s) - Y)) <= 1e-13 * np.max(np.abs(Y))
    # by hand: column j of Y is sum over l, k of H(:, k, l) * toeplitz(s_k)(l, j)
    j = 2
    col = sum(H[:, k, l] * (s[k, j - l] if j >= l else np.conj(s[k, l - j])) for l in range(L) for k in range(Nt))
    assert np.max(np.abs(Y[:, j] - col)) <= 1e-13 * np.max(np.abs(col))


def test_rank_points_are_the_reference_panels():
    from jstsp19_amd import montecarlo as M
    assert sorted(M.RANK_PANELS) == [1, 2, 3, 4, 5, 6] and M.RANK_PANELS == R.PANELS
    want = {1: (32, 2, 3), 2: (64, 2, 3), 3: (128, 2, 3), 4: (32, 3, 12), 5: (64, 3, 12), 6: (128, 3, 12)}
    for panel, (Nr, clusters, rays) in want.items():
        pts = M.rank_points(panel)
        assert [p.L for p in pts] == [1, 4, 8]
        assert all((p.Nr, p.clusters, p.rays, p.Nt, p.Mr_e, p.Mr, p.T_prop, p.Gr, p.Gt) == (Nr, clusters, rays, 4, 32, 4, 50, Nr, 4)
                   for p in pts)
        assert all(min(p.Nr, p.Mr_e) == 32 for p in pts)
    assert "rank_points" in M.__all__ and "run_rank" in M.__all__


def test_spectrum_and_rank_bound():
    rng = np.random.default_rng(1)
    A = rng.standard_normal((6, 3)) + 1j * rng.standard_normal((6, 3))
    Y = A @ (rng.standard_normal((3, 9)) + 1j * rng.standard_normal((3, 9)))
    s = R.spectrum(Y)
    assert s.shape == (6,) and np.all(np.diff(s) <= 0) and s[3] < 1e-14 * s[0] < s[2]
    assert np.array_equal(R.spectrum(Y, 2), s[:2])
    assert R.rank_bound(6, 1) == 4 and R.rank_bound(6, 8) == 6 and R.rank_bound(36, 4) == 16
    assert R.rank_bound(36, 8) == 32 and R.rank_bound(36, 8, Nr=32) == 32 and R.rank_bound(36, 16, Nr=128) == 36
    assert R.rank_bound(100, 30) == 50                                                   # capped by T


@pytest.mark.parametrize("panel", [1, 2, 3, 4, 5, 6])
def test_spectrum_drops_to_rounding_level_after_the_rank_bound(panel):
    """The restatement only: index r + 1 of the float64 spectrum against sigma_1, r = min(Np, L*Nt, Nr, T), at 100 x the level
    measured above.  (Panel 4 at L = 8 has r = 32 = Nr: Y has no 33rd singular value, the statement is empty there.)"""
    Nr, clusters, rays = R.PANELS[panel]
    rng = np.random.default_rng(20190913 + panel)
    for L in R.L_RANGE:
        r = R.rank_bound(clusters * rays, L, Nr=Nr)
        for _ in range(5):
            s = R.spectrum(R.realisation(Nr, L, clusters, rays, rng))
            assert s.shape == (min(Nr, R.T),)
            tail = s[r] / s[0] if r < s.size else 0.0
            assert tail < 100 * TAIL_MEASURED, (panel, L, r, tail)
            if L == 1:
                assert s[r - 1] > 1e-9 * s[0], (panel, L, r, s[r - 1] / s[0])           # ... and, with one tap, not before it


def test_monte_carlo_shape():
    m = R.monte_carlo(1, 2, np.random.default_rng(0))
    assert m.shape == (3, 32) and np.all(np.diff(m, axis=1) <= 0) and np.all(m[:, 0] > 0)
