"""CPU tier of the capacity / EE restatement (tests/capacity_ref.py): the two ASE forms agree, the 'quantized' codebook keeps
the reference's construction, and the power model is plot_ee.m's."""
import numpy as np
import pytest

import capacity_ref as R


def _rand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@pytest.mark.parametrize("Nr,T,Mr", [(32, 5, 1), (32, 5, 4), (32, 5, 5), (64, 5, 22), (128, 5, 128), (16, 20, 7)])
def test_det_and_sylvester_cholesky_forms_agree(Nr, T, Mr):
    rng = np.random.default_rng(Nr * 100 + Mr)
    Y = _rand(rng, Nr, T) * 0.3
    W = R.create_beamformer(Nr, "ZC")[:, :Mr] if Mr <= Nr else None
    a, b = R.ase_det(Y, W), R.ase_chol(Y, W)
    assert abs(a - b) <= 1e-10 * max(1.0, abs(a))


def test_quantized_codebook_facts():
    W64 = R.create_beamformer(64, "quantized")
    assert np.max(np.abs(W64 - np.fft.fft(np.eye(64)) / 8)) < 1e-13              # the unitary DFT at N = 64
    W128 = R.create_beamformer(128, "quantized")
    assert np.array_equal(W128[:, 0::2], W128[:, 1::2])                            # identical pairs of columns at N = 128
    assert len({tuple(np.round(W128[:, k], 12)) for k in range(32)}) == 16         # 32 columns, 16 distinct beams
    W32 = R.create_beamformer(32, "quantized")
    assert np.allclose(W32, W64[:32, :32] * np.sqrt(64 / 32))                       # the first 32 of the 64 phases
    assert abs(np.max(np.abs(W32.conj().T @ W32 - np.eye(32))) - 0.64) < 0.01       # not orthogonal
    W4 = R.create_beamformer(40, "quantized_4")                                     # N_q = 4, K = 3
    ph = np.round(np.angle(W4[1] * np.sqrt(40)) / (-2 * np.pi / 16)) % 16
    assert list(ph[:7]) == [0, 0, 0, 1, 1, 1, 2]


def test_power_model_hand_values():
    # plot_ee.m:69-77 at Nr = 64, Mr_e = 32: Nr^2 Plna + Nr (Nr+1) Pps_zc = 81.92 + 249.6
    assert R.power_model(64, 1, 32) == pytest.approx([331.52, 1.28 + 1.92, 1.28 + 7.68, 40.96 + 0.16 + 31.68], abs=1e-9)
    assert R.power_model(64, 31, 32)[1] == pytest.approx(31 * 64 * 0.02 + 64 * 32 * 0.015, abs=1e-9)
    from jstsp19_amd import montecarlo as M
    for Mr in range(1, 33, 3):
        assert M.power_model(64, Mr, 32) == pytest.approx(R.power_model(64, Mr, 32), rel=1e-15)


def test_capacity_points_are_the_reference_panels():
    from jstsp19_amd import montecarlo as M
    for panel, (Nr, Mr_e) in {1: (32, 32), 2: (64, 32), 3: (128, 64)}.items():
        pts = M.capacity_points(panel)
        assert [p.Mr for p in pts] == list(range(1, 33, 3))
        assert all((p.Nr, p.Mr_e, p.Nt, p.L, p.T_prop, p.clusters, p.rays) == (Nr, Mr_e, 16, 4, 5, 2, 3) for p in pts)
        assert pts[0].noise_var == pytest.approx(10 ** -1.5)
        d = M.capacity_designs(pts[3])
        assert d == [("ZC", Nr, 0), ("quantized", 10, 0), ("ZC", 10, 0), ("quantized", 10, Mr_e)]
