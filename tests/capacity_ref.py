"""Float64 restatement of plot_capacity.m / plot_ee.m (TEST INFRASTRUCTURE): the 'quantized' codebooks of
createBeamformer.m, the ASE of one realisation in the literal Mr x Mr determinant form and in the Sylvester / Cholesky form,
and a numpy Monte-Carlo run of panel points with the reference's own samplers (oracle/system_model.py)."""
from __future__ import annotations

import numpy as np

from oracle import system_model as OS

NT, L, T, CLUSTERS, RAYS = 16, 4, 5, 2, 3
NOISE_VAR = 10 ** (-15 / 10)
SCALE = 1.0 / (NOISE_VAR * NT)


def create_beamformer(N, kind):
    """createBeamformer.m:1-35 for 'ZC', 'fft', 'ps' and 'quantized' / 'quantized_4' (:18-31):
    A = vec(kron(ones(K,1), 0:2^Nq-1)).', K = ceil(N/2^Nq), so each phase index repeats K times in a row."""
    if kind not in ("quantized", "quantized_4"):
        return OS.create_beamformer(N, kind)
    nq = 4 if kind == "quantized_4" else 6
    K = int(np.ceil(N / 2 ** nq))
    A = np.kron(np.ones((K, 1)), np.arange(2 ** nq)[None, :]).reshape(-1, order="F")      # vec(): column-major
    omega = 2 * np.pi / 2 ** nq * A[:N]
    return np.exp(-1j * np.arange(N)[:, None] * omega[None, :]) / np.sqrt(N)


def ase_det(Y, Wc, scale=SCALE):
    """plot_capacity.m:47 as written: real(log2(det(eye(Mr) + scale * Wc'*(Y*Y')*Wc)))."""
    M = np.eye(Wc.shape[1]) + scale * (Wc.conj().T @ (Y @ Y.conj().T) @ Wc)
    return float(np.real(np.log2(np.linalg.det(M))))


def ase_chol(Y, Wc, scale=SCALE):
    """The same value on the smaller side (Sylvester: det(I + c P P^H) = det(I + c P^H P), P = Wc' Y) by Cholesky."""
    P = Wc.conj().T @ Y
    G = np.eye(P.shape[1]) + scale * (P.conj().T @ P) if P.shape[0] >= P.shape[1] else np.eye(P.shape[0]) + scale * (P @ P.conj().T)
    return float(2 * np.sum(np.log2(np.real(np.diag(np.linalg.cholesky(G))))))


def received(H, pilot_sym):
    """hbf.m:12-18 with N = 0: Y = sum_l H_l Psi_bar_l, Psi_bar_l(k, :) = row l of toeplitz(s_k).
    H: (Nr, Nt, L) or the (Nr, Nt*L) matrix [H_1 .. H_L]; pilot_sym: (Nt, T)."""
    Nt, Tf = pilot_sym.shape
    if H.ndim == 2:
        H = H.reshape(H.shape[0], Nt, -1, order="F")
    Y = np.zeros((H.shape[0], Tf), complex)
    for l in range(H.shape[2]):
        Psi = np.stack([OS.toeplitz_rows(pilot_sym[k], l + 1)[l] for k in range(Nt)])
        Y += H[:, :, l] @ Psi
    return Y


def designs_ase(Y, Nr, Mr, ind, W_zc, W_q, scale=SCALE):
    """The four designs of plot_capacity.m:44-64 on one Y: DBF, HBF-PS, HBF-ZC, proposed (ind: 0-based columns)."""
    return [ase_chol(Y, W_zc, scale), ase_chol(Y, W_q[:, :Mr], scale), ase_chol(Y, W_zc[:, :Mr], scale),
            ase_chol(Y, W_q[:, ind], scale)]


def power_model(Nr, Mr, Mr_e):
    """plot_ee.m:69-77 as written."""
    Pcirc, Psw, Pps, Plna, Pps_zc = 0, 0.005, 0.015, 0.02, 0.06
    return [Pcirc + Nr * Nr * Plna + Nr * (Nr + 1) * Pps_zc, Pcirc + Mr * Nr * Plna + Nr * (Mr + 1) * Pps,
            Pcirc + Mr * Nr * Plna + Nr * (Mr + 1) * Pps_zc, Pcirc + Mr_e * Nr * Plna + Mr_e * Psw + Nr * (Mr_e + 1) * Pps]


def monte_carlo(Nr, Mr_e, Mr, n_trials, rng):
    """plot_capacity.m:35-66 at one point with numpy draws from the reference's samplers: wideband_mmwave_channel (:36),
    qam4mod pilots (:37-41), randperm(Mr_e) (:63).  Returns (n_trials, 4) float64 ASE."""
    W_zc, W_q = create_beamformer(Nr, "ZC"), create_beamformer(Nr, "quantized")
    alphabet = OS.qam4_alphabet()
    Np = CLUSTERS * RAYS
    out = np.empty((n_trials, 4))
    for r in range(n_trials):
        gains = (rng.standard_normal((L, Np)) + 1j * rng.standard_normal((L, Np))) / np.sqrt(2)
        u_r, u_t = rng.random((L, Np)), rng.random((L, Np))
        H = OS.wideband_mmwave_channel(L, Nr, NT, CLUSTERS, RAYS, Nr, NT, gains, u_r, u_t)[0]
        s = alphabet[rng.integers(0, 4, size=(NT, T))]
        Y = received(H, s)
        out[r] = designs_ase(Y, Nr, Mr, rng.permutation(Mr_e)[:Mr], W_zc, W_q)
    return out
