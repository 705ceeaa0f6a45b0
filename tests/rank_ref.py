"""Float64 restatement of plot_rankR.m (TEST INFRASTRUCTURE): the noise-free receive signal of proposed_hbf.m:15-20 from a
channel and pilot symbols, its singular values by numpy's SVD, the rank bound the figure marks, and a numpy run of the
figure's points with the reference's own samplers (oracle/system_model.py)."""
from __future__ import annotations

import numpy as np

from oracle import system_model as OS

NT, T, MR_E, L_RANGE = 4, 50, 32, (1, 4, 8)
# (Nr, clusters, rays) of the six panels (plot_rankR.m:9-19, :70-80, :128-138, :189-199, :251-261, :313-323)
PANELS = {1: (32, 2, 3), 2: (64, 2, 3), 3: (128, 2, 3), 4: (32, 3, 12), 5: (64, 3, 12), 6: (128, 3, 12)}


def received(H, pilot_sym):
    """proposed_hbf.m:15-20 with N = 0: ``Psi_bar(k,:,l) = Psi_i(l,:,k)`` (row l of toeplitz(s_k), plot_rankR.m:34),
    ``Y = sum_l H(:,:,l)*Psi_bar(:,:,l)``.  H: (Nr, Nt, L) or the (Nr, Nt*L) matrix [H_1 .. H_L]; pilot_sym: (Nt, T)."""
    Nt, Tf = pilot_sym.shape
    if H.ndim == 2:
        H = H.reshape(H.shape[0], Nt, -1, order="F")
    L = H.shape[2]
    Psi_i = np.stack([OS.toeplitz_matlab(pilot_sym[k]) for k in range(Nt)], axis=2)       # (T, T, Nt)
    Psi_bar = np.zeros((Nt, Tf, L), complex)
    Y = np.zeros((H.shape[0], Tf), complex)
    for l in range(L):
        for k in range(Nt):
            Psi_bar[k, :, l] = Psi_i[l, :, k]
        Y = Y + H[:, :, l] @ Psi_bar[:, :, l]
    return Y


def spectrum(Y, n_keep=None):
    """plot_rankR.m:49-50: ``diag(S)`` of ``svd(Y)``, the first n_keep values."""
    s = np.linalg.svd(np.asarray(Y, dtype=np.complex128), compute_uv=False)
    return s if n_keep is None else s[:n_keep]


def rank_bound(Np, L, Nt=NT, Nr=None, Tf=T):
    """``min(Np, L*Nt)`` (plot_rankR.m:61), capped by the size of Y: the number of non-zero singular values at most."""
    r = min(Np, L * Nt, Tf)
    return r if Nr is None else min(r, Nr)


def realisation(Nr, L, clusters, rays, rng, Nt=NT, Tf=T):
    """plot_rankR.m:26-41 at one point with numpy draws from the reference's samplers: wideband_mmwave_channel (:26), one
    4-QAM sequence per transmit antenna (:33).  Returns the float64 (Nr, T) noise-free Y."""
    Np = clusters * rays
    gains = (rng.standard_normal((L, Np)) + 1j * rng.standard_normal((L, Np))) / np.sqrt(2)
    u_r, u_t = rng.random((L, Np)), rng.random((L, Np))
    H = OS.wideband_mmwave_channel(L, Nr, Nt, clusters, rays, Nr, Nt, gains, u_r, u_t)[0]
    s = OS.qam4_alphabet()[rng.integers(0, 4, size=(Nt, Tf))]
    return received(H, s)


def monte_carlo(panel, n_trials, rng, n_keep=MR_E):
    """The three curves of one panel averaged over n_trials realisations: (3, n_keep)."""
    Nr, clusters, rays = PANELS[panel]
    return np.array([np.mean([spectrum(realisation(Nr, L, clusters, rays, rng), n_keep) for _ in range(n_trials)], axis=0)
                     for L in L_RANGE])
