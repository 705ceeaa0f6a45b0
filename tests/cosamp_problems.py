"""Seeded CoSaMP problems (CPU only).  Every input is complex64, and the float64 reference (tests/cosamp_ref.py) runs
on exactly those values widened, so the device and the reference solve the same problem.

A group is a dict: name, cls ('a' noiseless exactly K-sparse, 'b' the same with noise, 'c' Kronecker factors, 'e' the
driver's own problem), kind ('dense' | 'kron'), K, iters, tol, the dictionary (Phi, or Af and Bf; 2-D = shared by the
group's problems, 3-D = one per problem), y (n x measures) and, for 'a', the planted x0 (n x size_d); for 'e' Zbar.
The edges of class (d) - u = 0, 2K = size_d, a repeated column, 2^+-40 scaling - are derived from these in the tests."""
import numpy as np

from oracle import solvers as O
from oracle import system_model as sm

import cosamp_ref as R

ITERS, TOL = 12, 1e-5
E_TRIALS, E_ITERS, E_K = 64, 4, 100


def _c(rng, *s):
    return (rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2)


def _planted(rng, n, size_d, K):
    x = np.zeros((n, size_d), np.complex128)
    for t in range(n):
        at = rng.choice(size_d, K, replace=False)
        x[t, at] = (1 + rng.random(K)) * np.exp(2j * np.pi * rng.random(K))
    return x.astype(np.complex64)


def _gauss(name, cls, seed, meas, size_d, K, n, noise, own):
    rng = np.random.default_rng(seed)
    Phi = (_c(rng, n, meas, size_d) if own else _c(rng, meas, size_d)) / np.sqrt(meas)
    Phi = Phi.astype(np.complex64)
    x0 = _planted(rng, n, size_d, K)
    P64 = Phi.astype(np.complex128)
    y = np.stack([(P64[t] if own else P64) @ x0[t].astype(np.complex128) for t in range(n)])
    y = y + noise * _c(rng, n, meas) * np.linalg.norm(y, axis=1, keepdims=True) / np.sqrt(meas)
    return dict(name=name, cls=cls, kind="dense", K=K, iters=ITERS, tol=TOL, Phi=Phi, y=y.astype(np.complex64), x0=x0)


def _kron(name, seed, N, M, Gr, G2, K, n, own):
    rng = np.random.default_rng(seed)
    Af = ((_c(rng, n, N, Gr) if own else _c(rng, N, Gr)) / np.sqrt(N)).astype(np.complex64)
    Bf = ((_c(rng, n, G2, M) if own else _c(rng, G2, M)) / np.sqrt(M)).astype(np.complex64)
    x0 = _planted(rng, n, Gr * G2, K)
    y = np.stack([R.Kron(Af[t] if own else Af, Bf[t] if own else Bf).cols(np.arange(Gr * G2)) @ x0[t].astype(np.complex128)
                  for t in range(n)])
    y = y + 1e-2 * _c(rng, n, N * M) * np.linalg.norm(y, axis=1, keepdims=True) / np.sqrt(N * M)
    return dict(name=name, cls="c", kind="kron", K=K, iters=ITERS, tol=TOL, Af=Af, Bf=Bf, y=y.astype(np.complex64), x0=x0)


# plot_time_comparisions.m:8-25
DRIVER = dict(Nt=4, Nr=32, Mr_e=32, Gr=32, Gt=4, clusters=2, rays=3, L=4, Mr=4, T=35, noise_var=10 ** (-5 / 10))
T_HBF = int(round(DRIVER["T"] / (DRIVER["Nr"] / DRIVER["Mr"]))) * DRIVER["Nt"]          # :22


def driver_trial(seed):
    """plot_time_comparisions.m:54-75 for one seed: (A, Gb = B*B', y = vec(Y_hbf*B'), Zbar), float64."""
    p = DRIVER
    rng = np.random.default_rng(seed)
    d = sm.draw_trial(rng, p)
    H, Zbar, _, _, Dr, Dt = sm.wideband_mmwave_channel(p["L"], p["Nr"], p["Nt"], p["clusters"], p["rays"], p["Gr"], p["Gt"],
                                                       d["gains"], d["u_r"], d["u_t"])
    Psi_rows = np.stack([sm.toeplitz_rows(sm.qam4_alphabet()[d["qam_idx"][k]], p["L"]) for k in range(p["Nt"])], axis=2)
    Nn = np.sqrt(p["noise_var"] / 2) * d["noise"]
    Yc, Wc, Psi_bar, _ = sm.hbf(H, Nn[:, :T_HBF], Psi_rows[:, :T_HBF, :], T_HBF, p["Nr"], sm.create_beamformer(p["Nr"], "ZC"))   # :68
    A = Wc.conj().T @ Dr                                                                    # :69
    B = np.concatenate([Dt.conj().T @ Psi_bar[:, :, l] for l in range(p["L"])])             # :70-73
    return A, B @ B.conj().T, O.vec(Yc @ B.conj().T), Zbar                                  # :74-75


def _driver(n=E_TRIALS):
    tr = [driver_trial(7000 + t) for t in range(n)]
    return dict(name="e_driver", cls="e", kind="kron", K=E_K, iters=E_ITERS, tol=TOL,
                Af=np.stack([t[0] for t in tr]).astype(np.complex64), Bf=np.stack([t[1] for t in tr]).astype(np.complex64),
                y=np.stack([t[2] for t in tr]).astype(np.complex64), Zbar=np.stack([t[3] for t in tr]))


def groups(with_driver=True):
    g = [_gauss("a_shared", "a", 101, 128, 256, 8, 16, 0.0, False),
         _gauss("a_own", "a", 102, 96, 192, 6, 5, 0.0, True),
         _gauss("b_shared", "b", 103, 128, 256, 8, 16, 1e-2, False),
         _gauss("b_own", "b", 104, 96, 192, 6, 5, 1e-2, True),
         _kron("c_shared", 105, 12, 14, 10, 16, 6, 8, False),
         _kron("c_own", 106, 12, 14, 10, 16, 6, 3, True)]
    if with_driver:
        g.append(_driver())
    return g


def operator(g, t):
    pick = lambda a: a[t] if a.ndim == 3 else a
    return R.Dense(pick(g["Phi"])) if g["kind"] == "dense" else R.Kron(pick(g["Af"]), pick(g["Bf"]))


def n_problems(g):
    return g["y"].shape[0]


def reference(g):
    return [R.cosamp(operator(g, t), g["y"][t], g["K"], g["iters"], g["tol"]) for t in range(n_problems(g))]


def nmse_capped(x, Zbar):
    """plot_errorVSsnr.m:138-141 on x = vec(S)"""
    return float(O.nmse_capped(np.asarray(x).reshape(Zbar.shape, order="F"), Zbar))
