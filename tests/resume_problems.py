"""Problems for the resumed float64 ADMM (tests/test_gpu_resume64.py): batch 3, complex128, per-trial tau_Y, tau_S, rho, a
sparse S0 observed on half the entries, B per trial or shared, at

  R1  32, 140, 32, 16   the reference's own driver shape: Gram order 32, the in-LDS Jacobi
  R2  72, 80, 24, 20    Gram order 72 > 64: the global-memory Jacobi

N >= Gr and M >= G2 in both, so Alg. 1 ('std') is a least-squares solve.  indx_S puts the support of S0 at ranks 31 ... 34 of
its trial: the mask of iteration i holds the first 10 + 5 i ranks (angles :36), so these entries are masked away up to
iteration 4 and kept from iteration 5 on - a second leg that restarts the count at 0 is told apart from one that goes on.
"""
import functools

import numpy as np

SHAPES = {"R1": (32, 140, 32, 16), "R2": (72, 80, 24, 20)}
BATCH = 3
SUPPORT_RANKS = (31, 32, 33, 34)


def _c(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


@functools.lru_cache(maxsize=None)
def problem(name, shared_B):
    """dict(subY, Omega, A, B, tau_Y, tau_S, rho, indx_S): batch-first arrays, A shared, B shared or per trial."""
    N, M, Gr, G2 = SHAPES[name]
    rng = np.random.default_rng([20190913, N, int(shared_B)])
    A = _c(rng, N, Gr) / np.sqrt(N)
    B = _c(rng, G2, M) / np.sqrt(G2) if shared_B else _c(rng, BATCH, G2, M) / np.sqrt(G2)
    S0 = np.zeros((BATCH, Gr, G2), complex)
    idx = np.zeros((BATCH, Gr * G2), np.int32)
    for t in range(BATCH):
        sup = rng.choice(Gr * G2, len(SUPPORT_RANKS), replace=False)
        flat = np.zeros(Gr * G2, complex)
        flat[sup] = 3 * _c(rng, len(sup))
        S0[t] = flat.reshape(Gr, G2, order="F")
        rest = rng.permutation(np.setdiff1d(np.arange(Gr * G2), sup))
        order = np.concatenate([rest[:SUPPORT_RANKS[0]], sup, rest[SUPPORT_RANKS[0]:]])
        idx[t] = order + 1                                        # 1-based linear indices, column-major
    Om = (rng.random((BATCH, N, M)) < 0.5).astype(float)
    subY = Om * (A @ S0 @ B + 0.05 * _c(rng, BATCH, N, M))
    tY = 0.02 + 0.01 * rng.random(BATCH); tS = 0.02 + 0.01 * rng.random(BATCH); rho = 0.2 + 0.3 * rng.random(BATCH)
    return dict(subY=subY, Omega=Om, A=A, B=B, tau_Y=tY, tau_S=tS, rho=rho, indx_S=idx)


def trial(p, t):
    """The arguments of tests/resume_ref.py solve() for trial t: (subY, Omega, A, B), (tau_Y, tau_S, rho), indx_S."""
    B = p["B"] if p["B"].ndim == 2 else p["B"][t]
    return (p["subY"][t], p["Omega"][t], p["A"], B), (float(p["tau_Y"][t]), float(p["tau_S"][t]), float(p["rho"][t])), p["indx_S"][t]
