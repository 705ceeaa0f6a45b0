"""Problems for the float64 re-fit (tests/test_gpu_refit64.py, tests/test_refit_ref.py; TEST INFRASTRUCTURE): R1 and R2 of
tests/resume_problems.py - batch 3, B per trial or shared - with S_in the estimate tests/resume_ref.py returns after 6 iterations of
Alg. 2 (a dense S, as the solver's is), and one larger trial whose g = 8192 entries exceed the selection kernel's list of 4096 and
whose products span several tiles."""
import functools

import numpy as np

import resume_problems as P
import resume_ref as R

NAMES = ("R1", "R2")
KS = (4, 40, None)              # None: K = g, no mask
ITERS = (1, 6)
LAMS = (0.0, 0.1)
BIG_SHAPE = (64, 256, 64, 128)  # N, M, Gr, G2
BIG_K, BIG_ITERS = 4096, 3


@functools.lru_cache(maxsize=None)
def s_in(name, shared_B):
    """(batch, Gr, G2): S of tests/resume_ref.py after 6 iterations, per trial."""
    p = P.problem(name, shared_B)
    out = []
    for t in range(P.BATCH):
        m, prm, _ = P.trial(p, t)
        out.append(R.solve(*m, 6, *prm, "approximate", want_ce=False)[0])
    S = np.stack(out)
    S.setflags(write=False)
    return S


def trial(name, shared_B, t):
    """(subY, Omega, A, B, S_in) of trial t."""
    p = P.problem(name, shared_B)
    return P.trial(p, t)[0] + (s_in(name, shared_B)[t],)


def k_of(name, K):
    N, M, Gr, G2 = P.SHAPES[name]
    return Gr * G2 if K is None else K


@functools.lru_cache(maxsize=None)
def big():
    """dict(subY, Omega, A, B, S_in), batch 1: a sparse S0 seen on half the entries in noise, S_in = S0 plus a dense perturbation."""
    N, M, Gr, G2 = BIG_SHAPE
    rng = np.random.default_rng([20190913, 8192])
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    A, B = c(N, Gr) / np.sqrt(N), c(G2, M) / np.sqrt(G2)
    flat = np.zeros(Gr * G2, complex)
    sup = rng.choice(Gr * G2, 12, replace=False)
    flat[sup] = 3 * c(12)
    S0 = flat.reshape(Gr, G2, order="F")
    Om = (rng.random((N, M)) < 0.5).astype(float)
    subY = Om * (A @ S0 @ B + 0.05 * c(N, M))
    S = S0 + 0.05 * c(Gr, G2)
    return dict(subY=subY[None], Omega=Om[None], A=A, B=B, S_in=S[None])
