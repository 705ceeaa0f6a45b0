"""Problems for Alg. 1 in float64 (jstsp_proposed_std_f64; tests/test_gpu_std64.py), all complex128 with N >= Gr and M >= G2:

  P1  7, 13, 5, 9, Imax 25     ragged: every GEMM tile partial
  P2  6, 9, 6, 9, Imax 20      square K2 = kron(B.', A): U\\(L\\k) is an exact solve
  P3  batch 5 of 16, 40, 12, 24, Imax 20, per-trial B, shared A, per-trial scalars, with and without indx_S; trial 3 also at
      Imax 60 with indx_S, where the cumulative mask count 10 + 5 i passes Gr G2 = 288 (i >= 56) and saturates
  P4  8, 520, 6, 6, Imax 8     B^H is 520 x 6: one workgroup per column pair in the Hestenes rounds (column length > 512)
  P5  72, 80, 8, 10, Imax 4    min(N, M) > 64: svt and lambda_max on the global-memory Jacobi
  P6  P1 with B = Q1 diag(d) Q2, d = geomspace(1, 1e-6): cond(B) = 1e6, exact pseudo-inverse Q2^H diag(1 / d) Q1^H

``reference(name)`` is oracle.solvers.proposed_algorithm(..., 'std') per trial, computed once per session.  ``std_loop`` is that
function's 'std' loop with the two pseudo-inverses as arguments (tests/test_std64_problems.py holds it to the oracle's bits when
they are numpy's); ``p6_spread()`` runs it on P6 with numpy's pinv(B) and with the exact one: the distance between the two is
what a float64 evaluation of P6 can be told apart by, and sets P6's bound.
"""
import functools

import numpy as np

from std_problems import haar

TOL64_S, TOL64_CE = 1e-10, 1e-8          # the sibling entry's bounds (tests/test_gpu_f64_proposed.py)
P6_MARGIN = 100.0                        # the margin the sibling bounds took over the spread of two float64 restatements
REFNATIVE = (32, 140, 32, 16)            # N, M, Gr, G2 of the reference's own driver


def _c(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def _single(seed, N, M, Gr, G2, Imax, B=None, nnz=3):
    """One trial: (subY, Omega, A, B, Imax, tau_Y, tau_S, rho) on a sparse S0 observed on half the entries."""
    rng = np.random.default_rng(seed)
    A = _c(rng, N, Gr) / np.sqrt(N)
    if B is None:
        B = _c(rng, G2, M) / np.sqrt(G2)
    S0 = np.zeros((Gr, G2), complex)
    S0.flat[rng.choice(Gr * G2, nnz, replace=False)] = 3 * _c(rng, nnz)
    Om = (rng.random((N, M)) < 0.5).astype(float)
    subY = Om * (A @ S0 @ B + 0.05 * _c(rng, N, M))
    return subY, Om, A, B, Imax, 0.01, 0.02, 0.3


def p6_factor():
    """(B, pinv(B) exact, d): 9 x 13, singular values geomspace(1, 1e-6, 9)."""
    rng = np.random.default_rng([20190913, 6])
    d = np.geomspace(1.0, 1e-6, 9)
    Q1, Q2 = haar(rng, 9, 9), haar(rng, 13, 9).conj().T
    return (Q1 * d) @ Q2, (Q2.conj().T / d) @ Q1.conj().T, d


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, indx_S): batch-first arrays for P3, one trial otherwise."""
    if name == "P3":
        rng = np.random.default_rng(31)
        N, M, Gr, G2, nb = 16, 40, 12, 24, 5
        A = _c(rng, N, Gr) / np.sqrt(N)
        B = _c(rng, nb, G2, M) / np.sqrt(G2)
        S0 = np.zeros((nb, Gr, G2), complex)
        for t in range(nb):
            S0[t].flat[rng.choice(Gr * G2, 4, replace=False)] = 3 * _c(rng, 4)
        Om = (rng.random((nb, N, M)) < 0.5).astype(float)
        subY = Om * (A @ S0 @ B + 0.05 * _c(rng, nb, N, M))
        tY = 0.02 + 0.01 * rng.random(nb); tS = 0.02 + 0.01 * rng.random(nb); rho = 0.2 + 0.3 * rng.random(nb)
        idx = np.stack([rng.permutation(Gr * G2) + 1 for _ in range(nb)]).astype(np.int32)
        return dict(subY=subY, Omega=Om, A=A, B=B, Imax=20, tau_Y=tY, tau_S=tS, rho=rho, indx_S=idx)
    spec = {"P1": (7, 7, 13, 5, 9, 25), "P2": (2, 6, 9, 6, 9, 20), "P4": (4, 8, 520, 6, 6, 8), "P5": (5, 72, 80, 8, 10, 4),
            "P6": (7, 7, 13, 5, 9, 25)}[name]
    k = ("subY", "Omega", "A", "B", "Imax", "tau_Y", "tau_S", "rho")
    p = dict(zip(k, _single(*spec, B=p6_factor()[0] if name == "P6" else None)))
    p["indx_S"] = None
    return p


NAMES = ("P1", "P2", "P3", "P4", "P5", "P6")
P3_SATURATE = (3, 60)                    # (trial, Imax) of the P3 run in which the mask count saturates


def args(name):
    p = problem(name)
    return tuple(p[k] for k in ("subY", "Omega", "A", "B", "Imax", "tau_Y", "tau_S", "rho"))


@functools.lru_cache(maxsize=None)
def reference(name, angles=False, trial=None, Imax=None):
    """oracle 'std' on the problem: (S, Y, ce), stacked over the batch for P3 (or one `trial` of it, at `Imax`)."""
    from oracle import solvers as O
    p = problem(name)
    im = p["Imax"] if Imax is None else Imax
    if name != "P3":
        return O.proposed_algorithm(p["subY"], p["Omega"], p["A"], p["B"], im, p["tau_Y"], p["tau_S"], p["rho"], "std")
    run = lambda t: O.proposed_algorithm(p["subY"][t], p["Omega"][t], p["A"], p["B"][t], im, p["tau_Y"][t], p["tau_S"][t], p["rho"][t], "std",
                                         indx_S=p["indx_S"][t] if angles else None)
    if trial is not None:
        return run(trial)
    out = [run(t) for t in range(5)]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def std_loop(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, pA, pB):
    """The 'std' loop of oracle.solvers.proposed_algorithm, statement for statement, with pinv(A), pinv(B) given."""
    from oracle import solvers as O
    N, M = subY.shape
    ce = np.zeros((Imax, 3))
    X = np.zeros((N, M), complex); V1 = np.zeros((N, M), complex); V2 = np.zeros((N, M), complex)
    C = np.zeros((N, M), complex); Xs = np.zeros((N, M), complex)
    inv_d = 1.0 / (Omega + 2 * rho)
    for i in range(1, Imax + 1):
        Y = O.svt(X - V1 / rho, tau_Y / rho)
        X = (V1 + rho * Y + subY + V2 + rho * C + rho * Xs) * inv_d
        K = X - V2 / rho - C
        V = pA @ K @ pB
        S = O.soft_threshold_complex(V, tau_S / rho)
        Xs = A @ S @ B
        C = rho / (rho + 1) * (X - Xs - V2 / rho)
        V1 = V1 + rho * (Y - X)
        V2 = V2 + rho * (C - X + Xs)
        nX = O.spectral_norm(X) ** 2
        ce[i - 1, 0] = O._div(O.spectral_norm(V1) ** 2, nX)
        ce[i - 1, 1] = O._div(O.spectral_norm(V2) ** 2, nX)
    return S, Y, ce


def rel_err(a, b):
    den = np.max(np.abs(b))
    return float(np.max(np.abs(a - b)) / (den if den > 0 else 1.0))


def ce_spread(ce, ref):
    fin = np.isfinite(ref)
    return float(np.max(np.abs(ce[fin] - ref[fin]) / np.abs(ref[fin]))) if fin.any() else 0.0


@functools.lru_cache(maxsize=None)
def p6_spread():
    """(d, d_ce): on P6, numpy's pinv(B) against the exact pseudo-inverse in the same loop - d over S and Y (max|.| / max|ref|),
    d_ce over convergence_error(:, 1:2) (relative per entry)."""
    a = args("P6")
    pA = np.linalg.pinv(a[2])
    Sn, Yn, cen = std_loop(*a, pA, np.linalg.pinv(a[3]))
    Se, Ye, cee = std_loop(*a, pA, p6_factor()[1])
    return max(rel_err(Sn, Se), rel_err(Yn, Ye)), ce_spread(cen[:, :2], cee[:, :2])


def p6_bounds():
    """(bound on S and Y, bound on convergence_error): max(sibling bound, 100 d)."""
    d, dce = p6_spread()
    return max(TOL64_S, P6_MARGIN * d), max(TOL64_CE, P6_MARGIN * dce)

