"""Float64 numpy restatement of the least-squares re-fit of an estimate on its support (jstsp_refit_f64, include/jstsp.h; TEST
INFRASTRUCTURE, not a test module): conjugate gradients from the given estimate on the normal equations of

    min_x ||Omega .* (A x B) - subY||_F^2 + lam ||x||_F^2        x supported on T

with T the first K entries of ``indx_S`` (1-based, column-major linear indices; entries outside 1 .. g ignored) or, without one,
of ``order_of(S_in)`` of tests/refresh_ref.py (descending magnitude, equal keys in ascending index, NaN first).  K == g: no mask.

    G(x) = m .* (A^H ((Omega .* Omega) .* (A x B)) B^H) + lam x;   b = m .* (A^H (Omega .* subY) B^H)
    x = m .* S_in; r = b - G(x); p = r; gamma = <r, r>
    k = 1 .. iters:  q = G(p); delta = Re<p, q>; alpha = gamma / delta; x += alpha p; r -= alpha q; gamma' = <r, r>;
                     p = r + (gamma' / gamma) p; gamma = gamma'

A trial freezes at the first k at whose start gamma == 0 or (tol > 0 and) gamma <= tol^2 gamma_0, or whose delta is not positive
and finite; x stays as it is.  ``refit`` returns ``(x, steps, resid)``: resid = gamma_0 .. gamma_iters, NaN after the last step.
``trace``, when a list is passed, receives x after every step (x_0 first)."""
import numpy as np

from refresh_ref import order_of


def support_mask(S_in, K, indx_S=None):
    """The indicator of T as a (Gr, G2) array of 0 / 1."""
    Gr, G2 = S_in.shape
    g = Gr * G2
    assert 1 <= K <= g
    if K == g:
        return np.ones((Gr, G2))
    lin = (order_of(S_in) if indx_S is None else np.asarray(indx_S, dtype=np.int64).reshape(-1))[:K].astype(np.int64) - 1
    lin = lin[(lin >= 0) & (lin < g)]
    m = np.zeros(g)
    m[lin] = 1
    return m.reshape(Gr, G2, order="F")


def objective(subY, Omega, A, B, x, lam=0.0):
    """||Omega .* (A x B) - subY||_F^2 + lam ||x||_F^2"""
    return float(np.linalg.norm(Omega * (A @ x @ B) - subY) ** 2 + lam * np.linalg.norm(x) ** 2)


def refit(subY, Omega, A, B, S_in, K, iters, lam=0.0, tol=0.0, indx_S=None, trace=None):
    subY = np.asarray(subY, dtype=np.complex128)
    Omega = np.asarray(Omega, dtype=np.float64)
    A = np.asarray(A, dtype=np.complex128)
    B = np.asarray(B, dtype=np.complex128)
    S_in = np.asarray(S_in, dtype=np.complex128)
    assert iters >= 1 and lam >= 0 and tol >= 0
    m = support_mask(S_in, K, indx_S)
    on = m != 0
    Ah, Bh, w2 = A.conj().T, B.conj().T, Omega * Omega

    def mask(Z):                                    # (not m * Z: a NaN or Inf off the support must not come through)
        return np.where(on, Z, 0)

    def G(x):
        return mask(Ah @ (w2 * (A @ x @ B)) @ Bh) + lam * x

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x = mask(S_in)
        r = mask(Ah @ (Omega * subY) @ Bh) - G(x)
        p = r.copy()
        gamma = gamma0 = float(np.vdot(r, r).real)
        resid = np.full(iters + 1, np.nan)
        resid[0] = gamma
        steps = 0
        if trace is not None:
            trace.append(x.copy())
        for k in range(1, iters + 1):
            if gamma == 0.0 or (tol > 0.0 and gamma <= tol * tol * gamma0):
                break
            q = G(p)
            delta = float(np.vdot(p, q).real)
            if not (delta > 0.0 and np.isfinite(delta)):
                break
            alpha = gamma / delta
            x = x + alpha * p
            r = r - alpha * q
            gnew = float(np.vdot(r, r).real)
            p = r + (gnew / gamma) * p
            gamma = gnew
            resid[k] = gamma
            steps = k
            if trace is not None:
                trace.append(x.copy())
    return x, steps, resid
