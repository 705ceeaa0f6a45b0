"""Float64 numpy restatement of proposed_algorithm.m / proposed_algorithm_angles.m ('approximate' and 'std') that takes and
returns the state of the iteration and the index of the first iteration (TEST INFRASTRUCTURE; the reference of every
arbitrary-state test of the resumed solvers).

The state of one trial is the block of include/jstsp.h (jstsp_admm_state_elems): ``[X | V1 | V2 | C]`` (N M each) then
``[v | S]`` (Gr G2 each), every matrix flattened column-major.  ``solve(..., state=None, it0=0)`` runs iterations
``it0 + 1 ... it0 + Imax`` (proposed_algorithm.m:32) and returns ``(S, Y, ce, state)``; ``ce`` has the rows of these iterations.
The statements are those of oracle/solvers.py proposed_algorithm (structured form), in its order of operations, so that from
the zero state the two agree to rounding; ``A S B`` is recomputed from the stored ``S``, which is the same product the loop
leaves behind, so a split run repeats the arithmetic of the whole one exactly.
"""
import numpy as np


def state_elems(N, M, Gr, G2):
    return 4 * N * M + 2 * Gr * G2


def pack_state(X, V1, V2, C, V, S):
    return np.concatenate([np.asarray(Z, dtype=np.complex128).reshape(-1, order="F") for Z in (X, V1, V2, C, V, S)])


def unpack_state(state, N, M, Gr, G2):
    state = np.asarray(state, dtype=np.complex128)
    assert state.shape == (state_elems(N, M, Gr, G2),)
    nm, g = N * M, Gr * G2
    mats = [state[k * nm:(k + 1) * nm].reshape(N, M, order="F") for k in range(4)]
    mats += [state[4 * nm + k * g:4 * nm + (k + 1) * g].reshape(Gr, G2, order="F") for k in range(2)]
    # row-major copies, the layout the loop's own results have: BLAS sums a product in the same order then (0 ulp, split vs whole)
    return [np.ascontiguousarray(Z) for Z in mats]


def _div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(a) / np.float64(b)


def _cdiv(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.complex128(a) / np.complex128(b)


def _norm2sq(X):
    return float(np.linalg.norm(X, 2)) ** 2 if min(X.shape) > 1 else float(np.linalg.norm(X.ravel())) ** 2


def svt(Y, tau):
    """svt.m:1-15: an exactly zero singular value makes 0/0 = NaN and the whole output zeros (:8-12)."""
    U, lam, Vh = np.linalg.svd(Y, full_matrices=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        soft = np.maximum(0.0, lam - tau) * lam / np.abs(lam)
    if np.any(np.isnan(soft)):
        return np.zeros(Y.shape, dtype=np.complex128)
    return (U * soft) @ Vh


def soft(v, t):
    return (np.maximum(np.abs(v.real) - t, 0) * np.sign(v.real) + 1j * np.maximum(np.abs(v.imag) - t, 0) * np.sign(v.imag))


def solve(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type_="approximate", indx_S=None, state=None, it0=0, want_ce=True):
    subY = np.asarray(subY, dtype=np.complex128)
    Omega = np.asarray(Omega, dtype=np.float64)
    A = np.asarray(A, dtype=np.complex128)
    B = np.asarray(B, dtype=np.complex128)
    N, M = subY.shape
    Gr, G2 = A.shape[1], B.shape[0]
    assert it0 >= 0 and (state is not None or it0 == 0) and type_ in ("approximate", "std")
    if state is None:
        state = np.zeros(state_elems(N, M, Gr, G2), dtype=np.complex128)                  # :8-12, :27
    X, V1, V2, C, V, S = unpack_state(state, N, M, Gr, G2)
    Xs = A @ S @ B                                                                      # what :58 left behind
    inv_d = 1.0 / (Omega + 2 * rho)                                                     # :14-20
    Ah, Bh = A.conj().T, B.conj().T
    if type_ == "approximate":
        GA, GB = Ah @ A, B @ Bh                                                         # :25
    else:
        pA, pB = np.linalg.pinv(A), np.linalg.pinv(B)                                   # :29, :53 for a K2 of full column rank
    ce = np.zeros((Imax, 3))
    Y = np.zeros((N, M), dtype=np.complex128)
    for i in range(it0 + 1, it0 + Imax + 1):                                            # :32
        Y = svt(X - V1 / rho, tau_Y / rho)                                              # :35
        X = (V1 + rho * Y + subY + V2 + rho * C + rho * Xs) * inv_d                     # :38-40
        K = X - V2 / rho - C                                                            # :43
        if type_ == "approximate":
            Res = Ah @ K @ Bh - GA @ V @ GB                                             # :47
            alpha = _cdiv(np.vdot(Res, Res), np.vdot(Res, GA @ Res @ GB))               # :48
            Vp = V
            V = V + alpha * Res                                                         # :50
            ce[i - it0 - 1, 2] = _div(np.linalg.norm(Vp - V) ** 2, np.linalg.norm(Vp) ** 2)      # :51
        else:
            V = pA @ K @ pB                                                             # :53
        S = soft(V, tau_S / rho)                                                        # :56
        if indx_S is not None:                                                          # angles :36, :68 (the mask only grows)
            lin = np.asarray(indx_S[:min(10 + 5 * i, Gr * G2)], dtype=np.int64) - 1
            mask = np.zeros(Gr * G2)
            mask[lin] = 1
            S = mask.reshape(Gr, G2, order="F") * S
        Xs = A @ S @ B                                                                  # :58
        C = rho / (rho + 1) * (X - Xs - V2 / rho)                                       # :61
        V1 = V1 + rho * (Y - X)                                                         # :64
        V2 = V2 + rho * (C - X + Xs)                                                    # :65
        if want_ce:
            nX = _norm2sq(X)
            ce[i - it0 - 1, 0] = _div(_norm2sq(V1), nX)                                 # :67
            ce[i - it0 - 1, 1] = _div(_norm2sq(V2), nX)                                 # :69
    return S, Y, ce, pack_state(X, V1, V2, C, V, S)
