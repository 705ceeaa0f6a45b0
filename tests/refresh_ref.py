"""Float64 numpy restatement of the refreshed Alg. 2 (jstsp_proposed_refresh_f64; TEST INFRASTRUCTURE, not a test module): the
loop of tests/resume_ref.py ('approximate') with the support policy written out directly - at a refresh iteration the order is a
stable argsort of the key of the new v, and the mask of every iteration is the head of the order in force.

    i refreshes  <=>  i > start and (i - start - 1) % period == 0      (period >= 1)
                      i == start + 1                                   (period == 0)
    cnt(i) = min(10 + 5 i, g);  a refreshed order lists top = min(g, 4096) entries, an indx_S its own n; entries that the order
    in force does not list are never admitted; without an order in force nothing is masked.

``solve`` returns ``(S, Y, ce, state, order)``; ``order`` is the list of the call's last refresh, or ``indx_S`` as given when the
call ran none.  ``gaps``, when a list is passed, receives per iteration under a refreshed order the relative gap between the keys
on either side of the mask boundary (``None`` where the mask holds the whole list): what decides whether a last-bit difference in
v can change the mask."""
import numpy as np

import resume_ref as R

TOP_MAX = 4096


def is_refresh(i, start, period):
    return i > start and ((i - start - 1) % period == 0 if period else i == start + 1)


def schedule(it0, Imax, start, period):
    """The refresh iterations (global, 1-based) among it0 + 1 ... it0 + Imax."""
    return [i for i in range(it0 + 1, it0 + Imax + 1) if is_refresh(i, start, period)]


def key(V):
    """|z|^2 = x*x + y*y of vec(V), column-major, every product and the sum rounded to float64."""
    v = np.asarray(V, dtype=np.complex128).reshape(-1, order="F")
    with np.errstate(over="ignore", invalid="ignore"):
        return v.real * v.real + v.imag * v.imag


def order_of(V):
    """[~, indx] = sort(abs(vec(V)), 'descend'), 1-based: a stable argsort of the negated key, NaN first, equal keys by index."""
    k = key(V)
    o = np.argsort(-k, kind="stable")                       # numpy sorts a NaN last, in index order
    nan = np.isnan(k[o])
    return (np.concatenate([o[nan], o[~nan]]) + 1).astype(np.int32)


def solve(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, start=0, period=1, indx_S=None, state=None, it0=0, want_ce=True, gaps=None):
    subY = np.asarray(subY, dtype=np.complex128)
    Omega = np.asarray(Omega, dtype=np.float64)
    A = np.asarray(A, dtype=np.complex128)
    B = np.asarray(B, dtype=np.complex128)
    N, M = subY.shape
    Gr, G2 = A.shape[1], B.shape[0]
    g = Gr * G2
    assert it0 >= 0 and (state is not None or it0 == 0) and start >= 0 and period >= 0
    if state is None:
        state = np.zeros(R.state_elems(N, M, Gr, G2), dtype=np.complex128)
    X, V1, V2, C, V, S = R.unpack_state(state, N, M, Gr, G2)
    Xs = A @ S @ B
    inv_d = 1.0 / (Omega + 2 * rho)
    Ah, Bh = A.conj().T, B.conj().T
    GA, GB = Ah @ A, B @ Bh
    ce = np.zeros((Imax, 3))
    Y = np.zeros((N, M), dtype=np.complex128)
    in_force = None if indx_S is None else np.asarray(indx_S, dtype=np.int64).reshape(-1)
    order, fresh_key = indx_S, None
    for i in range(it0 + 1, it0 + Imax + 1):
        Y = R.svt(X - V1 / rho, tau_Y / rho)
        X = (V1 + rho * Y + subY + V2 + rho * C + rho * Xs) * inv_d
        K = X - V2 / rho - C
        Res = Ah @ K @ Bh - GA @ V @ GB
        alpha = R._cdiv(np.vdot(Res, Res), np.vdot(Res, GA @ Res @ GB))
        Vp = V
        V = V + alpha * Res
        ce[i - it0 - 1, 2] = R._div(np.linalg.norm(Vp - V) ** 2, np.linalg.norm(Vp) ** 2)
        S = R.soft(V, tau_S / rho)
        if is_refresh(i, start, period):                    # the order of the new v: its top entries, nothing else listed
            order = order_of(V)[:min(g, TOP_MAX)]
            in_force, fresh_key = order.astype(np.int64), key(V)
        if in_force is not None:
            cnt = min(10 + 5 * i, g)
            lin = in_force[:cnt] - 1
            lin = lin[(lin >= 0) & (lin < g)]
            mask = np.zeros(g)
            mask[lin] = 1
            S = mask.reshape(Gr, G2, order="F") * S
            if gaps is not None and fresh_key is not None:
                if cnt < in_force.size:
                    a, b = fresh_key[in_force[cnt - 1] - 1], fresh_key[in_force[cnt] - 1]
                    gaps.append(abs(a - b) / abs(a) if a != 0 else 0.0)
                else:
                    gaps.append(None)
        Xs = A @ S @ B
        C = rho / (rho + 1) * (X - Xs - V2 / rho)
        V1 = V1 + rho * (Y - X)
        V2 = V2 + rho * (C - X + Xs)
        if want_ce:
            nX = R._norm2sq(X)
            ce[i - it0 - 1, 0] = R._div(R._norm2sq(V1), nX)
            ce[i - it0 - 1, 1] = R._div(R._norm2sq(V2), nX)
    return S, Y, ce, R.pack_state(X, V1, V2, C, V, S), order
