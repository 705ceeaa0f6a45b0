"""Float64 restatement of the CoSaMP loop that include/jstsp.h states (Needell & Tropp, Algorithm 1), numpy complex128,
CPU only, with a DECISION RECORD: what a device implementation may legitimately decide otherwise.

    a = 0; kept = {}; v = u
    for it = 1 .. iters:
        c = Phi' v;  Omega = the min(2K, size_d) largest |c|^2 (smaller index first among equals);  T = sort(Omega U kept)
        b = argmin ||Phi(:,T) b - u||  (numpy.linalg.lstsq);  kept = the K largest |b|^2 of T (smaller position first)
        a = b on kept, 0 elsewhere;  v = u - Phi a;  stop when ||v|| <= tol ||u||   (tol = 0: never)

Rank: Phi(:,T) with sigma_min / sigma_max <= RANK_R stops the problem with status 1 and the iterate it had.  (The device
tests a Cholesky pivot of the Gram against 1e-12 of its largest diagonal entry; the two rules agree wherever
r = sigma_min / sigma_max is above 1e-5 or below 1e-7, and the fixture's problems are kept out of the band between.)

The loop carries only the index set and, through v, the values of a; b is solved from u afresh.  So two correct
implementations part only at a decision.  For every selection, prune and stop test the record keeps the relative gap at
the boundary, and for every least squares |T| and r.  With beta = SAFETY |T| eps64 / r^2 (the forward error of a float64
normal-equations solve, n eps cond(G), times SAFETY):
    a prune is decided      when its gap >= max(FLOOR, beta)
    a selection is decided  when its gap >= max(FLOOR, beta ||u|| / ||v||), beta and v of the iteration before
    a stop test is decided  when | ||v|| / (tol ||u||) - 1 | >= FLOOR
and a problem is decided when all its decisions are."""
import numpy as np

SAFETY = 10.0
FLOOR = 1e-9
RANK_R = 1e-7
EPS = float(np.finfo(np.float64).eps)


class Dense:
    def __init__(self, Phi):
        self.Phi = np.asarray(Phi, np.complex128)
        self.meas, self.size_d = self.Phi.shape

    def corr(self, v):
        return self.Phi.conj().T @ v

    def cols(self, T):
        return self.Phi[:, T]


class Kron:
    """Phi = kron(Bf.', Af) from its factors, never formed: atom g + Gr h is kron(Bf[h, :], Af[:, g])."""

    def __init__(self, Af, Bf):
        self.Af, self.Bf = np.asarray(Af, np.complex128), np.asarray(Bf, np.complex128)
        (self.N, self.Gr), (self.G2, self.M) = self.Af.shape, self.Bf.shape
        self.meas, self.size_d = self.N * self.M, self.Gr * self.G2

    def corr(self, v):
        V = v.reshape(self.N, self.M, order="F")
        return (self.Af.conj().T @ V @ self.Bf.conj().T).reshape(-1, order="F")

    def cols(self, T):
        T = np.asarray(T)
        g, h = T % self.Gr, T // self.Gr
        # column j: vec(Af[:, g_j] Bf[h_j, :])
        return (self.Af[:, g][:, None, :] * self.Bf[h, :].T[None, :, :]).reshape(self.meas, len(T), order="F")


def _boundary_gap(score, k):
    """order (descending, smaller index first among equals) and the relative gap between the k-th and (k+1)-th value"""
    order = np.argsort(-score, kind="stable")
    if k >= score.size:
        return order, np.inf
    top = score[order[0]]
    return order, (float((score[order[k - 1]] - score[order[k]]) / top) if top > 0 else 0.0)


def cosamp(op, u, K, iters, tol):
    """Returns dict(x, support (1-based, ascending, zeros when nothing was kept), iters, resid, status, record).
    record: lists per executed iteration - sel_gap, sel_budget, nT, r, beta, prune_gap, stop_gap - and `decided`,
    `beta_max`, `sel_budget_max`, `r_min`."""
    u = np.asarray(u, np.complex128).reshape(-1)
    K = int(K)
    assert K >= 1 and 2 * K <= op.size_d and 3 * K <= op.meas and iters >= 1 and tol >= 0
    rec = dict(sel_gap=[], sel_budget=[], nT=[], r=[], beta=[], prune_gap=[], stop_gap=[])
    nu = float(np.linalg.norm(u))
    a = np.zeros(op.size_d, np.complex128)
    kept = np.zeros(0, np.int64)
    out = dict(x=a, support=np.zeros(K, np.int32), iters=0, resid=1.0 if nu > 0 else 0.0, status=0)
    v, beta_prev, nv = u.copy(), 0.0, nu
    decided = True
    for _ in range(int(iters) if nu > 0 else 0):
        c = op.corr(v)
        order, gap = _boundary_gap(c.real ** 2 + c.imag ** 2, min(2 * K, op.size_d))
        budget = max(FLOOR, beta_prev * nu / nv) if nv > 0 else np.inf
        T = np.union1d(order[:min(2 * K, op.size_d)], kept)
        P = op.cols(T)
        s = np.linalg.svd(P, compute_uv=False)
        r = float(s[-1] / s[0])
        rec["sel_gap"].append(gap); rec["sel_budget"].append(budget); rec["nT"].append(len(T)); rec["r"].append(r)
        decided &= gap >= budget
        if r <= RANK_R:
            out["status"] = 1
            break
        beta = SAFETY * len(T) * EPS / r ** 2
        b = np.linalg.lstsq(P, u, rcond=None)[0]
        porder, pgap = _boundary_gap(b.real ** 2 + b.imag ** 2, K)
        pos = np.sort(porder[:K])
        kept = T[pos]
        a = np.zeros(op.size_d, np.complex128)
        a[kept] = b[pos]
        v = u - P[:, pos] @ b[pos]
        nv = float(np.linalg.norm(v))
        sgap = abs(nv / (tol * nu) - 1.0) if tol > 0 else np.inf
        rec["beta"].append(beta); rec["prune_gap"].append(pgap); rec["stop_gap"].append(sgap)
        decided &= pgap >= max(FLOOR, beta) and sgap >= FLOOR
        beta_prev = beta
        out.update(x=a, support=(kept + 1).astype(np.int32), iters=out["iters"] + 1, resid=nv / nu)
        if tol > 0 and nv <= tol * nu:
            break
    rec["decided"] = bool(decided)
    rec["beta_max"] = float(max(rec["beta"], default=0.0))
    fin = [b_ for b_ in rec["sel_budget"] if np.isfinite(b_)]
    rec["sel_budget_max"] = float(max(fin, default=FLOOR))
    rec["r_min"] = float(min(rec["r"], default=1.0))
    out["record"] = rec
    return out
