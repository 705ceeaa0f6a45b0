"""Problems, error measures and a numpy restatement for the float64 SVD with vectors (jstsp_svd_f64 / jstsp_lowrank_f64,
csrc/svd64.hip) - not a test module, numpy only; imports neither the device code nor the oracle.

``jacobi_svd_ref`` restates the algorithm of the two device routes in complex128: orientation to m >= n columns, the power-of-two
prescale, the round-robin order of jacobi_sweeps, the floor fro2 eps^2 / n under which a column is left alone, the stop rule
|g| <= sqrt(m) eps sqrt(a b), the rotation formula, the sort (equal norms keep column order), the drop rule of pinv.m and the swap
of the factors for rows < cols.  It differs from the device in summation order only (numpy's pairwise sums against the xor tree
and FMA contraction).  The bounds of tests/test_gpu_svd64.py for the reconstruction and the two orthogonality measures are 4 x
the worst value THIS restatement reaches over ``problem_set(route)``; tests/test_svd64_problems.py checks on the CPU that those
bounds stay under the a-priori ceiling and that numpy's own SVD meets them."""
import functools
import json
import os

import numpy as np

import spectrum_problems as P

EPS = 2.220446049250313e-16
SWEEP_CAP = {"lds": 30, "global": 40}                     # SV_SWEEPS (csrc/jacobi64.h), PV_SWEEPS (csrc/pinv64.hip)
SV_BOUND = {"lds": 9e-14, "global": 3.6e-13}              # tests/test_gpu_singular_values.py, tests/test_gpu_spectrum.py
MARGIN = 4.0
LDS_BYTES = 159 * 1024                                    # SVD_LDS_LIMIT (csrc/svd64.hip)

LDS_SHAPES = [(64, 64), (32, 140), (140, 32), (128, 50), (7, 13), (13, 7), (33, 3), (5, 5), (1, 7), (7, 1)]
GLOBAL_SHAPES = [(96, 300), (200, 97), (66, 520), (520, 66), (40, 600)]
BATCH = 3


def route_of(rows, cols):
    """The route csrc/svd64.hip takes for a shape: the operand and V, the norms, 16 doubles and the places within 159 KiB."""
    m, n = max(rows, cols), min(rows, cols)
    return "lds" if n <= 64 and (m + n) * n * 16 + (n + 16) * 8 + n * 4 <= LDS_BYTES else "global"


def drop_threshold(rows, cols, smax):
    """pinv.m: max(size(A)) * eps(sigma_max), eps(x) = 2^(floor(log2 x) - 52)."""
    smax = np.asarray(smax, dtype=np.float64)
    safe = np.where(smax > 0, smax, 1.0)
    return np.where(smax > 0, max(rows, cols) * np.ldexp(1.0, np.frexp(safe)[1] - 1 - 52), 0.0)


def classes(rows, cols, count=BATCH):
    """[(name, (count, rows, cols) complex128)]: random always; rank 6, graded over 12 decades and repeated where n >= 6."""
    rng = np.random.default_rng(1000003 * rows + cols)
    out = [("random", P.rand(rng, count, rows, cols) * 0.3)]
    if min(rows, cols) >= 6:
        out += P.conditioning_cases(rng, rows, cols, count)
    return out


@functools.lru_cache(maxsize=None)
def problem_set(route):
    """The committed problem set of a route: [(rows, cols, name, A)]."""
    shapes = LDS_SHAPES if route == "lds" else GLOBAL_SHAPES
    for r, c in shapes:
        assert route_of(r, c) == route, (r, c)
    return [(r, c, name, A) for r, c in shapes for name, A in classes(r, c)]


# ---------------------------------------------------------------------------------------------- the restatement
def _pairs(n):
    """The rounds of jacobi_sweeps: for each round the arrays (p, q), p < q < n, of its disjoint pairs."""
    ne = n + (n & 1)
    half, ring = ne // 2, ne - 1
    rounds = []
    for r in range(ring):
        ps, qs = [], []
        for k in range(half):
            u = ring if k == 0 else (r + k) % ring
            v = r if k == 0 else (r + ring - k) % ring
            p, q = min(u, v), max(u, v)
            if q < n:
                ps.append(p); qs.append(q)
        rounds.append((np.array(ps, dtype=int), np.array(qs, dtype=int)))
    return rounds


def jacobi_svd_ref(A, route=None):
    """(U, sv, V, rank, conv, sweeps) of a batch A (count, rows, cols) by the restated algorithm; U (count, rows, n),
    sv (count, n), V (count, cols, n).  ``sweeps``: the sweeps each matrix ran, the last (idle) one included."""
    A = np.asarray(A, dtype=np.complex128)
    if A.ndim == 2:
        A = A[None]
    B, rows, cols = A.shape
    route = route or route_of(rows, cols)
    tall = rows >= cols
    W = A.copy() if tall else np.conj(np.swapaxes(A, 1, 2)).copy()
    m, n = W.shape[1], W.shape[2]
    amax = np.max(np.maximum(np.abs(W.real), np.abs(W.imag)), axis=(1, 2))
    ex = np.where(amax > 0, np.frexp(np.where(amax > 0, amax, 1.0))[1], 0)
    ex = np.clip(ex, -1000, 1000)
    W *= np.ldexp(1.0, -ex)[:, None, None]                                   # exact
    fro2 = np.sum(W.real ** 2 + W.imag ** 2, axis=(1, 2))
    floor2 = fro2 * EPS * EPS / n
    tol = np.sqrt(float(m)) * EPS
    V = np.broadcast_to(np.eye(n, dtype=np.complex128), (B, n, n)).copy()
    active = np.ones(B, dtype=bool)
    sweeps = np.zeros(B, dtype=int)
    conv = np.zeros(B, dtype=int)
    rounds = _pairs(n)
    if n == 1:
        conv[:] = 1
    for _ in range(SWEEP_CAP[route] if n > 1 else 0):
        rotated = np.zeros(B, dtype=bool)
        for ps, qs in rounds:
            if ps.size == 0:
                continue
            cp, cq = W[:, :, ps], W[:, :, qs]
            a = np.sum(cp.real ** 2 + cp.imag ** 2, axis=1)                  # (sums down the rows, one after the other)
            b = np.sum(cq.real ** 2 + cq.imag ** 2, axis=1)
            g_c = np.sum(np.conj(cp) * cq, axis=1)
            g = np.abs(g_c)
            ab = np.sqrt(a) * np.sqrt(b)
            alive = (a > floor2[:, None]) & (b > floor2[:, None]) & active[:, None]
            signif = alive & (g > tol * ab)
            rot = signif if route == "lds" else alive & (g > 0.25 * EPS * ab)       # the global route also polishes
            rotated |= signif.any(axis=1)
            bi, hi = np.nonzero(rot)                                         # the pairs that rotate: (matrix, pair of the round)
            if bi.size == 0:
                continue
            a, b, g, g_c = a[bi, hi], b[bi, hi], g[bi, hi], g_c[bi, hi]
            z = (b - a) / (2.0 * g)
            t = np.copysign(1.0, z) / (np.abs(z) + np.hypot(1.0, z))
            c = 1.0 / np.sqrt(1.0 + t * t)
            s = (c * t)[:, None]
            c = c[:, None]
            wc = np.conj(g_c / g)[:, None]                                   # y conj(w), w = g / |g|
            pi, qi = ps[hi], qs[hi]
            for M in (W, V):
                x, y = M[bi, :, pi], M[bi, :, qi] * wc
                M[bi, :, pi] = c * x - s * y
                M[bi, :, qi] = s * x + c * y
        sweeps += active
        conv[active & ~rotated] = 1
        active &= rotated
        if not active.any():
            break
    nrm = np.sqrt(np.sum(W.real ** 2 + W.imag ** 2, axis=1))
    order = np.argsort(-nrm, axis=1, kind="stable")                          # equal norms keep column order
    snrm = np.take_along_axis(nrm, order, axis=1)
    thr = drop_threshold(rows, cols, snrm[:, 0])
    kept = snrm > thr[:, None]
    Wo = np.take_along_axis(W, order[:, None, :], axis=2)
    long = np.where(kept[:, None, :], Wo / np.where(kept, snrm, 1.0)[:, None, :], 0.0)
    short = np.take_along_axis(V, order[:, None, :], axis=2)
    sv = snrm * np.ldexp(1.0, ex)[:, None]
    U, Vo = (long, short) if tall else (short, long)
    return U, sv, Vo, kept.sum(axis=1).astype(np.int32), conv.astype(np.int32), sweeps


# ---------------------------------------------------------------------------------------------- the error measures
def numpy_svd(A):
    """(U, sv, V) of numpy.linalg.svd, econ, V not V^H, per matrix of a batch."""
    U, s, Vh = np.linalg.svd(np.asarray(A, dtype=np.complex128), full_matrices=False)
    return U, s, np.conj(np.swapaxes(Vh, -1, -2))


def _orth_err(Q):
    """max |Q^H Q - I| over the columns of Q (0 when there is none)."""
    if Q.shape[1] == 0:
        return 0.0
    return float(np.max(np.abs(np.conj(Q.T) @ Q - np.eye(Q.shape[1]))))


def measures(A, U, sv, V, ref_sv):
    """The four measures of one matrix at n_keep = n: dict e_sv, e_rec, e_long, e_short.  ref_sv: numpy.linalg.svd's values.
    The kept columns of the long-side factor are those the drop rule keeps on the values sv."""
    rows, cols = A.shape
    s1 = ref_sv[0]
    kept = int(np.sum(sv > drop_threshold(rows, cols, sv[0])))
    long, short = (U, V) if rows >= cols else (V, U)
    return {"e_sv": float(np.max(np.abs(sv - ref_sv)) / s1),
            "e_rec": float(np.linalg.norm(A - (U * sv) @ np.conj(V.T), 2) / s1),
            "e_long": _orth_err(long[:, :kept]),
            "e_short": _orth_err(short)}


def worst(rows_of_measures):
    keys = ("e_sv", "e_rec", "e_long", "e_short")
    return {k: max(r[k] for r in rows_of_measures) for k in keys}


@functools.lru_cache(maxsize=None)
def restatement_records(route):
    """Per problem of the route's set: (rows, cols, name, worst measures of the restatement, of numpy's SVD, largest sweep count,
    all converged)."""
    out = []
    for rows, cols, name, A in problem_set(route):
        ref = P.ref(A)
        U, sv, V, _, conv, sweeps = jacobi_svd_ref(A, route)
        Un, sn, Vn = numpy_svd(A)
        mine = worst([measures(A[t], U[t], sv[t], V[t], ref[t]) for t in range(A.shape[0])])
        nump = worst([measures(A[t], Un[t], sn[t], Vn[t], ref[t]) for t in range(A.shape[0])])
        out.append((rows, cols, name, mine, nump, int(sweeps.max()), bool(conv.all())))
    return out


def ceiling(route, n):
    """The a-priori ceiling 4 S (n - 1) 2^-52: one rounding of a complex rotation per rotation a column can meet, added linearly."""
    return 4.0 * SWEEP_CAP[route] * max(n - 1, 1) * 2.0 ** -52


def recomputed_worst(route):
    """The restatement's worst e_rec, e_long, e_short over the route's problem set, computed here (the global route: most of a minute)."""
    return worst([r[3] for r in restatement_records(route)])


FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svd64_restatement_worst.json")


@functools.lru_cache(maxsize=None)
def bounds(route):
    """The asserted bounds of a route: e_sv from the suites of the same rotations, the others MARGIN x the restatement's worst over
    the problem set, as recorded in tests/golden/svd64_restatement_worst.json (``python tests/svd64_problems.py`` writes it;
    tests/test_svd64_problems.py recomputes it and compares)."""
    with open(FIXTURE) as f:
        w = json.load(f)[route]["restatement"]
    return {"e_sv": SV_BOUND[route], "e_rec": MARGIN * w["e_rec"], "e_long": MARGIN * w["e_long"], "e_short": MARGIN * w["e_short"]}


if __name__ == "__main__":
    rec = {}
    for route in ("lds", "global"):
        rs = restatement_records(route)
        rec[route] = {"restatement": worst([r[3] for r in rs]), "numpy": worst([r[4] for r in rs]),
                      "sweeps": {"%dx%d %s" % (r[0], r[1], r[2]): r[5] for r in rs}}
    with open(FIXTURE, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, sort_keys=True))
