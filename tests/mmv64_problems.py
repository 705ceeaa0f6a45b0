"""Joint (MMV) OMP problems for jstsp_mmv_omp_f64 (csrc/mmv_omp64.hip), seeded and CPU only.

The 32 rows of tests/mmv_problems.py are reused unchanged (kinds M1-M7, complex64 values, both row scores) and two complex128
kinds are added, each row ``dict(kind, name, A, Y, K, ref={norm: dict(Z, sup, count, gaps)}, facts...)`` as there:

- M8 decisive only in float64: an axis-aligned dictionary (omp_problems.axis_dictionary) and Y = A Z0 with four planted rows of
  magnitudes 5, 3, 3 (1 + d), 1 with d in [1e-9, 8e-9]: the second selection has a float64 relative gap of about 2 d (l2) or d
  (l1) - far below what an fp32 score resolves - and the larger of the two rows sits at the HIGHER atom index, so breaking a
  false tie by the lowest index gives the wrong support.  Every other gap is >= 1e-3.
- M9 scale: the first M1 row with Y * 2^k, k in Y64_SCALES (exact in float64); the reference selects the unscaled support.

``restate`` is a float64 numpy restatement of the kernel's algorithm - the scaling by 2^-e, scores from A^H R, two passes of
Gram-Schmidt, the three stop rules with their constants, one back-substitution - that tests/test_mmv64_problems.py holds against
the oracle on every row: the tolerance of the GPU test is not asking for more than the algorithm can give."""
import functools

import numpy as np

import mmv_problems as P
from oracle import solvers as O
from omp_problems import axis_dictionary

NORMS = P.NORMS
Y64_SCALES = (-400, -100, 100, 400)
M8_GAP = (1e-10, 1e-6)              # the float64 gap of the close selection
TOL_Z = 1e-12                       # cond(A[:, support]) <= 100 times 2^-53 times about 90 for dot products of up to 300 terms
GAP_MIN = 1e-9                      # a selection with a float64 gap >= this, or exactly 0, must be the oracle's


def reference(A, Y, K):
    out = {}
    for norm in NORMS:
        Z, sup, gaps = O.mmv_omp_margins(np.asarray(A, np.complex128), np.asarray(Y, np.complex128), K, norm)
        out[norm] = dict(Z=Z, sup=sup, count=len(sup), gaps=gaps)
    return out


def _row(kind, name, A, Y, K, **facts):
    A, Y = np.ascontiguousarray(A, np.complex128), np.ascontiguousarray(Y, np.complex128)
    return dict(kind=kind, name=name, A=A, Y=Y, K=int(K), ref=reference(A, Y, K), **facts)


def make_m8(seed, shape, name):
    N, Gr, S, K = shape
    for attempt in range(40):
        rng = np.random.default_rng(seed + attempt)
        A = axis_dictionary(N, Gr, rng).astype(np.complex128)
        atoms = np.sort(rng.choice(Gr, 4, replace=False))
        d = float(rng.uniform(1e-9, 8e-9))
        mags = {atoms[0]: 3.0, atoms[1]: 1.0, atoms[2]: 5.0, atoms[3]: 3.0 * (1.0 + d)}      # 3 (1 + d) above 3 in index
        Z0 = np.zeros((Gr, S), complex)
        for g, m in mags.items():
            Z0[g] = m * P.UNITS[rng.integers(0, 4, S)].astype(complex)
        row = _row("M8", name, A, A @ Z0, K, d=d, close=1, atoms=atoms + 1)
        ok = True
        for norm in NORMS:
            r = row["ref"][norm]
            g = r["gaps"]
            ok &= r["count"] == 4 and list(r["sup"]) == [atoms[2] + 1, atoms[3] + 1, atoms[0] + 1, atoms[1] + 1]
            ok &= len(g) == 4 and M8_GAP[0] <= g[1] <= M8_GAP[1] and min(g[0], g[2], g[3]) >= P.DECISIVE
        if ok:
            return row
    raise RuntimeError("no M8 problem found")


def exact_scale64(X, k):
    out = np.ldexp(X.real, k) + 1j * np.ldexp(X.imag, k)
    assert np.all(np.isfinite(out))
    back = np.ldexp(out.real, -k) + 1j * np.ldexp(out.imag, -k)
    assert np.array_equal(back, X) and not np.any((out == 0) & (X != 0))
    return out


def make_m9(base):
    rows = []
    for k in Y64_SCALES:
        rows.append(_row("M9", "M9y%+d" % k, base["A"], exact_scale64(base["Y"].astype(np.complex128), k), base["K"], scale_y=k,
                         base=base["name"]))
    for row in rows:
        for norm in NORMS:
            if not np.array_equal(row["ref"][norm]["sup"], base["ref"][norm]["sup"]):
                raise RuntimeError("the reference is not scale-free on %s" % row["name"])
    return rows


@functools.lru_cache(maxsize=None)
def problems():
    """dict(rows, own, shared, mixed): the rows of mmv_problems.problems() followed by the M8 and M9 rows."""
    base = P.problems()
    rows = list(base["rows"])
    rows.append(make_m8(808, (32, 24, 10, 6), "M8"))
    rows.append(make_m8(909, (300, 280, 3, 7), "M8tall"))
    rows += make_m9(rows[0])
    names = [r["name"] for r in rows]
    assert len(set(names)) == len(names)
    return dict(rows=rows, own=base["own"], shared=base["shared"], mixed=base["mixed"])


def by_name(name):
    return next(r for r in problems()["rows"] if r["name"] == name)


def decisive(row, norm):
    """every selection the reference made has a float64 gap >= GAP_MIN or exactly 0."""
    g = row["ref"][norm]["gaps"]
    return bool(np.all((g >= GAP_MIN) | (g == 0.0)))


def restate(A, Y, K, norm):
    """float64 numpy restatement of mmv_omp64_kernel: (Z, support (1-based), residual ratio ||R||^2 / ||Y||^2 at the end)."""
    A = np.asarray(A, np.complex128)
    Y = np.asarray(Y, np.complex128)
    N, Gr = A.shape
    S = Y.shape[1]
    comp = np.abs(np.concatenate([Y.real.ravel(), Y.imag.ravel()]))
    comp = comp[np.isfinite(comp)]
    ey = int(np.frexp(comp.max())[1]) if comp.size and comp.max() > 0 else 0
    R = np.ldexp(Y.real, -ey) + 1j * np.ldexp(Y.imag, -ey)
    y2 = float(np.sum(R.real ** 2 + R.imag ** 2))
    kmax = min(K, N, Gr)
    Q = np.zeros((N, kmax), complex)
    Rt = np.zeros((kmax, kmax), complex)
    T = np.zeros((kmax, S), complex)
    sup, taken, r2 = [], np.zeros(Gr, bool), y2
    for k in range(kmax):
        C = A.conj().T @ R
        c2 = C.real ** 2 + C.imag ** 2
        score = np.sum(np.sqrt(c2), axis=1) if norm == "l1" else np.sum(c2, axis=1)
        score[taken] = -1.0
        score[np.isnan(score)] = -2.0
        g = int(np.argmax(score))
        if not (score[g] > -1.0):                              # every candidate taken or NaN
            break
        q = A[:, g].copy()
        n0 = float(np.vdot(q, q).real)
        for _ in range(2):
            if k:
                d = Q[:, :k].conj().T @ q
                q = q - Q[:, :k] @ d
                Rt[:k, k] += d
        n1 = float(np.vdot(q, q).real)
        if not (n1 > 1e-10 * n0) or not (n0 > 0.0):
            break
        Q[:, k] = q / np.sqrt(n1)
        Rt[k, k] = np.sqrt(n1)
        sup.append(g)
        taken[g] = True
        T[k] = Q[:, k].conj() @ R
        R = R - np.outer(Q[:, k], T[k])
        r2 = float(np.sum(R.real ** 2 + R.imag ** 2))
        if r2 <= 1e-12 * y2:
            break
    n = len(sup)
    Z = np.zeros((Gr, S), complex)
    if n:
        coef = np.zeros((n, S), complex)
        for r in range(n - 1, -1, -1):
            coef[r] = (T[r] - Rt[r, r + 1:n] @ coef[r + 1:n]) / Rt[r, r].real
        Z[sup] = np.ldexp(coef.real, ey) + 1j * np.ldexp(coef.imag, ey)
    return Z, np.array(sup, np.int64) + 1, (r2 / y2 if y2 > 0 else 0.0)
