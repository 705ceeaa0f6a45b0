"""Engineered joint (MMV) OMP problems for jstsp_mmv_omp_c32 (csrc/mmv_omp.hip), seeded and CPU only.

Every array is complex64 and the float64 reference (``oracle.solvers.mmv_omp_margins``) is run on exactly those values, for
both row scores (``l2``, ``l1``): what a device receives and what the reference solves are the same problem.  A row is
``dict(kind, name, A (N x Gr), Y (N x S), K, ref={norm: dict(Z, sup, count, gaps)}, facts...)``.  The kinds:

- M1 random decisive: row-sparse truth plus noise at the shapes of ``M1_SHAPES`` (every score split of the kernel: one to
  256 column groups, one or several atom passes - the support then holds an atom of the last pass -, block-strided loops
  with N > 256, S > 256, N = 1, Gr = 1), plus a batch of
  three problems at the first shape with dictionaries of their own and three on a shared dictionary.  Every selection has
  a float64 relative gap >= DECISIVE and cond(A[:, support]) <= COND_MAX.
- M2 exact ties: later columns equal to column j, to -column j and to 1i * column j; j wins iteration 1 with a float64 gap
  of exactly 0, later iterations are decisive.
- M3 early stop, exact: an axis-aligned dictionary (omp_problems.axis_dictionary), Y in the span of s < K atoms with
  Gaussian-integer coefficients: the residual is exactly 0 in fp32 and float64 after s atoms; ``Z_exact`` is the answer.
- M4 early stop, random noiseless: Y = A Z0 rounded to complex64, s < K rows; the reference stops at s.
- M5 dependent atom: A = (N x r)(r x Gr) rounded to complex64 with r < K and Y random: the reference stops with count r
  (``M5b``: two exactly equal columns, the first of them planted in Y, so iteration 1 is an exact tie as well).
- M6 zero input: Y = 0: support [1], count 1, Z = 0.
- M7 scale: the first M1 problem with Y * 2^k (k in Y_SCALES) and with A * 2^k (k in A_SCALES): exact in complex64, and the
  reference, run on the scaled values, selects the unscaled support."""
import functools

import numpy as np

from oracle import solvers as O
from omp_problems import axis_dictionary

DECISIVE = 1e-3                       # float64 relative gap of a selection no fp32 kernel may get wrong
COND_MAX = 100.0
Y_SCALES = (-100, -70, 70, 100)
A_SCALES = (-40, 40)
NORMS = ("l2", "l1")
M1_SHAPES = [(32, 32, 16, 6), (24, 40, 70, 10), (64, 300, 40, 10), (128, 128, 140, 12), (300, 513, 3, 9), (16, 4096, 5, 6),
             (64, 256, 1, 5), (64, 257, 300, 8), (8, 1, 4, 3), (1, 5, 3, 2)]
COUNTS = {"M1": len(M1_SHAPES) + 6, "M2": 2, "M3": 2, "M4": 2, "M5": 2, "M6": 2, "M7": len(Y_SCALES) + len(A_SCALES)}
TRIES = 60
UNITS = np.array([1, -1, 1j, -1j], np.complex64)


def _c(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def reference(A, Y, K):
    """float64 joint OMP on the given complex64 values, per row score: dict(Z, sup, count, gaps)."""
    out = {}
    for norm in NORMS:
        Z, sup, gaps = O.mmv_omp_margins(np.asarray(A, np.complex128), np.asarray(Y, np.complex128), K, norm)
        out[norm] = dict(Z=Z, sup=sup, count=len(sup), gaps=gaps)
    return out


def support_cond(A, sup):
    return float(np.linalg.cond(np.asarray(A, np.complex128)[:, np.asarray(sup) - 1])) if len(sup) else 1.0


def _row(kind, name, A, Y, K, **facts):
    A, Y = np.ascontiguousarray(A, np.complex64), np.ascontiguousarray(Y, np.complex64)
    return dict(kind=kind, name=name, A=A, Y=Y, K=int(K), ref=reference(A, Y, K), **facts)


def _decisive(row, first=0, upto=None):
    """every selection from ``first`` on (up to ``upto``) has a gap >= DECISIVE and the support is well conditioned."""
    for norm in NORMS:
        r = row["ref"][norm]
        g = r["gaps"][first:upto]
        if len(g) and g.min() < DECISIVE:
            return False
        if support_cond(row["A"], r["sup"]) > COND_MAX:
            return False
    return True


def _dictionary(rng, N, Gr):
    return (_c(rng, N, Gr) / np.sqrt(2 * N)).astype(np.complex64)


def last_pass(Gr):
    """0-based atoms of the kernel's last atom pass (passes of 256 atoms; all atoms when there is one pass)."""
    return np.arange(256 * ((Gr - 1) // 256), Gr)


def _truth(rng, A, S, rows, amp=3.0, noise=0.05):
    """row-sparse truth plus noise; beyond 256 atoms one of the rows is an atom of the last atom pass."""
    N, Gr = A.shape
    Z0 = np.zeros((Gr, S), complex)
    atoms = rng.choice(Gr, rows, replace=False)
    if Gr > 256 and not np.isin(atoms, last_pass(Gr)).any():
        atoms[0] = rng.choice(last_pass(Gr))
    Z0[atoms] = amp * _c(rng, rows, S)
    return A.astype(np.complex128) @ Z0 + noise * _c(rng, N, S)


def make_m1(rng, shape, name, A=None):
    N, Gr, S, K = shape
    for _ in range(TRIES):
        D = _dictionary(rng, N, Gr) if A is None else A
        row = _row("M1", name, D, _truth(rng, D, S, min(4, N, Gr)), K, shape=shape)
        wide = Gr <= 256 or all(np.isin(row["ref"][n]["sup"] - 1, last_pass(Gr)).any() for n in NORMS)
        if wide and _decisive(row):
            return row
    raise RuntimeError("no decisive M1 problem found at %s" % (shape,))


def make_m2(rng, shape, name):
    """column j < k1 < k2 < k3 with A[:, k1] = A[:, j], A[:, k2] = -A[:, j], A[:, k3] = 1i * A[:, j] (exact in complex64)."""
    N, Gr, S, K = shape
    for _ in range(TRIES):
        A = _dictionary(rng, N, Gr)
        j, k1, k2, k3 = (int(i) for i in np.sort(rng.choice(Gr, 4, replace=False)))
        A[:, k1] = A[:, j]
        A[:, k2] = -A[:, j]
        A[:, k3] = np.complex64(1j) * A[:, j]
        Y = _truth(rng, A, S, 3, amp=1.5)
        Y += 8.0 * np.outer(A[:, j].astype(complex), _c(rng, S))
        row = _row("M2", name, A, Y, K, j=j, copies=[k1, k2, k3])
        ok = True
        for norm in NORMS:
            r = row["ref"][norm]
            ok &= r["sup"][0] == j + 1 and r["gaps"][0] == 0.0
        if ok and _decisive(row, first=1):
            return row
    raise RuntimeError("no M2 problem found")


def make_m3(rng, shape, s, name):
    N, Gr, S, K = shape
    assert s < K and s < Gr <= N
    A = axis_dictionary(N, Gr, rng)
    atoms = rng.choice(Gr, s, replace=False)
    mags = rng.permutation(np.arange(1, s + 1)).astype(np.float32)           # row scores S m^2 (l2), S m (l1): decisive
    Z = np.zeros((Gr, S), np.complex64)
    Z[atoms] = mags[:, None] * UNITS[rng.integers(0, 4, (s, S))]
    Y = (A.astype(complex) @ Z.astype(complex)).astype(np.complex64)        # exact: one nonzero term per entry
    return _row("M3", name, A, Y, K, s=s, Z_exact=Z, atoms=atoms[np.argsort(-mags)] + 1)


def make_m4(rng, shape, s, name):
    N, Gr, S, K = shape
    assert s < K
    for _ in range(TRIES):
        A = _dictionary(rng, N, Gr)
        row = _row("M4", name, A, _truth(rng, A, S, s, noise=0.0), K, s=s)
        if all(row["ref"][n]["count"] == s for n in NORMS) and _decisive(row, upto=s):
            return row
    raise RuntimeError("no M4 problem found")


def make_m5(rng, shape, r, twin, name):
    """A of rank r (rounded to complex64: the other singular values are at 1e-7); ``twin``: column q > p equal to column p
    and Y with a strong component on it, so p wins iteration 1 in an exact tie with q."""
    N, Gr, S, K = shape
    assert r < K and r < min(N, Gr)
    for _ in range(TRIES):
        A = ((_c(rng, N, r) @ _c(rng, r, Gr)) / np.sqrt(4 * N * r)).astype(np.complex64)
        Y = _c(rng, N, S)
        facts = {}
        if twin:
            p, q = (int(i) for i in np.sort(rng.choice(Gr, 2, replace=False)))
            A[:, q] = A[:, p]
            Y = Y + 6.0 * np.outer(A[:, p].astype(complex) / np.linalg.norm(A[:, p]), _c(rng, S))
            facts = dict(p=p, q=q)
        row = _row("M5", name, A, Y, K, r=r, **facts)
        ok = all(row["ref"][n]["count"] == r for n in NORMS)
        if twin:
            ok = ok and all(row["ref"][n]["sup"][0] == p + 1 and row["ref"][n]["gaps"][0] == 0.0 for n in NORMS)
        if ok and _decisive(row, first=1 if twin else 0, upto=r):
            return row
    raise RuntimeError("no M5 problem found")


def make_m6(rng, shape, name):
    N, Gr, S, K = shape
    return _row("M6", name, _dictionary(rng, N, Gr), np.zeros((N, S), np.complex64), K)


def exact_scale(X, k):
    """X * 2^k in complex64, asserted exact (no rounding, overflow or lost bits) against float64."""
    out = (X * np.float32(2.0) ** np.float32(k)).astype(np.complex64)
    assert np.float32(2.0) ** np.float32(k) == 2.0 ** k
    assert np.all(np.isfinite(out)) and np.array_equal(out.astype(np.complex128), X.astype(np.complex128) * 2.0 ** k)
    return out


def make_m7(base):
    rows = []
    for k in Y_SCALES:
        rows.append(_row("M7", "M7y%+d" % k, base["A"], exact_scale(base["Y"], k), base["K"], scale_y=k, base=base["name"]))
    for k in A_SCALES:
        rows.append(_row("M7", "M7a%+d" % k, exact_scale(base["A"], k), base["Y"], base["K"], scale_a=k, base=base["name"]))
    for row in rows:
        for norm in NORMS:
            if not np.array_equal(row["ref"][norm]["sup"], base["ref"][norm]["sup"]):
                raise RuntimeError("the reference is not scale-free on %s" % row["name"])
    return rows


@functools.lru_cache(maxsize=None)
def problems(seed=2024):
    """the whole set: dict(rows=[...], own=[names], shared=[names], mixed=[names]) - ``own`` are the three M1 problems with
    dictionaries of their own (one batch, also with strideA = N Gr + 7), ``shared`` the three on the dictionary of the first
    M1 row (as are the M7 rows with a scaled Y), ``mixed`` one row of each early-stop kind at one shape and K."""
    rng = np.random.default_rng(seed)
    rows = [make_m1(rng, shape, "M1_%dx%dx%d_K%d" % shape) for shape in M1_SHAPES]
    own = [make_m1(rng, M1_SHAPES[0], "M1own%d" % i) for i in range(3)]
    shared = [make_m1(rng, M1_SHAPES[0], "M1shared%d" % i, A=rows[0]["A"]) for i in range(3)]
    rows += own + shared
    rows.append(make_m2(rng, (32, 48, 12, 6), "M2"))
    rows.append(make_m2(rng, (40, 300, 9, 5), "M2wide"))
    rows.append(make_m3(rng, (32, 24, 10, 8), 5, "M3"))
    rows.append(make_m3(rng, (300, 280, 3, 6), 3, "M3tall"))
    rows.append(make_m4(rng, (32, 48, 12, 6), 3, "M4"))
    rows.append(make_m4(rng, (64, 300, 20, 8), 4, "M4wide"))
    rows.append(make_m5(rng, (32, 48, 12, 6), 5, False, "M5"))
    rows.append(make_m5(rng, (32, 48, 12, 6), 5, True, "M5b"))
    rows.append(make_m6(rng, (32, 48, 12, 6), "M6"))
    rows.append(make_m6(rng, (16, 300, 3, 4), "M6wide"))
    rows += make_m7(rows[0])
    names = [r["name"] for r in rows]
    assert len(set(names)) == len(names)
    return dict(rows=rows, own=[r["name"] for r in own], shared=[r["name"] for r in shared],
                mixed=["M2", "M4", "M5", "M5b", "M6"])


def by_name(name, seed=2024):
    return next(r for r in problems(seed)["rows"] if r["name"] == name)
