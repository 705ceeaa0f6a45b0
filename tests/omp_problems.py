"""Engineered OMP problems for the selection step of OMP.m:17 (``[~, idx] = max(abs(A'*r))``), seeded and CPU only.

Every array is complex64, and the float64 reference (``oracle.solvers.omp_literal_margins``) is run on exactly those
values, so what a device receives and what the reference solves are the same problem.  The kinds:

- E1 random: a sparse signal plus noise; every iteration decisive (float64 relative gap of the top two >= DECISIVE).
- E2 exact ties: two later columns equal to column j and to -column j; j wins iteration 1 with a float64 gap of 0.
- E3 near-ties: at iteration 1 two atoms p < q lead every other atom by far and differ by 1 to 4 fp32 ulps in float64;
  ``E3hi`` is won by q (the higher index), ``E3lo`` by p.  Later iterations decisive.
- E4 zero residual: an axis-aligned dictionary (columns are unit-modulus multiples of distinct unit vectors), v in the
  span of s < m atoms, so the residual is exactly 0 in fp32 and in float64 after s iterations and the next selection
  is index 1, as MATLAB's max of zeros.  ``E4a``: atom 1 is in the support (s = m - 1): the re-selection is a duplicate
  and pinv splits its coefficient.  ``E4b``: atom 1 is not (s = m - 2): it enters with coefficient 0, then is
  re-selected.  (Once targetMatrix holds a duplicate column, pinv leaves a float64 residual at 1e-16 instead of 0 and
  the literal reference's later picks are noise, so no zero-residual iteration follows a duplicate here.)
- E5 v = 0: index set all ones, x_hat = 0.
- E6 scale: the E1 problem with v * 2^k (k in +-70, +-100) and with the dictionary * 2^k (k = +-40); powers of two are
  exact, so the index set is E1's and x_hat is E1's times the exact factor.

Dense sets come from ``dense_groups``, Kronecker sets (Phi = kron(Bf.', Af), built from the factors) from ``kron_groups``.
A group is one dictionary with its rows; every row carries the float64 reference of its own values."""
import numpy as np

from oracle import solvers as O

DECISIVE = 1e-4                       # float64 relative gap of a selection no fp32 kernel may get wrong
V_SCALES = (-100, -70, 70, 100)
A_SCALES = (-40, 40)


def _c(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def _phase(rng, n=None):
    return np.exp(2j * np.pi * rng.random(n))


def reference(Phi, v, m):
    """float64 OMP.m on the given complex64 values: dict(x, idx, T, gaps)."""
    x, idx, _, T, gaps = O.omp_literal_margins(np.asarray(Phi, np.complex128), np.asarray(v, np.complex128), m)
    return dict(x=x, idx=idx, T=T, gaps=gaps)


def first_corr(Phi, v):
    """|Phi' v| exactly as the reference's first iteration computes it."""
    return np.abs(np.asarray(Phi, np.complex128).conj().T @ np.asarray(v, np.complex128))


def ulp32(x):
    return float(np.spacing(np.float32(x)))


def _row(Phi, v, m, kind, **facts):
    return dict(v=v.astype(np.complex64), kind=kind, ref=reference(Phi, v.astype(np.complex64), m), **facts)


def _sparse(Phi64, rng, atoms, mags):
    x = np.zeros(Phi64.shape[1], complex)
    x[atoms] = np.asarray(mags) * _phase(rng, len(atoms))
    return Phi64 @ x


def _pick(rng, n, k, avoid):
    pool = np.setdiff1d(np.arange(n), np.asarray(sorted(avoid), dtype=np.int64))
    return rng.choice(pool, k, replace=False)


def _noise(rng, meas, level):
    return level * _c(rng, meas) / np.sqrt(2 * meas)


def make_e1(Phi64, m, rng, avoid, tries=400):
    meas, size_d = Phi64.shape
    for _ in range(tries):
        v = _sparse(Phi64, rng, _pick(rng, size_d, 6, avoid), [3.0, 2.6, 2.2, 1.8, 1.4, 1.0]) + _noise(rng, meas, 0.3)
        row = _row(Phi64, v, m, "E1")
        if row["ref"]["gaps"].min() >= DECISIVE:
            return row
    raise RuntimeError("no decisive E1 problem found")


def make_e2(Phi64, m, rng, j, copies, avoid, tries=400):
    """column j wins iteration 1 in a bit-exact tie with its copies (all at higher indices).  A later iteration is
    decisive or is again an exact tie (a copy and its column: |corr| bit-equal, so the first index is defined)."""
    meas, size_d = Phi64.shape
    for _ in range(tries):
        v = 3.0 * _phase(rng) * Phi64[:, j] + _sparse(Phi64, rng, _pick(rng, size_d, 4, avoid), [1.6, 1.3, 1.0, 0.8]) \
            + _noise(rng, meas, 0.3)
        row = _row(Phi64, v, m, "E2", j=j, copies=list(copies))
        g = row["ref"]["gaps"]
        if row["ref"]["idx"][0] == j + 1 and g[0] == 0.0 and np.all((g[1:] >= DECISIVE) | (g[1:] == 0.0)):
            return row
    raise RuntimeError("no E2 problem found")


def make_e3(Phi64, m, rng, p, q, high_wins, avoid, tries=400):
    """atoms p < q lead iteration 1 and differ by 1..4 fp32 ulps (float64); the winner is q if high_wins else p.
    v = 6 a_p e^{i phi} + b a_q e^{i psi} + (smaller atoms) + noise, with the real b solved by bisection for the wanted
    ratio |c_q| / |c_p| and v rounded to complex64 afterwards (a draw whose rounded gap leaves the range is redrawn)."""
    meas, size_d = Phi64.shape
    ap, aq = Phi64[:, p], Phi64[:, q]
    for _ in range(tries):
        rest = _sparse(Phi64, rng, _pick(rng, size_d, 3, avoid), [0.6, 0.45, 0.3]) + _noise(rng, meas, 0.2)
        base, dq = 6.0 * _phase(rng) * ap + rest, _phase(rng) * aq
        t = rng.uniform(1.5, 3.5)

        def f(b):
            c = np.abs(np.array([ap.conj() @ (base + b * dq), aq.conj() @ (base + b * dq)]))
            want = t * ulp32(c.max())
            return (c[1] - c[0] - want) if high_wins else (c[0] - c[1] - want)

        lo, hi = (0.0, 100.0) if high_wins else (100.0, 0.0)        # f(lo) < 0 < f(hi)
        if not (f(lo) < 0 < f(hi)):
            continue
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if f(mid) < 0:
                lo = mid
            else:
                hi = mid
        v = (base + 0.5 * (lo + hi) * dq).astype(np.complex64)
        c = first_corr(Phi64, v)
        win, lose = (q, p) if high_wins else (p, q)
        third = np.delete(c, [p, q]).max()
        gap_ulps = (c[win] - c[lose]) / ulp32(c[win])
        if not (1.0 <= gap_ulps <= 4.0 and third < 0.8 * c[lose]):
            continue
        row = _row(Phi64, v, m, "E3hi" if high_wins else "E3lo", p=p, q=q, winner=win, gap_ulps=gap_ulps)
        g = row["ref"]["gaps"]
        if row["ref"]["idx"][0] == win + 1 and g[1:].min() >= DECISIVE:
            return row
    raise RuntimeError("no E3 problem found")


def axis_dictionary(rows, cols, rng):
    """column i = (one of 1, -1, 1j, -1j) * e_{perm(i)}: orthonormal, and Gram-Schmidt on it is exact in fp32."""
    assert cols <= rows
    D = np.zeros((rows, cols), np.complex64)
    D[rng.permutation(rows)[:cols], np.arange(cols)] = np.array([1, -1, 1j, -1j], np.complex64)[rng.integers(0, 4, cols)]
    return D


def make_e4(Phi64, m, rng, with_atom1):
    """v in the span of s atoms of an axis-aligned dictionary, magnitudes distinct by >= 1 % (decisive)."""
    size_d = Phi64.shape[1]
    s = m - 1 if with_atom1 else m - 2
    assert 1 <= s < size_d
    atoms = rng.choice(np.arange(1, size_d), s - 1 if with_atom1 else s, replace=False)
    if with_atom1:
        atoms = np.concatenate([[0], atoms])
    mags = rng.permutation(np.linspace(1.0, 2.0 + 0.02 * s, s)).astype(np.float32)
    x = np.zeros(size_d, np.complex64)
    x[atoms] = mags * np.array([1, -1, 1j, -1j], np.complex64)[rng.integers(0, 4, s)]
    v = (Phi64 @ x.astype(complex)).astype(np.complex64)          # exact: one nonzero term per entry
    return _row(Phi64, v, m, "E4a" if with_atom1 else "E4b", support=np.sort(atoms), s=s)


def e4_residual_norms(Phi64, v, idx):
    """max |r| after each iteration of the literal reference (pinv of the selected columns) on the row's values."""
    Phi64, v = np.asarray(Phi64, np.complex128), np.asarray(v, np.complex128)
    out = []
    for k in range(1, len(idx) + 1):
        T = Phi64[:, np.asarray(idx[:k]) - 1]
        out.append(float(np.max(np.abs(v - T @ (np.linalg.pinv(T) @ v)))))
    return np.array(out)


def _groups(Phi_of, factors_of, m, rng, tie_cols, pairs, ident_factors, tie_dict=None, tie_avoid=()):
    """the dictionaries of a set: main (E1, E2, E3hi, E3lo, E5, E6 on v), ident (E4a, E4b), main * 2^+-40, and with
    ``tie_dict`` a dictionary of its own for E2 (random supports avoid ``tie_avoid`` there).  Random supports avoid the
    engineered atoms."""
    main = factors_of(1.0)
    Phi64 = Phi_of(main)
    meas = Phi64.shape[0]
    j, copies = tie_cols
    special = {*pairs[0], *pairs[1]} | (set() if tie_dict is not None else {j, *copies})
    rows = {}
    rows["E1"] = e1 = make_e1(Phi64, m, rng, special)
    if tie_dict is None:
        rows["E2"] = make_e2(Phi64, m, rng, j, copies, special)
    for name, pair, high in (("E3hi", pairs[0], True), ("E3lo", pairs[1], False)):
        for attempt in range(20):                     # (a pair too coherent with its neighbours: the next free pair)
            try:
                rows[name] = make_e3(Phi64, m, rng, *pair, high, special, tries=100)
                break
            except RuntimeError:
                pair = tuple(int(i) for i in np.sort(_pick(rng, Phi64.shape[1], 2, special)))
                special |= set(pair)
        else:
            raise RuntimeError("no %s problem found" % name)
    rows["E5"] = _row(Phi64, np.zeros(meas, np.complex64), m, "E5")
    for k in V_SCALES:
        rows["E6v%+d" % k] = _row(Phi64, e1["v"] * np.float32(2.0 ** k), m, "E6", scale_v=k)
    groups = [dict(name="main", dict=main, Phi64=Phi64, rows=rows)]
    idict = ident_factors()
    iPhi = Phi_of(idict)
    groups.append(dict(name="ident", dict=idict, Phi64=iPhi,
                       rows={"E4a": make_e4(iPhi, m, rng, True), "E4b": make_e4(iPhi, m, rng, False)}))
    for k in A_SCALES:
        sc = factors_of(2.0 ** k)
        sPhi = Phi_of(sc)
        groups.append(dict(name="A%+d" % k, dict=sc, Phi64=sPhi,
                           rows={"E6A%+d" % k: _row(sPhi, e1["v"], m, "E6", scale_A=k)}))
    if tie_dict is not None:
        tPhi = Phi_of(tie_dict)
        groups.append(dict(name="tie", dict=tie_dict, Phi64=tPhi,
                           rows={"E2": make_e2(tPhi, m, rng, j, copies, {j, *copies, *tie_avoid})}))
    return groups


def dense_groups(meas, size_d, m, seed):
    """dictionaries meas x size_d (the axis-aligned one meas x min(size_d, meas)); dict = A (complex64)."""
    rng = np.random.default_rng(seed)
    A = (_c(rng, meas, size_d) / np.sqrt(meas)).astype(np.complex64)
    cols = rng.choice(size_d, 7, replace=False)
    j, k1, k2 = np.sort(cols[:3])
    A[:, k1] = A[:, j]
    A[:, k2] = -A[:, j]
    pairs = [tuple(np.sort(cols[3:5])), tuple(np.sort(cols[5:7]))]
    return _groups(lambda a: np.asarray(a, np.complex128),
                   lambda s: (A * np.float32(s)).astype(np.complex64), m, rng, (int(j), (int(k1), int(k2))),
                   [tuple(int(i) for i in p) for p in pairs],
                   lambda: axis_dictionary(meas, min(size_d, meas), rng))


def kron_phi(f):
    Af, Bf = f
    return np.kron(np.asarray(Bf, np.complex128).T, np.asarray(Af, np.complex128))


def kron_groups(N, M, Gr, G2, m, seed):
    """Phi = kron(Bf.', Af), atom g + Gr h = vec(Af(:, g) Bf(h, :)); dict = (Af, Bf).  E2 (a dictionary of its own): two
    rows of Bf equal to row h0 and to -row h0, so atom (g, h0) ties with (g, h1) and (g, h2) for every g (copies in Bf rather
    than Af keep the rank, Gr (G2 - 2), above m at the test shapes: beyond the rank the residual is round-off and the
    reference's picks are noise); E4: Af and Bf axis-aligned (Gr <= N, G2 <= M)."""
    rng = np.random.default_rng(seed)
    Af = (_c(rng, N, Gr) / np.sqrt(N)).astype(np.complex64)
    Bf = (_c(rng, G2, M) / np.sqrt(M)).astype(np.complex64)
    h0, h1, h2 = (int(i) for i in np.sort(rng.choice(G2, 3, replace=False)))
    Bft = Bf.copy()
    Bft[h1] = Bft[h0]
    Bft[h2] = -Bft[h0]
    g = int(rng.integers(0, Gr))
    p = np.sort(rng.choice(Gr * G2, 4, replace=False))
    pairs = [(int(p[0]), int(p[1])), (int(p[2]), int(p[3]))]
    ties = (g + Gr * h0, (g + Gr * h1, g + Gr * h2))
    tied = {gg + Gr * hh for gg in range(Gr) for hh in (h0, h1, h2)}      # every atom built on the shared row
    return _groups(kron_phi, lambda s: ((Af * np.float32(s)).astype(np.complex64), Bf), m, rng, ties, pairs,
                   lambda: (axis_dictionary(N, Gr, rng), axis_dictionary(M, G2, rng).T.copy()), tie_dict=(Af, Bft),
                   tie_avoid=tied)
