"""OMP problems for jstsp_omp_f64 / jstsp_omp_kron_f64 (csrc/omp64.hip), seeded and CPU only: the engineered rows of
tests/omp_problems.py (E1-E6, complex64 values) plus rows that only float64 can express, on the same dictionaries:

- D1 near-tie: at iteration 1 two atoms p < q lead every other atom by far and their |Phi' v| differ by a float64 relative gap
  inside D1_GAP = [1e-9, 1e-8] - below a fifth of an fp32 ulp, and seven decades above the float64 round-off of the correlation.
  ``D1hi`` is won by q (the higher index), ``D1lo`` by p.  v is complex128 and is NOT rounded to complex64 (rounded, the pair is
  decided by the rounding).  Later iterations are decisive (gap >= omp_problems.DECISIVE) or exact ties.
- D2 scale: the E1 problem with v * 2^k, k = +-400 - no complex64 value; the index set is E1's and x_hat is E1's times 2^k.

Every row carries the float64 literal reference (``omp_problems.reference``) of its own values, and the generator asserts the gap
ranges itself.  ``dense_groups`` / ``kron_groups`` return the groups of omp_problems with the D rows added to the main group."""
import functools

import numpy as np

import omp_problems as P

D1_GAP = (1e-9, 1e-8)
GAP_MIN = 1e-9                        # the float64 relative gap above which the device must select what the reference selects
V64_SCALES = (-400, 400)
DENSE = [(96, 160, 10), (100, 300, 8)]            # the smallest shape of tests/test_gpu_omp_paths.py; measures not a multiple of 64, size_d > 256
KRON = [(8, 16, 8, 16, 24)]


def _row128(Phi64, v, m, kind, **facts):
    v = np.asarray(v, np.complex128)
    return dict(v=v, kind=kind, ref=P.reference(Phi64, v, m), **facts)


def decisive(row):
    """every selection of the row's reference has a float64 relative gap >= GAP_MIN or exactly 0"""
    g = row["ref"]["gaps"]
    return bool(np.all((g >= GAP_MIN) | (g == 0.0)))


def make_d1(Phi64, m, rng, high_wins, tries=400):
    """atoms p < q lead iteration 1 and differ by a relative gap inside D1_GAP; the winner is q if high_wins else p.
    v = 6 a_p e^{i phi} + b a_q e^{i psi} + (smaller atoms) + noise, the real b solved by bisection in float64."""
    meas, size_d = Phi64.shape
    for _ in range(tries):
        p, q = (int(i) for i in np.sort(rng.choice(size_d, 2, replace=False)))
        ap, aq = Phi64[:, p], Phi64[:, q]
        rest = P._sparse(Phi64, rng, P._pick(rng, size_d, 3, {p, q}), [0.6, 0.45, 0.3]) + P._noise(rng, meas, 0.2)
        base, dq = 6.0 * P._phase(rng) * ap + rest, P._phase(rng) * aq
        t = rng.uniform(2.5e-9, 7e-9)

        def f(b):
            c = np.abs(np.array([ap.conj() @ (base + b * dq), aq.conj() @ (base + b * dq)]))
            want = t * c.max()
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
        v = base + 0.5 * (lo + hi) * dq
        c = P.first_corr(Phi64, v)
        win, lose = (q, p) if high_wins else (p, q)
        if not np.delete(c, [p, q]).max() < 0.8 * c[lose]:
            continue
        row = _row128(Phi64, v, m, "D1hi" if high_wins else "D1lo", p=p, q=q, winner=win)
        g = row["ref"]["gaps"]
        if row["ref"]["idx"][0] == win + 1 and D1_GAP[0] <= g[0] <= D1_GAP[1] and np.all((g[1:] >= P.DECISIVE) | (g[1:] == 0.0)):
            return row
    raise RuntimeError("no D1 problem found")


def _with_d_rows(groups, m, seed):
    main = groups[0]
    assert main["name"] == "main"
    rng = np.random.default_rng(seed + 64)
    Phi64 = main["Phi64"]
    rows = dict(main["rows"])
    rows["D1hi"] = make_d1(Phi64, m, rng, True)
    rows["D1lo"] = make_d1(Phi64, m, rng, False)
    for r in (rows["D1hi"], rows["D1lo"]):                        # the facts the GPU test relies on, asserted where they are made
        g = r["ref"]["gaps"]
        assert D1_GAP[0] <= g[0] <= D1_GAP[1] and r["ref"]["idx"][0] == r["winner"] + 1 and r["p"] < r["q"]
        assert np.all((g[1:] >= P.DECISIVE) | (g[1:] == 0.0))
    e1 = rows["E1"]
    for k in V64_SCALES:
        r = rows["D2v%+d" % k] = _row128(Phi64, e1["v"].astype(np.complex128) * 2.0 ** k, m, "D2", scale_v=k)
        assert np.array_equal(r["ref"]["idx"], e1["ref"]["idx"]) and np.all(np.isfinite(r["v"]))
    return [dict(main, rows=rows)] + list(groups[1:])


@functools.lru_cache(maxsize=None)
def dense_groups(shape):
    meas, size_d, m = shape
    return _with_d_rows(P.dense_groups(meas, size_d, m, seed=sum(shape)), m, sum(shape))


@functools.lru_cache(maxsize=None)
def kron_groups(shape):
    N, M, Gr, G2, m = shape
    return _with_d_rows(P.kron_groups(N, M, Gr, G2, m, seed=sum(shape)), m, sum(shape))


def all_rows():
    """(tag, group, row name, row) over every shape of the set"""
    for shape in DENSE:
        for G in dense_groups(shape):
            for n, r in G["rows"].items():
                yield ("dense%s" % (shape,), G, n, r)
    for shape in KRON:
        for G in kron_groups(shape):
            for n, r in G["rows"].items():
                yield ("kron%s" % (shape,), G, n, r)
