"""CPU checks of tests/svd64_tall_problems.py, the numpy restatement of the QR route of jstsp_svd_tall_f64: it is an SVD (against
numpy.linalg.svd on the small shapes), its recomputed worst error measures do not exceed the recorded ones from which
tests/test_gpu_svd64_tall.py takes its bounds (tests/golden/svd64_tall_restatement_worst.json), and on the graded class its
long-side factor is orthonormal to rounding level - which neither A V Sigma^-1 nor the back-application without the correction is.

The rounding-level ceiling for max |L^H L - I|, a priori: a column of the long-side factor meets n reflectors per chunk and at most
30 (n - 1) rotations of the Jacobi; one rounding of a complex operation each, 2^-52, added linearly, times 4 (the form of
svd64_problems.ceiling).  Measured on the graded class (sigma over 12 decades): restatement 2e-15 .. 1.1e-14; without the
correction 4e-10 .. 8e-10 at n >= 48 and 1.1e-11 at 9000 x 33 (second order in eps sigma_1 / sigma_k); A V Sigma^-1 2e-4 .. 4e-4
(first order)."""
import numpy as np
import pytest

import spectrum_problems as P
import svd64_problems as S
import svd64_tall_problems as T

GRADED_SHAPES = [(128, 48), (129, 49), (200, 64), (64, 200), (9000, 33)]


def rounding_ceiling(rows, cols):
    m, n = max(rows, cols), min(rows, cols)
    return 4.0 * (n * (-(-m // T.tq_chunk(n))) + S.SWEEP_CAP["lds"] * max(n - 1, 1)) * 2.0 ** -52


def test_restatement_is_an_svd_on_the_small_shapes():
    bd = T.bounds()
    for rows, cols, name, mine, nump, conv, dropped in T.small_records():
        assert conv, (rows, cols, name)
        for k in ("e_sv", "e_rec", "e_long", "e_short"):
            assert mine[k] <= bd[k], (rows, cols, name, k, mine[k], bd[k])
            assert nump[k] <= bd[k], (rows, cols, name, k, nump[k], bd[k])           # numpy's own SVD meets the bounds
        if not dropped:
            assert mine["e_rec"] <= bd["e_rec_nothing_dropped"] and nump["e_rec"] <= bd["e_rec_nothing_dropped"], (rows, cols, name)
        assert mine["e_long"] <= rounding_ceiling(rows, cols) and mine["e_short"] <= rounding_ceiling(rows, cols), (rows, cols, name)
    assert [r[:3] for r in T.small_records() if r[6]] == [(9000, 33, "graded")]


def test_recomputed_worst_values_are_the_recorded_ones():
    """The worst values recomputed over the small shapes against the fixture's record of the SAME shapes (its all-shapes entry
    also holds the 64 x 65536 matrix, whose e_long is 9 x larger and would hide a drift).  Two-sided: a stale fixture or a changed
    restatement is caught either way.  The factor 1.5 is a deliberate allowance, as in tests/test_svd64_problems.py: numpy's sums
    may differ in the last bits from one build to another, and with them the pairs that still rotate in the last sweeps.  The
    all-shapes record, from which the GPU bounds come, is never below the small-shape one."""
    got, rec, bd = T.recomputed_worst(), T.recorded_small(), T.bounds()
    for k in ("e_sv", "e_rec", "e_long", "e_short", "e_rec_nothing_dropped"):
        print("%s: restatement over the small shapes %.3g, recorded %.3g" % (k, got[k], rec[k]))
        assert rec[k] / 1.5 <= got[k] <= rec[k] * 1.5, (k, got[k], rec[k])
        if k != "e_sv":
            assert T.MARGIN * rec[k] <= bd[k], (k, rec[k], bd[k])
    assert got["e_sv"] <= T.QR_TOL and bd["e_sv"] == T.QR_TOL
    assert bd["e_rec_nothing_dropped"] <= rounding_ceiling(64, 65536)


@pytest.mark.parametrize("rows,cols", [(9000, 33), (200, 64), (3, 5)])
def test_rank_zero_columns_edge_cases_and_the_swap(rows, cols):
    for name, A in T.classes(rows, cols):
        ref = P.ref(A)
        U, sv, V, rank, conv = T.tsqr_svd_ref(A)
        thr = S.drop_threshold(rows, cols, ref[:, 0])[:, None]
        assert not np.any((ref > thr / T.CLEAR) & (ref < thr * T.CLEAR)), (rows, cols, name)
        assert np.array_equal(rank, np.sum(ref > thr, axis=1)), (name, rank)
        if (rows, cols, name) == (9000, 33, "rank6"):
            assert np.all(rank == 6)
        long = U if rows >= cols else V
        for t in range(A.shape[0]):
            assert np.all(long[t][:, rank[t]:] == 0)
    rng = np.random.default_rng(1)
    A = P.rand(rng, 3, 9, 5)
    A[1] = 0.0
    U, sv, V, rank, conv = T.tsqr_svd_ref(A)
    assert np.all(sv[1] == 0) and rank[1] == 0 and conv[1] == 1 and np.all(U[1] == 0) and np.array_equal(V[1], np.eye(5))
    for k in (70, -70):                                                      # the prescale is exact
        Uk, svk, Vk = T.tsqr_svd_ref(A * 2.0 ** k)[:3]
        assert np.array_equal(Uk, U) and np.array_equal(Vk, V) and np.array_equal(svk, sv * 2.0 ** k)
    Uh, svh, Vh = T.tsqr_svd_ref(np.conj(np.swapaxes(A, 1, 2)))[:3]          # the swap of the factors
    assert np.array_equal(Uh, V) and np.array_equal(Vh, U) and np.array_equal(svh, sv)
    assert T.tq_chunk(48) == 128 and T.tq_chunk(49) == 64
    assert T.workspace_bytes(64, 65536, 64) == 65536 * 64 * 16 + 3 * 64 * 1024 * 8 + 2 * 64 * 64 * 16 + 4


@pytest.mark.parametrize("rows,cols", GRADED_SHAPES)
def test_graded_long_side_is_orthonormal_to_rounding_level_and_the_alternatives_are_not(rows, cols):
    """The reason the route exists, and that the bound can tell the three apart: the restated long-side factor meets the a-priori
    rounding ceiling; A V Sigma^-1 from the same triangle misses it by eight orders of magnitude; the back-application alone,
    without L (I + E^H E / 2), misses it as well (its loss is second order in eps sigma_1 / sigma_k)."""
    A = dict(T.classes(rows, cols))["graded"]
    ceil = rounding_ceiling(rows, cols)
    tall = rows >= cols
    U, sv, V, rank, _ = T.tsqr_svd_ref(A)
    U0, _, V0, _, _ = T.tsqr_svd_ref(A, correct=False)
    AV = T.av_long_side(A)
    e, e0, eav = [], [], []
    for t in range(A.shape[0]):
        k = rank[t]
        e.append(S._orth_err((U[t] if tall else V[t])[:, :k]))
        e0.append(S._orth_err((U0[t] if tall else V0[t])[:, :k]))
        eav.append(S._orth_err(AV[t][:, :k]))
        # the correction moves nothing the reconstruction can see
        d = np.linalg.norm((U[t] * sv[t]) @ np.conj(V[t].T) - (U0[t] * sv[t]) @ np.conj(V0[t].T), 2) / sv[t, 0]
        assert d <= ceil, d
    print("%dx%d graded: restatement %.3g, without the correction %.3g, A V / sigma %.3g, ceiling %.3g" % (rows, cols, max(e), max(e0), min(eav), ceil))
    assert max(e) <= ceil, (e, ceil)
    assert max(e0) > ceil and min(eav) > 1e4 * ceil, (e0, eav, ceil)
