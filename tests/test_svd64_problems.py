"""CPU checks of tests/svd64_problems.py - that the bounds of tests/test_gpu_svd64.py come from the restatement and not from the
inputs: the restatement's worst values over the problem set are recomputed here and compared with the recorded ones
(tests/golden/svd64_restatement_worst.json), 4 x them stays under the a-priori ceiling 4 S (n - 1) 2^-52, numpy's own SVD meets
the resulting bounds on every problem, the restatement's singular values agree with numpy's within the bounds the project asserts
for the same rotations, and the rank-deficient inputs keep every reference value a factor 4 away from the drop threshold."""
import numpy as np
import pytest

import spectrum_problems as P
import svd64_problems as S

ROUTES = ("lds", "global")


@pytest.mark.parametrize("route", ROUTES)
def test_recorded_worst_values_are_the_restatements(route):
    """numpy's sums may differ in the last bits from one build to another, and with them the pairs that still rotate in the last
    sweeps: the recorded values have to be met within a factor 1.5 either way, not on the bits."""
    got, bd = S.recomputed_worst(route), S.bounds(route)
    for k in ("e_rec", "e_long", "e_short"):
        print("%s %s: restatement %.3g, recorded bound %.3g" % (route, k, got[k], bd[k]))
        assert bd[k] / 1.5 <= S.MARGIN * got[k] <= bd[k] * 1.5, (route, k, got[k], bd[k])
    assert bd["e_sv"] == S.SV_BOUND[route]


@pytest.mark.parametrize("route", ROUTES)
def test_bounds_stay_under_the_a_priori_ceiling_and_numpy_meets_them(route):
    bd = S.bounds(route)
    n_max = max(min(r[0], r[1]) for r in S.restatement_records(route))
    for k in ("e_rec", "e_long", "e_short"):
        assert bd[k] <= S.ceiling(route, n_max), (route, k, bd[k], S.ceiling(route, n_max))
    for rows, cols, name, mine, nump, sweeps, conv in S.restatement_records(route):
        for k in ("e_sv", "e_rec", "e_long", "e_short"):
            assert nump[k] <= bd[k], (rows, cols, name, k, nump[k], bd[k])           # numpy's own SVD
            assert mine[k] <= bd[k], (rows, cols, name, k, mine[k], bd[k])           # sv of the restatement against P.ref
        assert conv and sweeps <= S.SWEEP_CAP[route], (rows, cols, name, sweeps)


@pytest.mark.parametrize("route", ROUTES)
def test_reference_values_are_clear_of_the_drop_threshold(route):
    for rows, cols, name, A in S.problem_set(route):
        ref = P.ref(A)
        thr = S.drop_threshold(rows, cols, ref[:, 0])[:, None]
        assert not np.any((ref > thr / 4) & (ref < thr * 4)), (rows, cols, name)
        want = {"rank6": 6, "repeated": min(50, min(rows, cols))}.get(name, min(rows, cols))
        assert np.all(np.sum(ref > thr, axis=1) == want), (rows, cols, name)


def test_restatement_on_the_edge_cases():
    rng = np.random.default_rng(1)
    A = P.rand(rng, 4, 9, 5)
    A[1] = 0.0
    U, sv, V, rank, conv, sweeps = S.jacobi_svd_ref(A)
    assert np.all(sv[1] == 0) and rank[1] == 0 and conv[1] == 1 and np.all(U[1] == 0) and np.array_equal(V[1], np.eye(5))
    assert list(rank[[0, 2, 3]]) == [5, 5, 5] and np.all(conv == 1)
    for k in (40, -40):                                                      # the prescale is exact
        Uk, svk, Vk = S.jacobi_svd_ref(A * 2.0 ** k)[:3]
        assert np.array_equal(Uk, U) and np.array_equal(Vk, V) and np.array_equal(svk, sv * 2.0 ** k)
    Ah = np.conj(np.swapaxes(A, 1, 2))                                       # the swap of the factors
    Uh, svh, Vh = S.jacobi_svd_ref(Ah)[:3]
    assert np.array_equal(Uh, V) and np.array_equal(Vh, U) and np.array_equal(svh, sv)
    assert S.route_of(64, 64) == S.route_of(32, 140) == S.route_of(128, 50) == "lds"
    assert S.route_of(40, 600) == S.route_of(66, 520) == S.route_of(65, 65) == "global"
    x = np.array([1.0, 1.5, 2.0, 3.9, 0.0])
    assert np.array_equal(S.drop_threshold(8, 3, x), [8 * 2.0 ** -52, 8 * 2.0 ** -52, 8 * 2.0 ** -51, 8 * 2.0 ** -51, 0.0])
