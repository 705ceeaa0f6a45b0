"""tests/until32_problems.py without a GPU: what makes tests/test_gpu_until32.py a test of the fp32 solver's decisions and not of
luck.  Every decision that every (case, policy, indx_S, min_iters, warm) of the GPU tests takes keeps |ce3 / tol - 1| >= 5e-2 in the
float64 reference - a hundred times TOL_CE = 5e-4, the bound the fp32 convergence_error meets against float64 - for EVERY trial, and
the stops are the ones the cases were built for (three distinct iterations per batch)."""
import numpy as np
import pytest

import until32_problems as P
import until_ref as U
from conftest import TOL_CE

MARGIN = 5e-2
REF_CASES = ("a", "b", "d")                     # c is b under a switch of the library


def test_the_margin_is_a_hundred_times_the_fp32_bound():
    assert MARGIN >= 100 * TOL_CE


@pytest.mark.parametrize("use_indx", [False, True], ids=["plain", "indx"])
@pytest.mark.parametrize("refresh", P.POLICIES, ids=["none", "0_1", "2_3"])
@pytest.mark.parametrize("case", REF_CASES)
def test_every_decision_keeps_its_margin_and_the_stops_are_the_tables(case, refresh, use_indx):
    ref = P.reference(case, refresh, use_indx)
    for t, got in enumerate(ref):
        m = U.margin(got[2], got[5], P.TOL[t], P.MIN_ITERS)
        print("%s refresh=%s indx=%s tol=%g: iters %d, margin %.3g" % (case, refresh, use_indx, P.TOL[t], got[5], m))
        assert m >= MARGIN
        assert got[5] < P.IMAX and got[6] <= P.TOL[t]           # the rule stopped it, not Imax
    assert [got[5] for got in ref] == P.STOPS[case]


@pytest.mark.parametrize("case", REF_CASES)
def test_the_late_min_iters_the_warm_start_and_the_loose_tol_keep_their_margin(case):
    late = P.reference(case, None, False, P.MIN_ITERS_LATE)
    for t, got in enumerate(late):
        assert got[5] == max(P.MIN_ITERS_LATE, P.STOPS[case][t])
        assert U.margin(got[2], got[5], P.TOL[t], P.MIN_ITERS_LATE) >= MARGIN
    warm = P.reference(case, None, False, P.MIN_ITERS, True, tols=(P.WARM_TOL,) * P.BATCH)
    for got in warm:
        print(case, "warm", got[5], U.margin(got[2], got[5], P.WARM_TOL, P.MIN_ITERS))
        assert P.MIN_ITERS <= got[5] < P.IMAX and U.margin(got[2], got[5], P.WARM_TOL, P.MIN_ITERS) >= MARGIN
    # (the "other trials' tol" test gives the others 0 - never - or 1e300 - at min_iters: no decision of theirs is near a threshold)
    for got in P.reference(case, None, False, tols=(1e300,) * P.BATCH):
        assert got[5] == P.MIN_ITERS


def test_legs_of_the_reference_compose():
    """Imax = 5, then from the returned state at it0 = 5: the sum of iters and the result are the whole call's (the rule is
    memoryless) - what the GPU test of legs relies on."""
    for t in range(P.BATCH):
        mats, prm, _ = P.trial("d", t)
        whole = P.reference("d")[t]
        a = U.solve_until(*mats, 5, *prm, P.TOL[t], P.MIN_ITERS, want_ce=False)
        if a[5] < 5:
            assert a[5] == whole[5]
            continue
        b = U.solve_until(*mats, P.IMAX - 5, *prm, P.TOL[t], P.MIN_ITERS, state=a[3], it0=5, want_ce=False)
        assert 5 + b[5] == whole[5] and np.array_equal(b[0], whole[0])
