"""tests/until_ref.py without a GPU: the one-iteration-at-a-time wrapper is the single solve of `iters` iterations, the rule is the
one include/jstsp.h states, and - what makes the GPU test of jstsp_proposed_until_f64 a test of bits - every decision the cases of
tests/test_gpu_until64.py take keeps its distance from the threshold.

The margin: min over the iterations i that ran and could stop of |ce3(i) / tol - 1| >= 1e-3, for EVERY trial of every case (no
trial is left out).  The solver agrees with the restatement to 1e-8 in convergence_error (TOL64_CE of tests/test_gpu_resume64.py),
five decades below."""
import numpy as np
import pytest

import refresh_ref as F
import resume_problems as P
import resume_ref as R
import until_ref as U

MARGIN = 1e-3


def _eq(a, b):
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("use_indx", [False, True], ids=["plain", "indx"])
@pytest.mark.parametrize("name", ["R1", "R2"])
def test_the_wrapper_is_one_solve_of_iters_iterations(name, use_indx):
    """B per trial; from zero and from the 30-iteration state of the next trial."""
    p = P.problem(name, False)
    for warm in (False, True):
        tols = (U.WARM_TOL,) * P.BATCH if warm else U.TOLS["abc"]
        for t, got in enumerate(U.reference(name, False, use_indx, None, tols, warm=warm)):
            mats, prm, ix = P.trial(p, t)
            S, Y, ce, state, order, iters, ce3 = got
            kw = dict(state=U.warm_state(name, False, (t + 1) % P.BATCH), it0=U.WARM_IT0) if warm else {}
            want = R.solve(*mats, iters, *prm, "approximate", indx_S=ix if use_indx else None, want_ce=False, **kw)
            _eq((S, Y, ce[:iters], state), want)
            assert np.isnan(ce[iters:]).all() and ce3 == want[2][-1, 2]
            assert 1 <= iters <= U.IMAX and (iters == U.IMAX or (iters >= U.MIN_ITERS and ce3 <= tols[t]))
            assert not any(U.stops(k + 1, ce[k, 2], tols[t], U.MIN_ITERS) for k in range(iters - 1))      # the FIRST such iteration


def test_the_wrapper_with_a_policy_is_the_refreshed_solve():
    p = P.problem("R1", False)
    for refresh in ((0, 1), (2, 3)):
        for t, got in enumerate(U.reference("R1", False, False, refresh, U.TOLS["abc"])):
            mats, prm, _ = P.trial(p, t)
            S, Y, ce, state, order, iters, ce3 = got
            want = F.solve(*mats, iters, *prm, start=refresh[0], period=refresh[1], want_ce=False)
            _eq((S, Y, ce[:iters], state, order), want)


def test_the_rule():
    assert U.stops(2, 1e-3, 1e-3, 2) and not U.stops(1, 1e-3, 1e-3, 2) and not U.stops(5, 1.1e-3, 1e-3, 2)
    for never in (0.0, -1.0, np.nan):                           # a tol that is zero, negative or NaN stops nothing, not even ce3 = 0
        assert not U.stops(9, 0.0, never, 1)
    assert not U.stops(9, np.inf, 1e300, 1) and not U.stops(9, np.nan, 1.0, 1)
    # the Inf of iteration 1 from a zero state, min_iters = 1, a huge tol: the trial goes on
    mats, prm, _ = P.trial(P.problem("R1", False), 0)
    out = U.solve_until(*mats, 3, *prm, 1e300, 1, want_ce=False)
    assert np.isinf(out[2][0, 2]) and out[5] == 2


@pytest.mark.parametrize("name,shared_B,use_indx,refresh", U.CONFIGS)
def test_every_decision_of_the_gpu_cases_keeps_its_margin(name, shared_B, use_indx, refresh):
    """Also the two tol sets give the stops the GPU test is built on: three distinct iterations, and one trial at IMAX."""
    for key, tols in U.TOLS.items():
        ref = U.reference(name, shared_B, use_indx, refresh, tols)
        for t, got in enumerate(ref):
            m = U.margin(got[2], got[5], tols[t], U.MIN_ITERS)
            print("%s sharedB=%s indx=%s refresh=%s tol=%g: iters %d, margin %.3g" % (name, shared_B, use_indx, refresh, tols[t], got[5], m))
            assert m >= MARGIN
        iters = [got[5] for got in ref]
        assert len(set(iters)) == 3 and iters[0] < min(iters[1:])
        if key == "a0c":
            assert iters[1] == U.IMAX and ref[1][6] > 0


def test_the_warm_decisions_keep_their_margin():
    """R1, B per trial, from the next trial's state: min_iters = 1 stops at the leg's first iteration, min_iters = 5 at its fifth."""
    for min_iters in (1, 5):
        ref = U.reference("R1", False, False, None, (U.WARM_TOL,) * P.BATCH, min_iters, True)
        for got in ref:
            assert got[5] == min_iters
            # every iteration of the leg, not only those from min_iters on: none of them is near the threshold
            assert U.margin(got[2], got[5], U.WARM_TOL, 1) >= MARGIN
