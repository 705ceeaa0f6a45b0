"""tests/refresh_ref.py, the numpy restatement of the refreshed Alg. 2, checked without a GPU against what already stands: it
equals the chain of one-iteration legs of tests/resume_ref.py with a stable argsort between them, it is resume_ref when no
refresh falls into the call, its schedule is the one include/jstsp.h states - and the problems the GPU test compares it on keep
every mask-boundary key gap above 1e-9 relative, the floor of the decision rule of DESIGN.md section 9c."""
import numpy as np
import pytest

import refresh_ref as F
import resume_problems as P
import resume_ref as R

POLICIES = [(0, 1), (2, 0), (1, 2), (3, 1)]
IMAX = 6


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def chain(m, prm, Imax, start, period, indx_S=None, state=None, it0=0):
    """The refreshed solve through resume_ref alone: from s_{i-1} one unmasked iteration gives v_i and its order, one masked
    iteration from s_{i-1} under that order at it0 = i - 1 gives s_i; every other iteration is one iteration under the order in
    force."""
    N, M = m[0].shape
    Gr, G2 = m[2].shape[1], m[3].shape[0]
    g = Gr * G2
    force, order, rows = indx_S, indx_S, []
    if state is None:
        state = np.zeros(R.state_elems(N, M, Gr, G2), dtype=np.complex128)
    S = Y = None
    for i in range(it0 + 1, it0 + Imax + 1):
        if F.is_refresh(i, start, period):
            free = R.solve(*m, 1, *prm, "approximate", state=state, it0=i - 1)[3]
            v = R.unpack_state(free, N, M, Gr, G2)[4]
            order = force = F.order_of(v)[:min(g, F.TOP_MAX)]
        S, Y, ce, state = R.solve(*m, 1, *prm, "approximate", indx_S=force, state=state, it0=i - 1)
        rows.append(ce)
    return S, Y, np.concatenate(rows), state, order


@pytest.mark.parametrize("start,period", POLICIES)
def test_the_restatement_is_the_chain_of_one_iteration_legs(start, period):
    p = P.problem("R1", False)
    for t in (0, 2):
        m, prm, ix = P.trial(p, t)
        for prior in (None, ix):
            got = F.solve(*m, IMAX, *prm, start=start, period=period, indx_S=prior)
            want = chain(m, prm, IMAX, start, period, indx_S=prior)
            np.testing.assert_array_equal(got[4], want[4])
            for a, b in zip(got[:2] + (got[3],), want[:2] + (want[3],)):
                assert _rel(a, b) <= 1e-12
            fin = np.isfinite(want[2])
            assert np.array_equal(fin, np.isfinite(got[2])) and _rel(got[2][fin], want[2][fin]) <= 1e-12


def test_the_policies_differ_from_each_other_and_from_the_plain_solve():
    m, prm, ix = P.trial(P.problem("R1", False), 0)
    outs = [F.solve(*m, IMAX, *prm, start=s, period=q)[0] for s, q in POLICIES] + [R.solve(*m, IMAX, *prm)[0]]
    for a in range(len(outs)):
        for b in range(a):
            assert not np.array_equal(outs[a], outs[b]), (a, b)


def test_without_a_refresh_in_the_call_it_is_resume_ref():
    p = P.problem("R1", True)
    m, prm, ix = P.trial(p, 1)
    for prior in (None, ix):
        for start, period in ((IMAX, 1), (IMAX + 3, 0), (IMAX, 4)):
            got = F.solve(*m, IMAX, *prm, start=start, period=period, indx_S=prior)
            want = R.solve(*m, IMAX, *prm, "approximate", indx_S=prior)
            for a, b in zip(got[:4], want):
                assert np.array_equal(a, b, equal_nan=True)
            assert got[4] is prior
    # and a later leg: it0 + Imax <= start
    mid = R.solve(*m, 2, *prm, "approximate", indx_S=ix)[3]
    got = F.solve(*m, 3, *prm, start=5, period=1, indx_S=ix, state=mid, it0=2)
    want = R.solve(*m, 3, *prm, "approximate", indx_S=ix, state=mid, it0=2)
    for a, b in zip(got[:4], want):
        assert np.array_equal(a, b)


def test_legs_that_pass_the_order_on_are_the_whole_call():
    m, prm, ix = P.trial(P.problem("R1", False), 1)
    for start, period in POLICIES:
        whole = F.solve(*m, IMAX, *prm, start=start, period=period, indx_S=ix)
        for legs in ((1, 5), (2, 4), (3, 1, 2)):
            state, order, done, rows = None, ix, 0, []
            for n in legs:
                S, Y, ce, state, order = F.solve(*m, n, *prm, start=start, period=period, indx_S=order, state=state, it0=done)
                rows.append(ce)
                done += n
            for a, b in zip((S, Y, np.concatenate(rows), state, order), whole):
                assert np.array_equal(a, b)


def test_the_schedule():
    assert F.schedule(0, 6, 0, 1) == [1, 2, 3, 4, 5, 6]
    assert F.schedule(0, 6, 2, 0) == [3]
    assert F.schedule(0, 6, 1, 2) == [2, 4, 6]
    assert F.schedule(0, 10, 0, 3) == [1, 4, 7, 10]
    assert F.schedule(0, 10, 2, 3) == [3, 6, 9]
    assert F.schedule(4, 6, 2, 3) == [6, 9]                 # a function of the global index, not of where the call starts
    assert F.schedule(3, 4, 2, 0) == [] and F.schedule(2, 1, 2, 0) == [3]
    assert F.schedule(0, 6, 6, 1) == [] and F.schedule(0, 6, 5, 1) == [6]
    assert F.schedule(0, 0, 0, 1) == []


def test_the_wrapper_knows_whether_a_call_refreshes():
    from jstsp19_amd import solvers
    for it0 in range(0, 9):
        for Imax in range(1, 8):
            for start in range(0, 12):
                for period in (0, 1, 2, 3, 5):
                    s = F.schedule(it0, Imax, start, period)
                    assert solvers._refresh_first(it0, Imax, start, period) == (s[0] if s else None), (it0, Imax, start, period)


# The problems of tests/test_gpu_refresh64.py (h): (name, shared_B, start, period), every trial, Imax = 6
BOUNDED = [(n, sh, s, q) for n in ("R1", "R2") for sh in (False, True) for s, q in ((0, 1), (1, 2))]


@pytest.mark.parametrize("name,shared_B,start,period", BOUNDED)
def test_the_mask_boundaries_of_the_compared_problems_are_decided(name, shared_B, start, period):
    """A device v that differs from the restatement's in its last bits selects the same mask when the keys on either side of every
    mask boundary differ by more than 1e-9 relative (|z|^2 carries twice the relative error of z, far below)."""
    p = P.problem(name, shared_B)
    for t in range(P.BATCH):
        m, prm, _ = P.trial(p, t)
        gaps = []
        F.solve(*m, IMAX, *prm, start=start, period=period, gaps=gaps, want_ce=False)
        seen = [x for x in gaps if x is not None]
        assert len(gaps) == IMAX - start and seen and min(seen) > 1e-9, (t, gaps)
