"""Float64 numpy restatement of the stopping rule of jstsp_proposed_until_f64 (TEST INFRASTRUCTURE, not a test module): the loop
of tests/resume_ref.py ('approximate') - or, with a support policy, of tests/refresh_ref.py - run ONE iteration at a time, with the
rule applied between two iterations.

    trial t runs the global iterations it0 + 1, it0 + 2, ...
    it stops after the first iteration i with  i - it0 >= min_iters  and  ce(i, 3) <= tol      (ce(i, 3): proposed_algorithm.m:51)
    failing that it stops after it0 + Imax

The rule is memoryless - a function of i, it0 and the iterate alone.  A tol that is zero, negative or NaN never stops the trial
(``ce <= tol`` is false for a NaN on either side, and ce >= 0); neither does the Inf of iteration 1 from a zero state.

``solve_until`` returns ``(S, Y, ce, state, order, iters, ce3)``: ``ce`` has Imax rows, NaN after the last iteration that ran;
``order`` is that of refresh_ref.solve over the iterations that ran (``indx_S`` as given when none of them refreshed, and without a
policy); ``ce3`` is ce(., 3) of the last iteration.  ``margin(ce, iters, tol, min_iters)`` is the distance of the closest of the
trial's decisions from its threshold, min over the iterations that ran and could stop of |ce3(i) / tol - 1|.
"""
import functools

import numpy as np

import refresh_ref
import resume_problems
import resume_ref


# ---- the cases of tests/test_gpu_until64.py; tests/test_until_ref.py checks the margin of every decision they take ----------------
IMAX = 40
MIN_ITERS = 2
TOLS = {"abc": (1e-2, 1e-3, 1e-4), "a0c": (1e-2, 0.0, 1e-4)}       # per trial: three distinct stops; one trial that runs to IMAX
WARM_IT0 = 30
WARM_TOL = 0.5                                                      # from another trial's 30-iteration state ce3 starts near 0.2
# (problem, B shared, indx_S in force, (start, period) or None); R2 has Gram order 72, the global-memory Jacobi
CONFIGS = [("R1", False, False, None), ("R1", True, False, None), ("R1", False, True, None), ("R1", False, False, (0, 1)),
           ("R1", False, False, (2, 3)), ("R2", False, False, None), ("R2", False, False, (2, 3))]


def stops(k, ce3, tol, min_iters):
    """The rule after the k-th iteration of the call (k = i - it0, 1-based)."""
    return bool(k >= min_iters and tol > 0 and ce3 <= tol)


@functools.lru_cache(maxsize=None)
def reference(name, shared_B, use_indx, refresh, tols, min_iters=MIN_ITERS, warm=False, Imax=IMAX):
    """solve_until of every trial of a case, once per session: a list of its result tuples.  warm: from the WARM_IT0-iteration
    state of the NEXT trial (plain Alg. 2 from zero), at it0 = WARM_IT0."""
    p = resume_problems.problem(name, shared_B)
    out = []
    for t in range(resume_problems.BATCH):
        mats, prm, ix = resume_problems.trial(p, t)
        kw = {}
        if warm:
            kw = dict(state=warm_state(name, shared_B, (t + 1) % resume_problems.BATCH), it0=WARM_IT0)
        out.append(solve_until(*mats, Imax, *prm, tols[t], min_iters, indx_S=ix if use_indx else None, refresh=refresh, want_ce=False, **kw))
    return out


@functools.lru_cache(maxsize=None)
def warm_state(name, shared_B, t):
    mats, prm, _ = resume_problems.trial(resume_problems.problem(name, shared_B), t)
    return resume_ref.solve(*mats, WARM_IT0, *prm, "approximate", want_ce=False)[3]


def solve_until(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, tol, min_iters=2, indx_S=None, refresh=None, state=None, it0=0,
                want_ce=True):
    assert Imax >= 1 and min_iters >= 1
    ce = np.full((Imax, 3), np.nan)
    order, in_force = indx_S, indx_S
    S = Y = None
    k = 0
    while k < Imax:
        if refresh is None:
            S, Y, c1, state = resume_ref.solve(subY, Omega, A, B, 1, tau_Y, tau_S, rho, "approximate", indx_S=indx_S, state=state,
                                               it0=it0 + k, want_ce=want_ce)
        else:
            S, Y, c1, state, in_force = refresh_ref.solve(subY, Omega, A, B, 1, tau_Y, tau_S, rho, start=refresh[0], period=refresh[1],
                                                          indx_S=in_force, state=state, it0=it0 + k, want_ce=want_ce)
            order = in_force
        ce[k] = c1[0]
        k += 1
        if stops(k, c1[0, 2], tol, min_iters):
            break
    return S, Y, ce, state, order, k, float(ce[k - 1, 2])


def margin(ce, iters, tol, min_iters=2):
    """min over the decisions taken (iterations min_iters ... iters of the call) of |ce3 / tol - 1|; Inf for a tol that never stops."""
    if not tol > 0:
        return np.inf
    c3 = np.asarray(ce)[min_iters - 1:iters, 2]
    with np.errstate(invalid="ignore"):
        m = np.abs(c3 / tol - 1.0)
    return float(np.nanmin(m)) if m.size and not np.all(np.isnan(m)) else np.inf
