"""The problems of tests/test_gpu_until32.py and tests/test_until32_ref.py (TEST INFRASTRUCTURE, not a test module): batch 3, four
sparse entries per trial, half of the measurements observed, on the four branches of the fp32 ADMM loop

  d  N = 32, M = 140, Gr = 32, G2 = 16, B per trial                              no pass (the shape does not take it)
  b  N = 64, M = 256, Gr = 64, G2 = 128, generic B per trial, JSTSP_H2=2         the general fused pass
  c  b with JSTSP_FUSED=0                                                        the three-kernel iteration
  a  b's shape with a block-Toeplitz B of block height 64, JSTSP_H2=2            the window kernel of the fused pass

every input rounded to complex64 / float32, so that the float64 reference (tests/until_ref.py) runs on the values the fp32 solver is
given.  TOL = (1e-1, 1e-2, 1e-3) per trial, MIN_ITERS = 2, IMAX = 24: three distinct stops (3 / 7 / 13 on d, 3 / 7 / 17 on a and
b) whose every decision keeps |ce3 / tol - 1| >= 5e-2 (tests/test_until32_ref.py), a hundred times the 5e-4 the fp32
convergence_error is held to against float64 - so the reference alone decides every stop.
"""
import functools

import numpy as np

import until_ref

BATCH, IMAX, MIN_ITERS = 3, 24, 2
TOL = (1e-1, 1e-2, 1e-3)
SHAPES = {"d": (32, 140, 32, 16), "b": (64, 256, 64, 128), "c": (64, 256, 64, 128), "a": (64, 256, 64, 128)}
CASES = ("a", "b", "c", "d")
ENV = {"a": {"JSTSP_H2": "2"}, "b": {"JSTSP_H2": "2"}, "c": {"JSTSP_H2": "2", "JSTSP_FUSED": "0"}, "d": {}}
POLICIES = (None, (0, 1), (2, 3))
STOPS = {"d": [3, 7, 13], "b": [3, 7, 17], "c": [3, 7, 17], "a": [3, 7, 17]}      # without indx_S, every policy
MIN_ITERS_LATE = 10
WARM_IT0, WARM_TOL = 6, 1.7e-2          # (every warm decision keeps its margin at this tol: tests/test_until32_ref.py)


@functools.lru_cache(maxsize=None)
def problem(case):
    """dict(subY, Omega, A, B, tau_Y, tau_S, rho, indx_S): complex64 / float32 arrays, float64 scalars, int32 (3, Gr G2) lists."""
    N, M, Gr, G2 = SHAPES[case]
    rng = np.random.default_rng([20190913, N, M, 1])
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    A = c(N, Gr) / np.sqrt(N)
    B = c(BATCH, G2, M) / np.sqrt(G2)
    if case == "a":                     # block ld is block 0 delayed by ld columns (the columns m < ld stay as drawn)
        for ld in range(1, G2 // 64):
            B[:, ld * 64:(ld + 1) * 64, ld:] = B[:, :64, :M - ld]
    S0 = np.zeros((BATCH, Gr, G2), complex)
    sups = []
    for t in range(BATCH):
        flat = np.zeros(Gr * G2, complex)
        sup = rng.choice(Gr * G2, 4, replace=False)
        flat[sup] = 3 * c(4)
        S0[t] = flat.reshape(Gr, G2, order="F")
        sups.append(sup)
    Om = rng.random((BATCH, N, M)) < 0.5
    subY = Om * (A @ S0 @ B + 0.05 * c(BATCH, N, M))
    tau_Y = 0.02 + 0.01 * rng.random(BATCH)
    tau_S = 0.02 + 0.01 * rng.random(BATCH)
    rho = 0.2 + 0.3 * rng.random(BATCH)
    # an order for indx_S (a generator of its own: the draws above are the recipe's): the true support first, then the rest shuffled
    rng2 = np.random.default_rng([20190913, N, M, 2])
    ix = np.empty((BATCH, Gr * G2), np.int32)
    for t in range(BATCH):
        rest = np.setdiff1d(np.arange(Gr * G2), sups[t])
        ix[t] = np.concatenate([sups[t], rng2.permutation(rest)]) + 1
    return dict(subY=subY.astype(np.complex64), Omega=Om.astype(np.float32), A=A.astype(np.complex64), B=B.astype(np.complex64),
                tau_Y=tau_Y, tau_S=tau_S, rho=rho, indx_S=ix)


def trial(case, t, subY=None):
    """the float64 arguments of until_ref.solve_until for trial t: (subY, Omega, A, B), (tau_Y, tau_S, rho), indx_S"""
    p = problem(case)
    w = lambda x: x.astype(np.complex128)
    y = p["subY"][t] if subY is None else subY
    return (w(y), p["Omega"][t].astype(np.float64), w(p["A"]), w(p["B"][t])), (float(p["tau_Y"][t]), float(p["tau_S"][t]), float(p["rho"][t])), \
        p["indx_S"][t]


@functools.lru_cache(maxsize=None)
def reference(case, refresh=None, use_indx=False, min_iters=MIN_ITERS, warm=False, Imax=IMAX, tols=TOL, want_ce=False):
    """until_ref.solve_until of the three trials, once per session.  Case c is case b (the switch is the library's).  warm: from the
    WARM_IT0-iteration state of the NEXT trial (plain Alg. 2 from zero) at it0 = WARM_IT0."""
    case = "b" if case == "c" else case
    out = []
    for t in range(BATCH):
        mats, prm, ix = trial(case, t)
        kw = dict(state=warm_state(case, (t + 1) % BATCH).astype(np.complex128), it0=WARM_IT0) if warm else {}
        out.append(until_ref.solve_until(*mats, Imax, *prm, tols[t], min_iters, indx_S=ix if use_indx else None, refresh=refresh,
                                         want_ce=want_ce, **kw))
    return out


@functools.lru_cache(maxsize=None)
def warm_state(case, t):
    import resume_ref
    mats, prm, _ = trial(case, t)
    return resume_ref.solve(*mats, WARM_IT0, *prm, "approximate", want_ce=False)[3].astype(np.complex64)     # (what the fp32 solver is given)
