"""Problems for the refreshed fp32 ADMM (jstsp_proposed_refresh_c32; TEST INFRASTRUCTURE, not a test module): host-made numpy
problems, batch 3, per-trial tau_Y, tau_S, rho, every complex array rounded to complex64 - the values the fp32 solver is given
are the values tests/refresh_ref.py restates in float64 - at

  R1, R2   of tests/resume_problems.py (32, 140, 32, 16 and 72, 80, 24, 20): neither shape takes the fused pass
  T        64, 256, 64, 128 with a block-Toeplitz B of block height 64, B(64 + g, m) == B(g, m - 1) bit for bit for m >= 1
  G        the same shape with a generic B

and the rule that says for which trials a float64 restatement decides the mask of the fp32 solver.

THE DECISION RULE.  Under a refreshed order the mask of iteration i is the first cnt(i) = min(10 + 5 i, g) entries of the order of
the v of the last refresh.  The fp32 solver is held to TOL_S * max|ref| per entry (tests/conftest.py), so two neighbouring entries
of that order can change places only if their magnitudes differ by at most 2 * TOL_S * max|v|.  A trial is DECIDED for a policy
when, at every iteration that runs under a refreshed order, the magnitude gap at the mask boundary

    (|v_(cnt)| - |v_(cnt + 1)|) / max|v|        (v: the restatement's v of the last refresh, sorted by descending magnitude)

exceeds 4 * TOL_S: the remaining factor 2 is the margin.  Where the mask holds the whole list there is no boundary and no condition.
"""
import functools

import numpy as np

import refresh_ref as RR
import resume_problems as P
import resume_ref as R
from conftest import TOL_S

BATCH = P.BATCH
SHAPES = dict(P.SHAPES, T=(64, 256, 64, 128), G=(64, 256, 64, 128))
NAMES = ("R1", "R2", "T", "G")
POLICIES = ((2, 0), (0, 1), (1, 2), (3, 1))         # (start, period)
IMAX = 6
GAP_MIN = 4 * TOL_S
SEED_NEW = 20190913                                 # the seed of T and G (tests/test_refresh32_ref.py holds it to the two conditions)


def _c(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def _new_shape(name):
    """T / G in the layout of resume_problems.problem, complex128 before the rounding: the same A, S0, Omega and noise for both,
    B per trial - block-Toeplitz of block height 64 (T) or generic of the same scale (G)."""
    N, M, Gr, G2 = SHAPES[name]
    Gt = 64
    rng = np.random.default_rng([SEED_NEW, N, 32])
    A = _c(rng, N, Gr) / np.sqrt(N)
    Bt = np.zeros((BATCH, G2, M), complex)
    Bt[:, :Gt] = _c(rng, BATCH, Gt, M) / np.sqrt(G2)
    Bt[:, Gt:, 1:] = Bt[:, :Gt, :-1]                    # block 1 = block 0 one column later
    Bt[:, Gt:, 0] = _c(rng, BATCH, Gt) / np.sqrt(G2)    # (its leading column is its own)
    Bg = _c(rng, BATCH, G2, M) / np.sqrt(G2)
    B = Bt if name == "T" else Bg
    g = Gr * G2
    S0 = np.zeros((BATCH, Gr, G2), complex)
    idx = np.zeros((BATCH, g), np.int32)
    for t in range(BATCH):
        sup = rng.choice(g, len(P.SUPPORT_RANKS), replace=False)
        flat = np.zeros(g, complex)
        flat[sup] = 3 * _c(rng, len(sup))
        S0[t] = flat.reshape(Gr, G2, order="F")
        rest = rng.permutation(np.setdiff1d(np.arange(g), sup))
        idx[t] = np.concatenate([rest[:P.SUPPORT_RANKS[0]], sup, rest[P.SUPPORT_RANKS[0]:]]) + 1
    Om = (rng.random((BATCH, N, M)) < 0.5).astype(float)
    noise = 0.05 * _c(rng, BATCH, N, M)
    tY = 0.02 + 0.01 * rng.random(BATCH); tS = 0.02 + 0.01 * rng.random(BATCH); rho = 0.2 + 0.3 * rng.random(BATCH)
    # subY is formed from the ROUNDED factors, so that T's dictionary stays block-Toeplitz on the bits and subY belongs to it
    A32, B32 = A.astype(np.complex64), B.astype(np.complex64)
    subY = Om * (A32.astype(complex) @ S0 @ B32.astype(complex) + noise)
    return dict(subY=subY, Omega=Om, A=A32, B=B32, tau_Y=tY, tau_S=tS, rho=rho, indx_S=idx)


@functools.lru_cache(maxsize=None)
def problem(name, shared_B=False):
    """dict(subY, Omega, A, B, tau_Y, tau_S, rho, indx_S) as the fp32 entries take it on the host path: complex64 / float32 arrays,
    float64 scalars per trial, int32 indx_S (batch, g).  shared_B: R1 and R2 only."""
    assert name in NAMES and (not shared_B or name in P.SHAPES)
    p = P.problem(name, shared_B) if name in P.SHAPES else _new_shape(name)
    out = dict(p)
    for k in ("subY", "A", "B"):
        out[k] = np.ascontiguousarray(p[k].astype(np.complex64))
    out["Omega"] = np.ascontiguousarray(p["Omega"].astype(np.float32))
    return out


def trial(p, t):
    """The arguments of refresh_ref.solve for trial t, widened to float64: (subY, Omega, A, B), (tau_Y, tau_S, rho)."""
    B = p["B"] if p["B"].ndim == 2 else p["B"][t]
    w = lambda a: np.asarray(a, dtype=np.complex128)
    return (w(p["subY"][t]), p["Omega"][t].astype(np.float64), w(p["A"]), w(B)), (float(p["tau_Y"][t]), float(p["tau_S"][t]), float(p["rho"][t]))


def boundary_gaps(arrs, prm, Imax, start, period, indx_S=None, state=None, it0=0):
    """The magnitude gaps of the decision rule, one per iteration it0 + 1 ... it0 + Imax that runs under a refreshed order and has a
    boundary: the restatement advanced one iteration at a time (in float64 its legs are the whole call), v taken from the state
    after each refresh."""
    N, M = arrs[0].shape
    Gr, G2 = arrs[2].shape[1], arrs[3].shape[0]
    g = Gr * G2
    gaps, mags, order = [], None, indx_S
    for i in range(it0 + 1, it0 + Imax + 1):
        _, _, _, state, order = RR.solve(*arrs, 1, *prm, start=start, period=period, indx_S=order, state=state, it0=i - 1, want_ce=False)
        if RR.is_refresh(i, start, period):
            v = R.unpack_state(state, N, M, Gr, G2)[4].reshape(-1, order="F")
            mags = np.abs(v)[np.asarray(order, dtype=np.int64) - 1]         # descending along the order
        cnt = min(10 + 5 * i, g)
        if mags is not None and cnt < mags.size:
            gaps.append(float((mags[cnt - 1] - mags[cnt]) / mags[0]))
    return gaps


@functools.lru_cache(maxsize=None)
def min_gap(name, shared_B, t, start, period, Imax=IMAX):
    """The smallest boundary gap of trial t under the policy from zero without a prior (inf: no iteration has a boundary)."""
    arrs, prm = trial(problem(name, shared_B), t)
    return min(boundary_gaps(arrs, prm, Imax, start, period), default=float("inf"))


def decided(name, shared_B, t, start, period, Imax=IMAX):
    return min_gap(name, shared_B, t, start, period, Imax) > GAP_MIN


def variants():
    """(name, shared_B) of every problem."""
    return [("R1", False), ("R1", True), ("R2", False), ("R2", True), ("T", False), ("G", False)]
