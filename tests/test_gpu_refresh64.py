"""jstsp_proposed_refresh_f64 (csrc/proposed64.hip; proposed_algorithm_refresh_f64): the float64 Alg. 2 whose support is
refreshed from its own iterate inside the loop, on the problems of tests/resume_problems.py (Gram order 32 and 72, batch 3,
per-trial scalars, shared and per-trial B, both memspaces), Imax = 6.

Bits: without a refresh in the call it is jstsp_proposed_resume_f64; with one, S, Y, convergence_error, the state and the order
equal the chain through the entries that were there - from s_{i-1} one unmasked iteration gives v_i, support_order_f64(v_i) is the
order, one masked iteration from s_{i-1} at it0 = i - 1 gives s_i - and legs that pass the order on return the whole call.
Bounds (not derived from this code): S and Y within 1e-10 of max|ref| and convergence_error within 1e-8 of tests/refresh_ref.py,
what include/jstsp.h asserts for this solver against its restatement, on problems whose mask boundaries are decided
(tests/test_refresh_ref.py checks that without a GPU)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import refresh_ref as F
import resume_problems as P
from conftest import check_below, ce_rel, rel_err  # noqa: E402
from test_drift_ref import TIE_VALUES
from test_gpu_resume64 import CASES, TOL64_CE, TOL64_S, _eq, _inputs, _mid_state, _np, _resume
from test_refresh_ref import BOUNDED

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = -4, -3
IMAX = 6
# (start, period) and whether the problem's indx_S is in force until the first refresh
POLICIES = [(0, 1, False), (2, 0, True), (1, 2, True), (3, 1, False)]
PREFIX = "proposed_algorithm refresh (float64)"


def _refresh(name, shared_B, mem, Imax, start, period, prior=False, state=None, it0=0, **kw):
    import jstsp19_amd as J
    arrs, ix, prm = _inputs(name, shared_B, mem)
    if prior is True:
        prior = ix
    elif prior is False:
        prior = None
    return J.proposed_algorithm_refresh_f64(*arrs, Imax, *prm, start=start, period=period, indx_S=prior, state=state, it0=it0, **kw)


def _v_of(state, name):
    """The v block of a (batch, elems) state as a (batch, Gr, G2) argument of support_order_f64."""
    N, M, Gr, G2 = P.SHAPES[name]
    blk = state[:, 4 * N * M:4 * N * M + Gr * G2]
    if isinstance(state, np.ndarray):
        return blk.reshape(-1, G2, Gr).swapaxes(1, 2)
    return blk.contiguous().reshape(-1, G2, Gr).transpose(1, 2)


def _chain(name, shared_B, mem, Imax, start, period, prior=False, state=None, it0=0):
    """The refreshed solve through proposed_algorithm_resume_f64 and support_order_f64 alone, one iteration a call."""
    import jstsp19_amd as J
    arrs, ix, prm = _inputs(name, shared_B, mem)
    force = ix if prior else None
    order, rows = force, []
    for i in range(it0 + 1, it0 + Imax + 1):
        at = dict(state=state, it0=i - 1) if state is not None else {}
        if F.is_refresh(i, start, period):
            free = J.proposed_algorithm_resume_f64(*arrs, 1, *prm, want_ce=False, **at)[3]
            order = force = J.support_order_f64(_v_of(free, name))
        S, Y, ce, state = J.proposed_algorithm_resume_f64(*arrs, 1, *prm, indx_S=force, **at)
        rows.append(_np(ce))
    return _np(S), _np(Y), np.concatenate(rows, axis=1), _np(state), _np(order)


def _all(out):
    return tuple(_np(x) for x in out)


@functools.lru_cache(maxsize=None)
def _whole(name, shared_B, start, period, prior):
    """The refreshed solve at Imax = 6 on the host path, once per session."""
    return _all(_refresh(name, shared_B, "host", IMAX, start, period, prior))


# ---- (a) no refresh in the call: the resumed entry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shared_B,mem", CASES)
def test_without_a_refresh_in_the_call_it_is_the_resumed_entry(name, shared_B, mem):
    arrs, ix, prm = _inputs(name, shared_B, mem)
    for prior, kind in ((False, "approx"), (True, "angles")):
        want = _all(_resume(kind, name, shared_B, mem, IMAX))
        pr = ix if prior else False
        for start, period in ((IMAX, 1), (IMAX + 4, 0), (IMAX, 3)):
            got = _refresh(name, shared_B, mem, IMAX, start, period, pr)
            _eq(_all(got[:4]), want)
            assert got[4] is (ix if prior else None)            # no refresh: the caller's indx_S comes back
        # a later leg that ends where the first refresh would begin
        mid = _resume(kind, name, shared_B, mem, 2)[3]
        got = _refresh(name, shared_B, mem, 3, 5, 1, pr, state=mid, it0=2)
        _eq(_all(got[:4]), _all(_resume(kind, name, shared_B, mem, 3, state=mid, it0=2)))
    S, Y, ce, none, _ = _refresh(name, shared_B, mem, IMAX, IMAX, 1, True, want_ce=False, return_state=False)
    assert ce is None and none is None
    _eq(_all((S, Y)), want[:2])


def test_an_order_of_fewer_entries_admits_nothing_else():
    """indx_S with n = 22 entries per trial: the list of the resumed entry with the rest out of range (ignored there)."""
    import jstsp19_amd as J
    arrs, ix, prm = _inputs("R1", False, "host")
    short = ix[:, :22]
    padded = np.concatenate([short, np.zeros((P.BATCH, ix.shape[1] - 22), np.int32)], axis=1)
    want = J.proposed_algorithm_resume_f64(*arrs, IMAX, *prm, indx_S=padded)
    got = _refresh("R1", False, "host", IMAX, IMAX, 0, short)
    _eq(_all(got[:4]), _all(want))
    assert got[4] is short
    assert not np.array_equal(got[0], _resume("angles", "R1", False, "host", IMAX)[0])        # cnt(3) = 25 > 22: the full list admits more
    darrs, dix, _ = _inputs("R1", False, "device")
    got = J.proposed_algorithm_refresh_f64(*darrs, IMAX, *prm, start=IMAX, indx_S=dix[:, :22].contiguous())
    _eq(_all(got[:4]), _all(want))


# ---- (b) the chain through the entries that were there ------------------------------------------------------------------------------
@pytest.mark.parametrize("start,period,prior", POLICIES)
@pytest.mark.parametrize("name,shared_B,mem", CASES)
def test_the_refreshed_solve_is_the_chain_of_one_iteration_calls(name, shared_B, mem, start, period, prior):
    got = _all(_refresh(name, shared_B, mem, IMAX, start, period, prior))
    want = _chain(name, shared_B, mem, IMAX, start, period, prior)
    N, M, Gr, G2 = P.SHAPES[name]
    assert got[4].dtype == np.int32 and got[4].shape == (P.BATCH, Gr * G2)
    _eq(got, want)
    _eq(got, _whole(name, shared_B, start, period, prior))      # (the memspaces agree)
    for t in range(P.BATCH):                                    # a permutation; S lives on the head of the order in force
        assert np.array_equal(np.sort(got[4][t]), np.arange(1, Gr * G2 + 1))
        out = got[4][t][min(10 + 5 * IMAX, Gr * G2):] - 1
        assert not got[0][t].reshape(-1, order="F")[out].any()


# ---- (c) legs that pass the order on ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shared_B,mem", CASES)
def test_legs_that_pass_the_order_on_return_the_whole_call(name, shared_B, mem):
    for start, period, prior in POLICIES[:3]:
        whole = _whole(name, shared_B, start, period, prior)
        for legs in ((1, 5), (2, 4), (3, 1, 2)):
            state, order, done, rows = None, prior, 0, []
            for n in legs:
                S, Y, ce, state, order = _refresh(name, shared_B, mem, n, start, period, order, state=state, it0=done)
                rows.append(_np(ce))
                done += n
                if order is None:
                    order = False                               # (no refresh yet and no prior: still none)
            _eq((_np(S), _np(Y), np.concatenate(rows, axis=1), _np(state), _np(order)), whole)


# ---- (d) negative controls -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["R1", "R2"])
def test_the_policies_bind(name):
    every = _whole(name, False, 0, 1, False)[0]
    once = _whole(name, False, 2, 0, False)[0]
    plain = _np(_resume("approx", name, False, "host", IMAX)[0])
    for t in range(P.BATCH):
        assert not np.array_equal(every[t], once[t]) and not np.array_equal(every[t], plain[t]) and not np.array_equal(once[t], plain[t])
        assert np.count_nonzero(every[t]) <= 10 + 5 * IMAX < np.count_nonzero(plain[t])


# ---- (e) from a state that is no iterate of the problem ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shared_B", [("R1", False), ("R1", True), ("R2", False)])
def test_from_the_halved_state_of_another_trial_and_from_duplicate_magnitudes(name, shared_B):
    N, M, Gr, G2 = P.SHAPES[name]
    st = 0.5 * np.roll(_mid_state("approx", name, shared_B), -1, axis=0)
    dup = st.copy()                                             # a v of exact duplicate magnitudes (|3+4j| == |5|, |1| == |1j|, zeros)
    rng = np.random.default_rng(29)
    dup[:, 4 * N * M:4 * N * M + Gr * G2] = TIE_VALUES[rng.integers(0, TIE_VALUES.size, size=(P.BATCH, Gr * G2))]
    for s_in in (st, dup):
        keep = s_in.copy()
        for start, period, prior in ((0, 1, False), (4, 2, True)):
            got = _all(_refresh(name, shared_B, "host", 3, start, period, prior, state=s_in, it0=3))
            assert np.array_equal(s_in, keep)                   # state_in is not modified
            _eq(got, _chain(name, shared_B, "host", 3, start, period, prior, state=s_in, it0=3))


# ---- (f) a NaN stays in its trial ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["R1", "R2"])
def test_a_nan_in_one_trials_state_stays_in_that_trial(name):
    N, M, Gr, G2 = P.SHAPES[name]
    clean = _mid_state("approx", name, False)
    want = _all(_refresh(name, False, "host", 3, 0, 1, state=clean, it0=3))
    st = clean.copy()
    st[1, 5] = np.nan                                           # X(6, 1) of trial 1
    S, Y, ce, s_out, order = _all(_refresh(name, False, "host", 3, 0, 1, state=st, it0=3))
    assert not np.isfinite(Y[1]).all() and not np.isfinite(s_out[1]).all()
    assert np.array_equal(np.sort(order[1]), np.arange(1, Gr * G2 + 1))                        # (and its order is still a permutation)
    for t in (0, 2):
        assert np.isfinite(S[t]).all() and np.isfinite(Y[t]).all() and np.isfinite(ce[t]).all() and np.isfinite(s_out[t]).all()
        if min(N, M) <= 64:
            _eq((S[t], Y[t], ce[t], s_out[t], order[t]), tuple(w[t] for w in want))
        else:           # the global Jacobi sweeps the batch together (include/jstsp.h): the last bits may depend on the batch mates
            check_below("refresh64.%s.nan_mates" % name, max(rel_err(S[t], want[0][t]), rel_err(Y[t], want[1][t])), TOL64_S)


# ---- (g) refusals: the C ABI itself --------------------------------------------------------------------------------------------------------
def _raw(name, Imax, indx, n_indx, start, period, it0=0, state_in=None, order_out=None):
    from jstsp19_amd import solvers as SV
    arrs, _, prm = _inputs(name, False, "host")
    N, M, Gr, G2 = P.SHAPES[name]
    a = [SV._Arg(x, np.float64 if k == 1 else np.complex128, "arg") for k, x in enumerate(arrs)]
    c = SV._ctx_for(a, None)[0]
    sc = [SV._scalars(v, P.BATCH, "s")[1] for v in prm]
    outs = [SV._out(False, P.BATCH, r, cc, np.complex128) for r, cc in ((Gr, G2), (N, M))]
    ptr = lambda s: None if s is None else s.ctypes.data
    rc = c._lib.jstsp_proposed_refresh_f64(c.handle, N, M, Gr, G2, P.BATCH, a[0].ptr, a[1].ptr, a[2].ptr, 0, a[3].ptr, G2 * M, Imax, *sc,
                                           ptr(indx), n_indx, start, period, outs[0][0], outs[1][0], None, it0, ptr(state_in), None,
                                           ptr(order_out), 0)
    return rc


def test_refusals():
    import jstsp19_amd as J
    last = lambda: J.load().jstsp_last_error().decode()
    N, M, Gr, G2 = P.SHAPES["R1"]
    g = Gr * G2
    ix = np.ascontiguousarray(P.problem("R1", False)["indx_S"])
    st = _mid_state("approx", "R1", False)
    out = np.full((P.BATCH, g), -7, np.int32)
    for args in ((None, 0, -1, 1), (None, 0, 0, -1), (ix, 0, 0, 1), (ix, -3, 0, 1), (ix, g + 1, 0, 1), (None, 5, 0, 1)):
        assert _raw("R1", 2, *args, order_out=out) == E_ARG, args[1:]
        assert last().startswith(PREFIX + ": "), last()
    assert "n_indx = 5" in last()
    assert _raw("R1", 2, None, 0, 0, 1, it0=-1, state_in=st, order_out=out) == E_ARG and last().startswith(PREFIX + ": it0 = -1")
    assert _raw("R1", 2, None, 0, 0, 1, it0=3, order_out=out) == E_ARG and "without state_in" in last()
    assert _raw("R1", 2, None, 0, 0, 1, it0=2 ** 31 - 2, state_in=st, order_out=out) == E_ARG
    assert np.all(out == -7)                                    # nothing was written
    assert _raw("R1", 2, ix, g, 5, 1, order_out=out) == 0 and np.all(out == -7)                 # no refresh in the call: indx_out untouched
    assert _raw("R1", 2, ix, g, 1, 0, order_out=out) == 0 and np.all(np.sort(out, axis=1) == np.arange(1, g + 1))
    assert _raw("R1", 2, None, 0, 0, 1) == 0                    # indx_out NULL: not wanted


@pytest.mark.parametrize("memspace", [0, 1], ids=["host", "device"])
def test_a_batch_past_the_limit_is_refused_with_the_batch_that_fits_and_the_context_goes_on(memspace):
    from jstsp19_amd import _lib
    lib, ctx = _lib.load(), _lib.default_context(0)
    big, ones, dummy = 65535, np.ones(65535), np.zeros(1, complex)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    d = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    rc = lib.jstsp_proposed_refresh_f64(ctx.handle, 512, 512, 512, 512, big, p(dummy), p(dummy), p(dummy), 512 * 512, p(dummy), 512 * 512, 3,
                                        d(ones), d(ones), d(ones), None, 0, 0, 1, p(dummy), p(dummy), p(dummy), 0, None, None, p(dummy),
                                        memspace)
    msg = lib.jstsp_last_error().decode()
    assert rc == E_UNSUPPORTED and msg.startswith(PREFIX + ": "), (rc, msg)
    m = re.search(r"largest batch that fits is about (\d+)", msg)
    assert m and 1 <= int(m.group(1)) < big, msg
    assert _raw("R1", 1, None, 0, 0, 1) == 0                    # and the context goes on


# ---- (h) against the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shared_B,start,period", BOUNDED)
def test_against_the_restatement(name, shared_B, start, period):
    p = P.problem(name, shared_B)
    S, Y, ce, state, order = _whole(name, shared_B, start, period, False)
    tag = "refresh64.%s.%d_%d" % (name, start, period)
    for t in range(P.BATCH):
        m, prm, _ = P.trial(p, t)
        So, Yo, ceo, sto, oo = F.solve(*m, IMAX, *prm, start=start, period=period)
        check_below(tag + ".S", rel_err(S[t], So), TOL64_S)
        check_below(tag + ".Y", rel_err(Y[t], Yo), TOL64_S)
        check_below(tag + ".state", rel_err(state[t], sto), TOL64_S)
        check_below(tag + ".ce", ce_rel(ce[t], ceo), TOL64_CE)
        cnt = min(10 + 5 * IMAX, oo.size)                       # the last mask holds the restatement's entries
        np.testing.assert_array_equal(np.sort(order[t][:cnt]), np.sort(oo[:cnt]))
