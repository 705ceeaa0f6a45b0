"""jstsp_proposed_refresh_c32 (csrc/proposed.hip; proposed_algorithm_refresh): the fp32 ADMM whose support is refreshed from its own
iterate inside the loop, on the problems of tests/refresh32_problems.py and four branches of the loop, each confirmed the way
tests/test_gpu_resume32.py does (jstsp_last_dictionary_block, the "fused_pass" profile count, 0 fallbacks):

  T    64, 256, 64, 128, block-Toeplitz B of block height 64, JSTSP_H2=2     the window kernel of the fused pass
  G    the same shape with a generic B, JSTSP_H2=2                           the general fused pass
  G0   G with JSTSP_FUSED=0                                                  no pass: the three-kernel iteration
  R1   32, 140, 32, 16                                                       no pass (the shape does not take it)

each with and without convergence_error, batch 3.  What is exact is asserted on the bits (no refresh in the call; the hook; the
memspaces; the _c64 form; NaN isolation); what is a split fp32 solve or a comparison with float64 is held to TOL_S / TOL_CE of
tests/conftest.py, the latter on the trials the decision rule of refresh32_problems.py calls decided."""
import functools
import os

import numpy as np
import pytest

import refresh32_problems as Q
import refresh_ref as F
from conftest import TOL_CE, TOL_S, ce_rel, check_below, rel_err

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = -4, -3
BATCH, IMAX = Q.BATCH, Q.IMAX
CASES = ("T", "G", "G0", "R1")
PROBLEM = {"T": "T", "G": "G", "G0": "G", "R1": "R1"}
ENV = {"T": {"JSTSP_H2": "2"}, "G": {"JSTSP_H2": "2"}, "G0": {"JSTSP_H2": "2", "JSTSP_FUSED": "0"}, "R1": {}}
PREFIX = "proposed_algorithm refresh"


def _p(case):
    return Q.problem(PROBLEM[case])


def _dims(case):
    N, M, Gr, G2 = Q.SHAPES[PROBLEM[case]]
    return N, M, Gr, G2, Gr * G2, min(Gr * G2, F.TOP_MAX)


def _np(x):
    return x if x is None or isinstance(x, np.ndarray) else x.cpu().numpy()


def _run(case, kind, Imax, want_ce=True, env=None, mem="host", **kw):
    """One call under the case's switches.  kind: 'refresh' (kw: start, period, indx_S, state, it0), 'resume' (kw: indx_S, state,
    it0).  Returns (the call's outputs as numpy, fallbacks, fused passes launched, dictionary block)."""
    import jstsp19_amd as J
    p = _p(case)
    arrs = [p[k] for k in ("subY", "Omega", "A", "B")]
    if mem == "device":
        import torch
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        arrs = [J.colmajor(dev(a)) for a in arrs]
        kw = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    env = dict(ENV[case], **(env or {}))
    for k, v in env.items():
        os.environ[k] = v
    c = J.default_context(0)
    try:
        c.set_profiling(True)
        prm = (p["tau_Y"], p["tau_S"], p["rho"])
        if kind == "refresh":
            r = J.proposed_algorithm_refresh(*arrs, Imax, *prm, want_ce=want_ce, **kw)
        else:
            r = J.proposed_algorithm_resume(*arrs, Imax, *prm, "approximate", want_ce=want_ce, **kw)
        passes = c.get_profile("fused_pass")[0]
        c.set_profiling(False)
        return tuple(_np(x) for x in r), c.last_fused_fallbacks(), passes, c.last_dictionary_block()
    finally:
        for k in env:
            os.environ.pop(k, None)


def _on_branch(case, nfb, passes, block):
    assert nfb == 0 and (passes > 0) == (case in ("T", "G")) and block == (64 if case == "T" else 0), (case, nfb, passes, block)


def _eq(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), k
        if a is not None:
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def _flat(S):
    """(batch, Gr, G2) -> (batch, g) in column-major linear order"""
    return S.transpose(0, 2, 1).reshape(S.shape[0], -1)


def _v_of(state, case):
    N, M, Gr, G2, g, _ = _dims(case)
    return np.ascontiguousarray(state[:, 4 * N * M:4 * N * M + g].reshape(-1, G2, Gr).swapaxes(1, 2))


@functools.lru_cache(maxsize=None)
def _mid(case, want_ce=True, prior=False):
    """The state after three plain iterations (under the problem's indx_S with prior)."""
    return _run(case, "resume", 3, want_ce, indx_S=_p(case)["indx_S"] if prior else None)[0][3]


# ---- the raw C ABI, host memspace -------------------------------------------------------------------------------------------------------
def _raw(case, Imax, indx, n_indx, start, period, type=None, it0=0, state_in=None, state_out=None, order_out=None, c64=False, want_ce=True):
    """jstsp_proposed_refresh_c32 / _c64 itself.  Returns (rc, S, Y, ce) with the outputs as (batch, Gr, G2) / (batch, N, M) views."""
    from jstsp19_amd import _lib, solvers as SV
    p = _p(case)
    N, M, Gr, G2, g, _ = _dims(case)
    cdt, rdt = (np.complex128, np.float64) if c64 else (np.complex64, np.float32)
    a = [SV._Arg(p[k].astype(rdt if k == "Omega" else cdt), rdt if k == "Omega" else cdt, k) for k in ("subY", "Omega", "A", "B")]
    c = SV._ctx_for(a, None)[0]
    sc = [SV._scalars(p[k], BATCH, k)[1] for k in ("tau_Y", "tau_S", "rho")]
    S = np.full((BATCH, G2, Gr), -7, cdt); Y = np.full((BATCH, M, N), -7, cdt)
    ce = np.full((BATCH, 3, Imax), -7.0) if want_ce else None
    ptr = lambda s: None if s is None else s.ctypes.data
    fn = c._lib.jstsp_proposed_refresh_c64 if c64 else c._lib.jstsp_proposed_refresh_c32
    for k, v in ENV[case].items():
        os.environ[k] = v
    try:
        rc = fn(c.handle, N, M, Gr, G2, BATCH, a[0].ptr, a[1].ptr, a[2].ptr, 0, a[3].ptr, G2 * M, Imax, *sc,
                _lib.TYPE_APPROXIMATE if type is None else type, ptr(indx), n_indx, start, period, ptr(S), ptr(Y), ptr(ce), it0,
                ptr(state_in), ptr(state_out), ptr(order_out), _lib.HOST)
    finally:
        for k in ENV[case]:
            os.environ.pop(k, None)
    return rc, S.swapaxes(1, 2), Y.swapaxes(1, 2), None if ce is None else ce.swapaxes(1, 2)


# ---- 1. no refresh in the call: the resumed entries -----------------------------------------------------------------------------------
@pytest.mark.parametrize("want_ce", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_without_a_refresh_in_the_call_it_is_the_resumed_entry(case, want_ce):
    ix = _p(case)["indx_S"]
    for prior in (None, ix):
        want, nfb, passes, block = _run(case, "resume", IMAX, want_ce, indx_S=prior)
        _on_branch(case, nfb, passes, block)
        for start, period in ((IMAX, 1), (IMAX + 4, 0), (IMAX, 3)):
            got, nfb, passes, block = _run(case, "refresh", IMAX, want_ce, start=start, period=period, indx_S=prior)
            _on_branch(case, nfb, passes, block)
            _eq(got[:4], want)
            assert got[4] is prior                              # no refresh: the caller's indx_S comes back
        # a later leg that ends where the first refresh would begin
        mid = _mid(case, want_ce, prior is not None)
        got = _run(case, "refresh", 3, want_ce, start=5, period=1, indx_S=prior, state=mid, it0=2)[0]
        _eq(got[:4], _run(case, "resume", 3, want_ce, indx_S=prior, state=mid, it0=2)[0])
        assert got[4] is prior
    # the raw ABI: indx_out is not touched
    N, M, Gr, G2, g, R = _dims(case)
    out = np.full((BATCH, R), -7, np.int32)
    rc, S, Y, ce = _raw(case, IMAX, np.ascontiguousarray(ix), g, IMAX, 1, order_out=out, want_ce=want_ce)
    assert rc == 0 and np.all(out == -7)
    _eq((np.ascontiguousarray(S), np.ascontiguousarray(Y)), want[:2])


def test_an_order_of_fewer_entries_admits_nothing_else():
    ix = _p("R1")["indx_S"]
    short = np.ascontiguousarray(ix[:, :22])
    padded = np.concatenate([short, np.zeros((BATCH, ix.shape[1] - 22), np.int32)], axis=1)
    want = _run("R1", "resume", IMAX, indx_S=padded)[0]
    got = _run("R1", "refresh", IMAX, start=IMAX, period=0, indx_S=short)[0]
    _eq(got[:4], want)
    assert got[4] is short
    assert not np.array_equal(got[0], _run("R1", "resume", IMAX, indx_S=ix)[0][0])       # cnt(3) = 25 > 22: the full list admits more


# ---- 2. the hook, exactly ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_ce", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_one_refresh_at_the_last_iteration_is_the_plain_call_with_s_rewritten(case, want_ce):
    import jstsp19_amd as J
    N, M, Gr, G2, g, R = _dims(case)
    ix = _p(case)["indx_S"]
    for it0, k in ((0, 1), (0, 3), (3, 3)):
        for prior in (None, ix):
            state = _mid(case, want_ce, prior is not None) if it0 else None
            plain, nfb, passes, block = _run(case, "resume", k, want_ce, indx_S=prior, state=state, it0=it0)
            got, nfb2, passes2, block2 = _run(case, "refresh", k, want_ce, start=it0 + k - 1, period=0, indx_S=prior, state=state, it0=it0)
            if k > 1:
                _on_branch(case, nfb, passes, block)
                _on_branch(case, nfb2, passes2, block2)
            S, Y, ce, st, order = got
            v = _v_of(st, case)
            assert v.tobytes() == _v_of(plain[3], case).tobytes() and Y.tobytes() == plain[1].tobytes()
            assert order.dtype == np.int32 and order.shape == (BATCH, R)
            np.testing.assert_array_equal(order, J.support_top(v, R))
            cnt = min(10 + 5 * (it0 + k), g)
            Sf, Pf = _flat(S), _flat(plain[0])
            for t in range(BATCH):
                head = order[t, :cnt] - 1
                inside = np.zeros(g, bool); inside[head] = True
                assert not Sf[t, ~inside].any()                 # zero outside the new head, bit for bit (+0)
                assert Sf[t, ~inside].tobytes() == np.zeros(g - cnt, np.complex64).tobytes()
                if prior is None:
                    assert Sf[t, head].tobytes() == Pf[t, head].tobytes()
                else:                                           # equal bits wherever both masks admit the entry
                    both = inside.copy(); both[:] = False
                    both[np.intersect1d(head, prior[t, :cnt] - 1)] = True
                    assert Sf[t, both].tobytes() == Pf[t, both].tobytes()
            if want_ce:                                         # (the third column does not depend on the mask)
                assert ce[:, :, 2].tobytes() == plain[2][:, :, 2].tobytes()


# ---- 3. the order in force after the refresh ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _whole(case, start, period, want_ce=True):
    got, nfb, passes, block = _run(case, "refresh", IMAX, want_ce, start=start, period=period)
    _on_branch(case, nfb, passes, block)
    return got


@pytest.mark.parametrize("want_ce", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_the_order_stays_in_force_in_later_legs(case, want_ce):
    N, M, Gr, G2, g, R = _dims(case)
    whole = _whole(case, 2, 0, want_ce)
    first = _run(case, "refresh", 3, want_ce, start=2, period=0)[0]
    padded = np.concatenate([first[4], np.zeros((BATCH, g - R), np.int32)], axis=1)
    chains = (_run(case, "resume", 3, want_ce, indx_S=padded, state=first[3], it0=3)[0],
              _run(case, "refresh", 3, want_ce, start=2, period=0, indx_S=first[4], state=first[3], it0=3)[0])
    assert chains[1][4] is first[4]                             # the second leg runs no refresh: the order comes back as given
    for tag, (S, Y, ce, st, *_) in zip(("angles", "refresh"), chains):
        for t in range(BATCH):
            check_below("refresh32.%s.legs.%s.S" % (case, tag), rel_err(S[t], whole[0][t]), TOL_S)
            check_below("refresh32.%s.legs.%s.Y" % (case, tag), rel_err(Y[t], whole[1][t]), TOL_S)
            check_below("refresh32.%s.legs.%s.state" % (case, tag), rel_err(st[t], whole[3][t]), TOL_S)
            if want_ce:
                check_below("refresh32.%s.legs.%s.ce" % (case, tag), ce_rel(np.concatenate([first[2][t], ce[t]]), whole[2][t]), TOL_CE)
            assert np.count_nonzero(S[t]) <= 40
    for t in range(BATCH):
        assert np.count_nonzero(whole[0][t]) <= 40


# ---- 4. against the float64 restatement -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref(name, t, start, period):
    arrs, prm = Q.trial(Q.problem(name), t)
    return F.solve(*arrs, IMAX, *prm, start=start, period=period)


@pytest.mark.parametrize("want_ce", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_against_the_float64_restatement_on_decided_trials(case, want_ce):
    N, M, Gr, G2, g, R = _dims(case)
    cnt = min(10 + 5 * IMAX, g)
    compared = 0
    for start, period in Q.POLICIES:
        S, Y, ce, st, order = _whole(case, start, period, want_ce)
        for t in range(BATCH):
            if not Q.decided(PROBLEM[case], False, t, start, period):
                continue                                        # (left out of THIS test only; bounded by tests/test_refresh32_ref.py)
            compared += 1
            rS, rY, rce, rst, rorder = _ref(PROBLEM[case], t, start, period)
            tag = "refresh32.%s.ref" % case
            check_below(tag + ".S", rel_err(S[t].astype(np.complex128), rS), TOL_S)
            check_below(tag + ".Y", rel_err(Y[t].astype(np.complex128), rY), TOL_S)
            check_below(tag + ".state", rel_err(st[t].astype(np.complex128), rst), TOL_S)
            if want_ce:
                check_below(tag + ".ce", ce_rel(ce[t], rce), TOL_CE)
            assert set(order[t, :cnt]) == set(rorder[:cnt])     # the head of the order is the restatement's set
    assert compared >= 2 * len(Q.POLICIES)


# ---- 5. the re-solve ----------------------------------------------------------------------------------------------------------------------
def test_a_flagged_trial_is_solved_again_from_its_state_under_the_policy():
    import jstsp19_amd as J
    case = "G"
    N, M, Gr, G2, g, R = _dims(case)
    st3 = _mid(case)
    got, nfb, passes, _ = _run(case, "refresh", 3, start=0, period=1, state=st3, it0=3, env={"JSTSP_FUSED_KBACK": "-20"})
    assert nfb == BATCH and passes > 0
    # state_out == state_in through the raw ABI: the re-solve starts from the copy
    os.environ["JSTSP_FUSED_KBACK"] = "-20"
    try:
        inout = st3.copy()
        order2 = np.full((BATCH, R), -7, np.int32)
        rc, S2, Y2, ce2 = _raw(case, 3, None, 0, 0, 1, it0=3, state_in=inout, state_out=inout, order_out=order2)
        assert rc == 0 and J.default_context(0).last_fused_fallbacks() == BATCH
    finally:
        os.environ.pop("JSTSP_FUSED_KBACK", None)
    _eq((np.ascontiguousarray(S2), np.ascontiguousarray(Y2), np.ascontiguousarray(ce2), inout, order2), got)
    S, Y, ce, st, order = got
    cnt = min(10 + 5 * 6, g)
    for t in range(BATCH):
        assert np.array_equal(np.unique(order[t]), np.sort(order[t])) and np.unique(order[t]).size == R and order[t].min() >= 1 and order[t].max() <= g
        inside = np.zeros(g, bool); inside[order[t, :cnt] - 1] = True
        assert not _flat(S)[t, ~inside].any()
        arrs, prm = Q.trial(_p(case), t)
        s_in = st3[t].astype(np.complex128)
        if min(Q.boundary_gaps(arrs, prm, 3, 0, 1, state=s_in, it0=3), default=1.0) <= Q.GAP_MIN:
            continue
        rS, rY, rce, rst, _ = F.solve(*arrs, 3, *prm, start=0, period=1, state=s_in, it0=3)
        check_below("refresh32.G.resolve.S", rel_err(S[t].astype(np.complex128), rS), TOL_S)
        check_below("refresh32.G.resolve.Y", rel_err(Y[t].astype(np.complex128), rY), TOL_S)
        check_below("refresh32.G.resolve.state", rel_err(st[t].astype(np.complex128), rst), TOL_S)
        check_below("refresh32.G.resolve.ce", ce_rel(ce[t], rce), TOL_CE)


# ---- 6. negative controls ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["T", "R1"])
def test_the_policies_bind(case):
    every, once = _whole(case, 0, 1)[0], _whole(case, 2, 0)[0]
    plain = _run(case, "resume", IMAX)[0][0]
    for t in range(BATCH):
        assert not np.array_equal(every[t], once[t]) and not np.array_equal(every[t], plain[t]) and not np.array_equal(once[t], plain[t])
        assert np.count_nonzero(every[t]) <= 10 + 5 * IMAX < np.count_nonzero(plain[t])


# ---- 7. a NaN stays in its trial --------------------------------------------------------------------------------------------------------
def test_a_nan_in_one_trials_state_stays_in_that_trial():
    N, M, Gr, G2, g, R = _dims("R1")
    clean = _mid("R1")
    want = _run("R1", "refresh", 3, start=0, period=1, state=clean, it0=3)[0]
    st = clean.copy()
    st[1, 5] = np.nan                                           # X(6, 1) of trial 1
    S, Y, ce, s_out, order = _run("R1", "refresh", 3, start=0, period=1, state=st, it0=3)[0]
    assert not np.isfinite(Y[1]).all() and not np.isfinite(s_out[1]).all()
    assert np.array_equal(np.sort(order[1]), np.arange(1, g + 1))          # (and its order is still a permutation)
    for t in (0, 2):
        _eq((S[t], Y[t], ce[t], s_out[t], order[t]), tuple(w[t] for w in want))


# ---- 8. the memspaces -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["T", "R1"])
def test_host_and_device_memspace_return_the_same_bits(case):
    ix = _p(case)["indx_S"]
    for start, period, prior in ((0, 1, None), (1, 2, ix)):
        host = _run(case, "refresh", IMAX, start=start, period=period, indx_S=prior)[0]
        dev = _run(case, "refresh", IMAX, start=start, period=period, indx_S=prior, mem="device")[0]
        _eq(dev, host)
    mid = _mid(case)
    _eq(_run(case, "refresh", 3, start=0, period=1, state=mid, it0=3, mem="device")[0], _run(case, "refresh", 3, start=0, period=1, state=mid, it0=3)[0])


# ---- 9. refusals through the C ABI -----------------------------------------------------------------------------------------------------
def test_refusals():
    import jstsp19_amd as J
    from jstsp19_amd import _lib
    last = lambda: J.load().jstsp_last_error().decode()
    N, M, Gr, G2, g, R = _dims("R1")
    ix = np.ascontiguousarray(_p("R1")["indx_S"])
    st = _mid("R1")
    out = np.full((BATCH, R), -7, np.int32)
    outputs = []
    for args in ((None, 0, -1, 1), (None, 0, 0, -1), (ix, 0, 0, 1), (ix, -3, 0, 1), (ix, g + 1, 0, 1), (None, 5, 0, 1)):
        rc, *o = _raw("R1", 2, *args, order_out=out)
        assert rc == E_ARG, args[1:]
        assert last().startswith(PREFIX + ": "), last()
        outputs.append(o)
    assert "n_indx = 5" in last()
    rc, *o = _raw("R1", 2, None, 0, 0, 1, type=_lib.TYPE_STD, order_out=out)
    assert rc == E_UNSUPPORTED and last().startswith(PREFIX + ": 'std'"), last()
    outputs.append(o)
    rc, *o = _raw("R1", 2, None, 0, 0, 1, it0=-1, state_in=st, order_out=out)
    assert rc == E_ARG and last().startswith(PREFIX + ": it0 = -1")
    outputs.append(o)
    rc, *o = _raw("R1", 2, None, 0, 0, 1, it0=3, order_out=out)
    assert rc == E_ARG and last().startswith(PREFIX + ": ") and "without state_in" in last()
    outputs.append(o)
    assert np.all(out == -7)                                    # nothing was written
    for S, Y, ce in outputs:
        assert np.all(S == -7) and np.all(Y == -7) and np.all(ce == -7)
    rc, *_ = _raw("R1", 1, None, 0, 0, 1, order_out=out)        # and the context goes on
    assert rc == 0 and out.min() >= 1


# ---- 10. the _c64 form ----------------------------------------------------------------------------------------------------------------------
def test_the_c64_form_returns_the_c32_values():
    N, M, Gr, G2, g, R = _dims("R1")
    ne = 4 * N * M + 2 * g
    ix = np.ascontiguousarray(_p("R1")["indx_S"][:, :60])
    st = _mid("R1")
    for kw in (dict(it0=0), dict(it0=3, state_in=st)):
        o32, o64 = np.full((BATCH, R), -7, np.int32), np.full((BATCH, R), -7, np.int32)
        s32, s64 = np.zeros((BATCH, ne), np.complex64), np.zeros((BATCH, ne), np.complex128)
        kw64 = dict(kw, state_in=None if kw.get("state_in") is None else st.astype(np.complex128))
        rc, S, Y, ce = _raw("R1", 3, ix, 60, 1, 1, state_out=s32, order_out=o32, **kw)
        rc64, S64, Y64, ce64 = _raw("R1", 3, ix, 60, 1, 1, state_out=s64, order_out=o64, c64=True, **kw64)
        assert rc == 0 and rc64 == 0
        assert np.array_equal(S64, S.astype(np.complex128)) and np.array_equal(Y64, Y.astype(np.complex128))
        assert np.array_equal(s64, s32.astype(np.complex128)) and np.array_equal(ce64, ce) and np.array_equal(o64, o32) and o32.min() >= 1
