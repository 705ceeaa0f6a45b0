"""jstsp_proposed_until_c32 (csrc/proposed.hip, csrc/until.hip; proposed_algorithm_until): the fp32 Alg. 2 that stops each trial
when convergence_error(i, 3) <= tol[t], on the problems of tests/until32_problems.py - batch 3, tol (1e-1, 1e-2, 1e-3),
min_iters 2, Imax 24 - which reach the four branches of the loop (confirmed as tests/test_gpu_resume32.py confirms them):

  a  the window kernel of the fused pass     b  the general fused pass     c  b with JSTSP_FUSED=0     d  a shape without a pass

iters equal those of tests/until_ref.py (float64 on the same complex64 values; every decision keeps a margin of 5e-2, a hundred
times TOL_CE: tests/test_until32_ref.py); S, Y, the state, convergence_error and ce3 are within TOL_S / TOL_CE of tests/conftest.py
of that reference, and S, Y, the state within TOL_S of the sibling run for the trial alone over iters[t] iterations (whether the
bits are equal is recorded beside the measured deviations, through check_below with a bound it cannot miss, not asserted).
To the bit: check 1, 3, 64; the other trials' tol; duplicates in one batch; and with no positive tol the sibling itself."""
import functools
import os

import numpy as np
import pytest

import refresh_ref as F
import until32_problems as P
from conftest import TOL_CE, TOL_S, ce_rel, check_below, rel_err

pytestmark = pytest.mark.gpu

E_NULL, E_ARG, E_UNSUPPORTED = -1, -4, -3
_BITS = {}


def _np(x):
    return x if x is None or isinstance(x, np.ndarray) else x.cpu().numpy()


def _dev(a, colmajor=True):
    import torch
    import jstsp19_amd as J
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return J.colmajor(t) if colmajor else t


def _args(case, mem, sel=None, subY=None):
    p = P.problem(case)
    sel = list(range(P.BATCH)) if sel is None else list(sel)
    arrs = [p["subY"][sel] if subY is None else subY, p["Omega"][sel], p["A"], p["B"][sel]]
    ix = np.ascontiguousarray(p["indx_S"][sel])
    if mem == "device":
        import torch
        arrs = [_dev(a) for a in arrs]
        ix = torch.from_numpy(ix).to("cuda:0")
    return arrs, ix, (p["tau_Y"][sel], p["tau_S"][sel], p["rho"][sel])


def _run(case, fn, env=None):
    """fn(J) under the case's switches with profiling on: (its result as numpy, fallbacks, fused passes, dictionary block)"""
    import jstsp19_amd as J
    env = dict(P.ENV[case], **(env or {}))
    for k, v in env.items():
        os.environ[k] = v
    c = J.default_context(0)
    try:
        c.set_profiling(True)
        r = fn(J)
        passes = c.get_profile("fused_pass")[0]
        c.set_profiling(False)
        return tuple(_np(x) for x in r), c.last_fused_fallbacks(), passes, c.last_dictionary_block()
    finally:
        for k in env:
            os.environ.pop(k, None)


def _until(case, mem="host", tols=P.TOL, sel=None, use_indx=False, refresh=None, state=None, Imax=P.IMAX, env=None, subY=None, full=False,
           **kw):
    arrs, ix, prm = _args(case, mem, sel, subY)
    if state is not None and mem == "device":
        state = _dev(state, colmajor=False)
    kw.setdefault("want_ce", True)
    out = _run(case, lambda J: J.proposed_algorithm_until(*arrs, Imax, *prm, tol=tols, indx_S=ix if use_indx else None, refresh=refresh,
                                                          state=state, **kw), env)
    return out if full else out[0]


@functools.lru_cache(maxsize=None)
def _alone(case, t, Imax, use_indx=False, refresh=None, warm=False):
    """The sibling for trial t alone (a batch of one, host path) under the case's switches: (S, Y, ce, state[, order]) without the batch axis."""
    arrs, ix, prm = _args(case, "host", [t])
    kw = dict(indx_S=ix if use_indx else None)
    if warm:
        kw.update(state=P.warm_state("b" if case == "c" else case, (t + 1) % P.BATCH)[None], it0=P.WARM_IT0)
    if refresh is None:
        fn = lambda J: J.proposed_algorithm_resume(*arrs, Imax, *prm, **kw)
    else:
        fn = lambda J: J.proposed_algorithm_refresh(*arrs, Imax, *prm, start=refresh[0], period=refresh[1], **kw)
    return tuple(x[0] for x in _run(case, fn)[0])


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_outputs(out, want, sel=slice(None)):
    for a, b in zip(out, want):
        assert (a is None) == (b is None)
        if a is not None:
            _same(a[sel], b[sel])


def _against_the_reference(tag, out, ref, want_ce=True, state=True):
    S, Y, ce, st, order, iters, c3 = out
    assert iters.dtype == np.int32 and iters.tolist() == [got[5] for got in ref]
    for t, got in enumerate(ref):
        n = got[5]
        check_below(tag + ".S", rel_err(S[t].astype(np.complex128), got[0]), TOL_S)
        check_below(tag + ".Y", rel_err(Y[t].astype(np.complex128), got[1]), TOL_S)
        if state:
            check_below(tag + ".state", rel_err(st[t].astype(np.complex128), got[3]), TOL_S)
        check_below(tag + ".ce3", abs(c3[t] - got[6]) / abs(got[6]), TOL_CE)
        if want_ce:
            check_below(tag + ".ce", ce_rel(ce[t, :n], got[2][:n]), TOL_CE)
            assert np.isnan(ce[t, n:]).all()


def _branch(case, nfb, passes, block):
    assert nfb == 0 and (passes > 0) == (case in ("a", "b")) and block == (64 if case == "a" else 0), (case, nfb, passes, block)


# ---- iterations and values against the reference: every branch, policy, with and without indx_S, both memspaces, with and without ce ----
@pytest.mark.parametrize("use_indx", [False, True], ids=["plain", "indx"])
@pytest.mark.parametrize("refresh", P.POLICIES, ids=["none", "0_1", "2_3"])
@pytest.mark.parametrize("case", P.CASES)
def test_iters_and_values_of_the_reference(case, refresh, use_indx):
    ref = P.reference(case, refresh, use_indx, want_ce=True)
    tag = "until32.%s.%s%s" % (case, "plain" if refresh is None else "%d_%d" % refresh, ".indx" if use_indx else "")
    for mem in ("host", "device"):
        out, nfb, passes, block = _until(case, mem, refresh=refresh, use_indx=use_indx, full=True)
        print(tag, mem, out[5], out[6])
        _branch(case, nfb, passes, block)
        _against_the_reference(tag, out, ref)
        for k, tl in enumerate(P.TOL):                          # the rule, on the solver's own numbers
            assert P.MIN_ITERS <= out[5][k] < P.IMAX and out[6][k] <= tl
        two = _until(case, mem, refresh=refresh, use_indx=use_indx, want_ce=False, return_state=False)
        assert two[2] is None and two[3] is None
        _against_the_reference(tag + ".two", two, ref, want_ce=False, state=False)


# ---- against the sibling run for the trial alone over iters[t] iterations ------------------------------------------------------------
@pytest.mark.parametrize("case", P.CASES)
def test_values_of_the_sibling_alone_and_its_order(case):
    for refresh, use_indx in ((None, False), (None, True), ((0, 1), False), ((2, 3), False), ((2, 3), True)):
        out = _until(case, "host", refresh=refresh, use_indx=use_indx)
        S, Y, ce, st, order, iters, c3 = out
        key = "%s.%s%s" % (case, "plain" if refresh is None else "%d_%d" % refresh, ".indx" if use_indx else "")
        for t in range(P.BATCH):
            n = int(iters[t])
            want = _alone(case, t, n, use_indx, refresh)
            tag = "until32.sibling." + key
            check_below(tag + ".S", rel_err(S[t], want[0]), TOL_S)
            check_below(tag + ".Y", rel_err(Y[t], want[1]), TOL_S)
            check_below(tag + ".state", rel_err(st[t], want[3]), TOL_S)
            if refresh is not None:
                if F.schedule(0, n, *refresh):
                    _same(order[t], want[4])
                else:                                           # stopped before its first refresh: no list
                    assert not order[t].any()
            _BITS["%s.t%d" % (key, t)] = bool(S[t].tobytes() == want[0].tobytes() and Y[t].tobytes() == want[1].tobytes()
                                              and st[t].tobytes() == want[3].tobytes())
    print({k: v for k, v in _BITS.items() if k.startswith(case + ".")})
    # recorded, not asserted: 1 = some trial of the case differs from the sibling in a bit, 0 = none does
    check_below("until32.sibling.%s.differs_in_a_bit" % case, float(not all(v for k, v in _BITS.items() if k.startswith(case + "."))), 2.0)


# ---- to the bit, across configurations -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.CASES)
def test_check_the_other_trials_tol_and_duplicates_change_no_byte(case):
    for refresh in (None, (2, 3)):
        base = _until(case, "device", refresh=refresh, check=1)
        assert base[5].tolist() == P.STOPS[case]
        for check in (3, 64):
            _same_outputs(_until(case, "device", refresh=refresh, check=check), base)
    base = _until(case, "host", check=1)
    for t in range(P.BATCH):
        for other in (0.0, 1e300):                              # the others never stop / stop at min_iters
            tols = [P.TOL[k] if k == t else other for k in range(P.BATCH)]
            out = _until(case, "host", tols=tols)
            assert out[5].tolist() == [P.STOPS[case][k] if k == t else (P.IMAX if other == 0.0 else P.MIN_ITERS) for k in range(P.BATCH)]
            _same_outputs(out, base, t)
    six = _until(case, "device", tols=P.TOL * 2, sel=[0, 1, 2, 0, 1, 2])
    assert six[5].tolist() == P.STOPS[case] * 2
    for x in six:
        if x is not None:                                       # (no order without a policy)
            _same(x[:3], x[3:])


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("case", P.CASES)
def test_without_a_positive_tol_it_is_the_sibling(case, mem):
    arrs, ix, prm = _args(case, mem)
    n = 6
    want = _run(case, lambda J: J.proposed_algorithm_resume(*arrs, n, *prm))[0]
    for tol in (0.0, (-1.0, np.nan, 0.0)):
        out = _until(case, mem, tols=tol, Imax=n, check=1)
        _same_outputs(out[:4], want)
        assert out[4] is None and out[5].tolist() == [n] * P.BATCH
        _same(out[6], want[2][:, -1, 2])
    want = _run(case, lambda J: J.proposed_algorithm_resume(*arrs, n, *prm, want_ce=False, return_state=False))[0]
    _same_outputs(_until(case, mem, tols=0.0, Imax=n, want_ce=False, return_state=False)[:4], want)
    want = _run(case, lambda J: J.proposed_algorithm_refresh(*arrs, n, *prm, start=2, period=3, indx_S=ix))[0]
    _same_outputs(_until(case, mem, tols=np.nan, Imax=n, refresh=(2, 3), use_indx=True)[:5], want)


# ---- the loop leaves early, and the side streams are joined --------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b"])
def test_the_loop_leaves_early_and_the_next_call_is_undisturbed(case):
    import jstsp19_amd as J
    arrs, _, prm = _args(case, "device")
    plain = lambda: _run(case, lambda J_: J_.proposed_algorithm(*arrs, 5, *prm))
    want, _, fixed, _ = _run(case, lambda J_: J_.proposed_algorithm_resume(*arrs, P.IMAX, *prm))
    first = plain()[0]
    for check in (1, 2, 5):
        out, nfb, passes, block = _until(case, "device", check=check, full=True)
        after = plain()[0]                                      # at once, on the same context
        _branch(case, nfb, passes, block)
        assert passes <= max(out[5]) + check - 1 and passes < fixed, (passes, fixed, out[5])
        _same_outputs(after, first)
    assert fixed == P.IMAX - 1


# ---- a trial flagged by the pass is solved again under the rule ---------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
def test_every_trial_solved_again_stops_where_the_reference_stops(mem):
    ref = P.reference("b", None, False, want_ce=True)
    out, nfb, passes, _ = _until("b", mem, env={"JSTSP_FUSED_KBACK": "-20"}, full=True)
    assert nfb == P.BATCH and passes > 0
    _against_the_reference("until32.b.resolve", out, ref)
    out, nfb, _, _ = _until("b", mem, env={"JSTSP_FUSED_KBACK": "-20"}, refresh=(2, 3), full=True)
    assert nfb == P.BATCH
    _against_the_reference("until32.b.resolve.2_3", out, P.reference("b", (2, 3), False, want_ce=True))


# ---- other cases of the rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.CASES)
def test_a_late_min_iters_and_a_warm_start(case):
    ref = P.reference(case, None, False, P.MIN_ITERS_LATE, want_ce=True)
    out = _until(case, "device", min_iters=P.MIN_ITERS_LATE)
    assert out[5].tolist() == [max(P.MIN_ITERS_LATE, n) for n in P.STOPS[case]]
    _against_the_reference("until32.%s.late" % case, out, ref)
    rcase = "b" if case == "c" else case
    warm = np.stack([P.warm_state(rcase, (t + 1) % P.BATCH) for t in range(P.BATCH)])      # trial t from the state of trial t + 1
    ref = P.reference(case, None, False, P.MIN_ITERS, True, tols=(P.WARM_TOL,) * P.BATCH, want_ce=True)
    for mem in ("host", "device"):
        out = _until(case, mem, tols=P.WARM_TOL, state=warm, it0=P.WARM_IT0)
        _against_the_reference("until32.%s.warm" % case, out, ref)


@pytest.mark.parametrize("case", P.CASES)
def test_two_legs_stop_where_the_whole_call_stops(case):
    ref = P.reference(case, None, False)
    a = _until(case, "host", Imax=5)
    go = [t for t in range(P.BATCH) if not (a[5][t] >= P.MIN_ITERS and a[6][t] <= P.TOL[t])]      # came back unstopped
    assert go == [1, 2] and a[5].tolist() == [ref[0][5], 5, 5]
    b = _until(case, "host", tols=[P.TOL[t] for t in go], sel=go, state=a[3][go], it0=5, Imax=P.IMAX - 5)
    assert (5 + b[5]).tolist() == [ref[t][5] for t in go]
    check_below("until32.%s.legs.S" % case, rel_err(a[0][0].astype(np.complex128), ref[0][0]), TOL_S)
    for k, t in enumerate(go):
        check_below("until32.%s.legs.S" % case, rel_err(b[0][k].astype(np.complex128), ref[t][0]), TOL_S)
        check_below("until32.%s.legs.state" % case, rel_err(b[3][k].astype(np.complex128), ref[t][3]), TOL_S)


@pytest.mark.parametrize("case", P.CASES)
def test_a_nan_in_one_trials_data_leaves_the_others_alone(case):
    bad = P.problem(case)["subY"].copy()
    bad[1, 3, 5] = np.nan
    out = _until(case, "host", subY=bad)
    assert out[5][1] == P.IMAX and np.isnan(out[6][1])          # (a NaN never stops its trial)
    clean = _until(case, "host")
    for t in (0, 2):
        _same_outputs(out[:4] + out[5:], clean[:4] + clean[5:], t)


# ---- the C ABI: the _c64 form and the refusals -------------------------------------------------------------------------------------------
def _raw(entry="jstsp_proposed_until_c32", tol=P.TOL, min_iters=2, check=4, iters=True, type_=0, period=-1, start=0, it0=0, Imax=P.IMAX,
         n_indx=0):
    """The entry on case d, host arrays, no indx_S, every output: (rc, S, Y, ce, state, iters, ce3)"""
    from jstsp19_amd import solvers as SV
    wide = entry.endswith("c64")
    cdt, rdt = (np.complex128, np.float64) if wide else (np.complex64, np.float32)
    arrs, _, prm = _args("d", "host")
    N, M, Gr, G2 = P.SHAPES["d"]
    a = [SV._Arg(x.astype(rdt if k == 1 else cdt), rdt if k == 1 else cdt, "arg") for k, x in enumerate(arrs)]
    c = SV._ctx_for(a, None)[0]
    sc = [SV._scalars(v, P.BATCH, "s")[1] for v in prm]
    outs = [SV._out(False, P.BATCH, r, cc, dt) for r, cc, dt in ((Gr, G2, cdt), (N, M, cdt), (Imax, 3, np.float64))]
    st = np.zeros((P.BATCH, 4 * N * M + 2 * Gr * G2), cdt)
    it, c3 = np.full(P.BATCH, -7, np.int32), np.full(P.BATCH, -7.0)
    ptol = None if tol is None else SV._scalars(tol, P.BATCH, "tol")[1]
    rc = getattr(c._lib, entry)(c.handle, N, M, Gr, G2, P.BATCH, a[0].ptr, a[1].ptr, a[2].ptr, 0, a[3].ptr, G2 * M, Imax, *sc, type_, None,
                                n_indx, start, period, ptol, min_iters, check, outs[0][0], outs[1][0], outs[2][0], it0, None, st.ctypes.data,
                                None, it.ctypes.data if iters else None, c3.ctypes.data, 0)
    return (rc,) + tuple(x[1](False) for x in outs) + (st, it, c3)


def test_the_c64_form_is_the_c32_form_on_shape_d():
    lo, hi = _raw(), _raw("jstsp_proposed_until_c64")
    assert lo[0] == 0 and hi[0] == 0 and lo[5].tolist() == P.STOPS["d"]
    for a, b in zip(lo[1:5], hi[1:5]):
        assert b.dtype in (np.complex128, np.float64)
        _same(a.astype(b.dtype), b)
    _same(lo[5], hi[5]); _same(lo[6], hi[6])
    _same_outputs(lo[1:5] + (lo[5], lo[6]), [x for x in _until("d", "host", check=4) if x is not None])


def test_refusals():
    import jstsp19_amd as J
    last = lambda: J.load().jstsp_last_error().decode()
    prefix = "proposed_algorithm until: "
    r = _raw(min_iters=0)
    assert r[0] == E_ARG and last().startswith(prefix) and "min_iters = 0" in last() and np.all(r[5] == -7)
    assert _raw(check=0)[0] == E_ARG and "check = 0" in last()
    assert _raw(iters=False)[0] == E_NULL and last().startswith(prefix)
    assert _raw(tol=None)[0] == E_NULL
    assert _raw(type_=1)[0] == E_UNSUPPORTED and "'std'" in last()
    assert _raw(type_=7)[0] == E_ARG
    r = _raw(it0=3)
    assert r[0] == E_ARG and "without state_in" in last()                    # the siblings' refusals
    assert _raw(period=1, start=-1)[0] == E_ARG and _raw(n_indx=5)[0] == E_ARG
    assert np.all(r[5] == -7) and np.all(r[6] == -7.0)                       # nothing was written
    r = _raw(Imax=2)
    assert r[0] == 0 and r[5].tolist() == [2, 2, 2]                          # and the context goes on
    arrs, ix, prm = _args("d", "host")
    for kw in (dict(min_iters=0), dict(check=0), dict(type="std"), dict(refresh=(-1, 1)), dict(refresh=(0, -1)), dict(it0=3),
               dict(tol=(1e-3, 1e-3)), dict(indx_S=ix[:, :0])):
        with pytest.raises(ValueError):
            J.proposed_algorithm_until(*arrs, 4, *prm, **{"tol": 1e-3, **kw})
    with pytest.raises(TypeError):                              # tol is required
        J.proposed_algorithm_until(*arrs, 4, *prm)
