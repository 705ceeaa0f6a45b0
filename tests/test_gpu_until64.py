"""jstsp_proposed_until_f64 (csrc/proposed64.hip; proposed_algorithm_until_f64): the float64 Alg. 2 that stops each trial when
convergence_error(i, 3) <= tol[t], on the problems of tests/resume_problems.py, Imax = 40, min_iters = 2, per-trial tol
(1e-2, 1e-3, 1e-4) - three distinct stops - and (1e-2, 0, 1e-4) - one trial that runs to Imax.

R1 (Gram order 32, the in-LDS Jacobi): iters equal those of tests/until_ref.py (every decision keeps a margin of 1e-3 from its
threshold: tests/test_until_ref.py, without a GPU), and for every trial S, Y, the state, the order and the rows of
convergence_error are, bit for bit, what the sibling - proposed_algorithm_resume_f64, with a policy proposed_algorithm_refresh_f64 -
returns for that trial ALONE at Imax = iters[t]; rows beyond iters[t] are NaN.  For check in {1, 3, 64}, both memspaces, B shared
and per trial, indx_S, two policies, a batch of duplicates, warm starts, legs, tol = 0, a NaN trial, a batch that stops as one.

R2 (Gram order 72 > 64): eig64_global without `freeze` - what this solver family runs - sweeps on while ANY matrix of the call is
above the stop criterion (csrc/vamp64.hip, eig64: the loop over hoff), so a converged matrix is rotated again with its batch mates
and a trial's last bits depend on them.  THE BITS CONTRACT COVERS min(N, M) <= 64; on R2 iters equal the reference's and S, Y are
within TOL64_S = 1e-10 of max|ref| (the float64 solver's bound against its restatement, tests/test_gpu_resume64.py)."""
import functools

import numpy as np
import pytest

import refresh_ref as F
import resume_problems as P
import until_ref as U
from conftest import check_below, rel_err  # noqa: E402
from test_gpu_resume64 import TOL64_S, _np

pytestmark = pytest.mark.gpu

E_NULL, E_ARG = -1, -4
CHECKS = (1, 3, 64)                 # 64 > Imax: no compaction before the end
R1_CONFIGS = [c for c in U.CONFIGS if c[0] == "R1"]
R2_CONFIGS = [c for c in U.CONFIGS if c[0] == "R2"]


def _args(name, shared_B, mem, sel=None):
    """(subY, Omega, A, B), indx_S and the scalars of the trials `sel` (default: the three), numpy or column-major torch CUDA."""
    p = P.problem(name, shared_B)
    sel = list(range(P.BATCH)) if sel is None else list(sel)
    arrs = [p["subY"][sel], p["Omega"][sel], p["A"], p["B"] if shared_B else p["B"][sel]]
    ix = np.ascontiguousarray(p["indx_S"][sel])
    if mem == "device":
        import torch
        import jstsp19_amd as J
        dev = torch.device("cuda:0")
        arrs = [J.colmajor(torch.from_numpy(np.ascontiguousarray(a)).to(dev)) for a in arrs]
        ix = torch.from_numpy(ix).to(dev)
    return arrs, ix, (p["tau_Y"][sel], p["tau_S"][sel], p["rho"][sel])


def _state_arg(state, mem):
    if state is None or mem == "host":
        return state
    import torch
    return torch.from_numpy(np.ascontiguousarray(state)).to(torch.device("cuda:0"))


def _until(name, shared_B, mem, tol, sel=None, use_indx=False, refresh=None, state=None, Imax=U.IMAX, indx=None, subY=None, **kw):
    """The call under test as numpy arrays (None stays None).  indx: an order in force instead of the problem's; subY: other data."""
    import jstsp19_amd as J
    arrs, ix, prm = _args(name, shared_B, mem, sel)
    if subY is not None:
        arrs[0] = subY
    if indx is not None:
        ix, use_indx = _state_arg(indx, mem), True
    kw.setdefault("want_ce", True)
    out = J.proposed_algorithm_until_f64(*arrs, Imax, *prm, tol=tol, indx_S=ix if use_indx else None, refresh=refresh,
                                         state=_state_arg(state, mem), **kw)
    return tuple(None if x is None else _np(x) for x in out)


@functools.lru_cache(maxsize=None)
def _alone(name, shared_B, t, Imax, use_indx=False, refresh=None, warm=False):
    """The sibling for trial t alone (a batch of one, host path), once per session: (S, Y, ce, state[, order]) without the batch axis."""
    import jstsp19_amd as J
    arrs, ix, prm = _args(name, shared_B, "host", [t])
    kw = dict(indx_S=ix if use_indx else None)
    if warm:
        kw.update(state=_warm_states(name, shared_B)[(t + 1) % P.BATCH][None], it0=U.WARM_IT0)
    if refresh is None:
        out = J.proposed_algorithm_resume_f64(*arrs, Imax, *prm, **kw)
    else:
        out = J.proposed_algorithm_refresh_f64(*arrs, Imax, *prm, start=refresh[0], period=refresh[1], **kw)
    return tuple(_np(x)[0] for x in out)


@functools.lru_cache(maxsize=None)
def _warm_states(name, shared_B):
    """The 30-iteration states of the three trials (plain Alg. 2 from zero)."""
    import jstsp19_amd as J
    arrs, _, prm = _args(name, shared_B, "host")
    return _np(J.proposed_algorithm_resume_f64(*arrs, U.WARM_IT0, *prm, want_ce=False)[3])


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.tobytes() == b.tobytes()


def _assert_trials(out, name, shared_B, sel, use_indx=False, refresh=None, warm=False, it0=0, ce3=True):
    """Every slot k of `out` holds the bits of trial sel[k] alone over iters[k] iterations."""
    S, Y, ce, state, order, iters, c3 = out
    assert iters.dtype == np.int32 and iters.shape == (len(sel),) and c3.shape == (len(sel),)
    for k, t in enumerate(sel):
        n = int(iters[k])
        want = _alone(name, shared_B, t, n, use_indx, refresh, warm)
        _same(S[k], want[0]); _same(Y[k], want[1]); _same(state[k], want[3])
        _same(ce[k, :n], want[2])
        assert np.isnan(ce[k, n:]).all()
        if ce3:
            _same(c3[k], want[2][n - 1, 2])
        if refresh is not None and order is not None and not use_indx:
            if F.schedule(it0, n, *refresh):
                _same(order[k], want[4])
            else:                                               # stopped before its first refresh: no list
                assert not order[k].any()


def _ref_iters(name, shared_B, use_indx, refresh, tols, **kw):
    return [got[5] for got in U.reference(name, shared_B, use_indx, refresh, tuple(tols), **kw)]


# ---- 1, 2, 3: iters of the reference, the bits of the sibling alone, every check, both memspaces -------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("name,shared_B,use_indx,refresh", R1_CONFIGS)
def test_iters_of_the_reference_and_the_bits_of_the_sibling_alone(name, shared_B, use_indx, refresh, mem):
    for key in ("abc", "a0c") if (shared_B, use_indx, refresh) == (False, False, None) else ("abc",):
        tols = U.TOLS[key]
        want_iters = _ref_iters(name, shared_B, use_indx, refresh, tols)
        first = None
        for check in CHECKS:
            out = _until(name, shared_B, mem, tols, use_indx=use_indx, refresh=refresh, check=check)
            print(name, shared_B, use_indx, refresh, mem, key, check, out[5], out[6])
            assert out[5].tolist() == want_iters
            _assert_trials(out, name, shared_B, range(P.BATCH), use_indx, refresh)
            for k, t in enumerate(tols):                        # a trial that ran fewer than Imax iterations met the rule
                assert out[5][k] == U.IMAX or (out[5][k] >= U.MIN_ITERS and out[6][k] <= t)
            first = first or out
            for a, b in zip(out, first):                        # (check changes nothing)
                if a is not None:
                    _same(a, b)
        S, Y, ce, state, order, iters, c3 = _until(name, shared_B, mem, tols, use_indx=use_indx, refresh=refresh, want_ce=False,
                                                   return_state=False)
        assert ce is None and state is None and iters.tolist() == want_iters
        _same(S, first[0]); _same(Y, first[1])


@pytest.mark.parametrize("check", CHECKS)
def test_a_batch_of_duplicates_returns_identical_bits(check):
    sel = [0, 1, 2, 0, 1, 2]
    out = _until("R1", False, "device", U.TOLS["abc"] * 2, sel=sel, check=check)
    assert out[5].tolist() == _ref_iters("R1", False, False, None, U.TOLS["abc"]) * 2
    for x in out:
        if x is not None:
            _same(x[:3], x[3:])
    _assert_trials(out, "R1", False, sel)
    # a batch of 20: the one trial that stops first is too few to move the other 19 for (it runs on, captured), the next ten are not
    sel = [0] + [1] * 10 + [2] * 9
    out = _until("R1", False, "device", [U.TOLS["abc"][t] for t in sel], sel=sel, check=check)
    assert out[5].tolist() == [_ref_iters("R1", False, False, None, U.TOLS["abc"])[t] for t in sel]
    _assert_trials(out, "R1", False, sel)


# ---- 4: warm starts, min_iters, legs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
def test_a_warm_start_stops_at_its_first_iteration_and_min_iters_moves_it(mem):
    warm = np.roll(_warm_states("R1", False), -1, axis=0)       # trial t from the state of trial t + 1
    tols = (U.WARM_TOL,) * P.BATCH
    for min_iters in (1, 5):
        out = _until("R1", False, mem, U.WARM_TOL, state=warm, it0=U.WARM_IT0, min_iters=min_iters, check=1)
        assert out[5].tolist() == _ref_iters("R1", False, False, None, tols, min_iters=min_iters, warm=True) == [min_iters] * P.BATCH
        _assert_trials(out, "R1", False, range(P.BATCH), warm=True, it0=U.WARM_IT0)


@pytest.mark.parametrize("refresh", [None, (2, 3)])
def test_two_legs_of_an_unstopped_trial_are_one_call(refresh):
    tols = U.TOLS["abc"]
    whole = _until("R1", False, "host", tols, refresh=refresh)
    a = _until("R1", False, "host", tols, refresh=refresh, Imax=10)
    go = [t for t in range(P.BATCH) if not (a[5][t] >= U.MIN_ITERS and a[6][t] <= tols[t])]      # came back unstopped
    assert go == [1, 2] and a[5].tolist() == [whole[5][0], 10, 10]
    order = np.ascontiguousarray(a[4][go]) if refresh else None     # the order in force goes on with the state
    b = _until("R1", False, "host", [tols[t] for t in go], sel=go, indx=order, refresh=refresh, state=a[3][go], it0=10, Imax=30)
    assert (10 + b[5]).tolist() == whole[5][go].tolist()
    for k, t in enumerate(go):
        n = int(b[5][k])
        _same(b[0][k], whole[0][t]); _same(b[1][k], whole[1][t]); _same(b[3][k], whole[3][t]); _same(b[6][k], whole[6][t])
        _same(np.concatenate([a[2][t, :10], b[2][k, :n]]), whole[2][t, :10 + n])
        if refresh:
            _same(b[4][k], whole[4][t])
    _same(a[0][0], whole[0][0]); _same(a[3][0], whole[3][0])


# ---- 5: no positive tol: the sibling ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("name", ["R1", "R2"])
def test_without_a_positive_tol_it_is_the_sibling(name, mem):
    import jstsp19_amd as J
    arrs, ix, prm = _args(name, False, mem)
    want = tuple(_np(x) for x in J.proposed_algorithm_resume_f64(*arrs, 12, *prm, indx_S=ix))
    for tol in (0.0, (-1.0, np.nan, 0.0)):
        out = _until(name, False, mem, tol, use_indx=True, Imax=12, check=1)
        for a, b in zip(out[:4], want):
            _same(a, b)
        assert out[5].tolist() == [12] * P.BATCH
        _same(out[6], want[2][:, -1, 2])
    want = tuple(_np(x) for x in J.proposed_algorithm_refresh_f64(*arrs, 12, *prm, start=2, period=3))
    out = _until(name, False, mem, 0.0, refresh=(2, 3), Imax=12)
    for a, b in zip(out[:5], want):
        _same(a, b)


# ---- 6: a NaN stays in its trial --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("check", [1, 3])
def test_a_nan_in_one_trials_data_leaves_the_others_alone(check):
    bad = _args("R1", False, "host")[0][0].copy()
    bad[1, 3, 5] = np.nan
    tols = U.TOLS["abc"]
    out = _until("R1", False, "host", tols, check=check, subY=bad)
    assert out[5].tolist()[1] == U.IMAX and np.isnan(out[6][1])     # (a NaN never stops its trial; its S is soft(NaN) = 0)
    clean = _until("R1", False, "host", tols, check=check)
    for t in (0, 2):
        assert out[5][t] == clean[5][t]
        for a, b in zip(out[:4] + out[5:], clean[:4] + clean[5:]):
            _same(a[t], b[t])


# ---- 7: every trial stops at the same iteration: the loop leaves early ------------------------------------------------------------------
@pytest.mark.parametrize("check", [1, 7, 64])
def test_a_batch_that_stops_as_one(check):
    n = _ref_iters("R1", False, False, None, U.TOLS["abc"])[0]
    assert n == 7
    out = _until("R1", False, "device", 1e-2, sel=[0, 0, 0, 0], check=check)
    assert out[5].tolist() == [n] * 4
    _assert_trials(out, "R1", False, [0, 0, 0, 0])


# ---- R2: Gram order 72, the global-memory Jacobi (the header says why no bits) ------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("name,shared_B,use_indx,refresh", R2_CONFIGS)
def test_above_order_64_iters_of_the_reference_and_values_to_rounding(name, shared_B, use_indx, refresh, mem):
    tols = U.TOLS["abc"]
    ref = U.reference(name, shared_B, use_indx, refresh, tols)
    for check in (1, 64):
        out = _until(name, shared_B, mem, tols, use_indx=use_indx, refresh=refresh, check=check)
        assert out[5].tolist() == [got[5] for got in ref]
        for t, got in enumerate(ref):
            tag = "until64.%s.%s" % (name, "plain" if refresh is None else "%d_%d" % refresh)
            check_below(tag + ".S", rel_err(out[0][t], got[0]), TOL64_S)
            check_below(tag + ".Y", rel_err(out[1][t], got[1]), TOL64_S)
            assert np.isnan(out[2][t, got[5]:]).all() and np.isfinite(out[2][t, 1:got[5]]).all()


# ---- 8: refusals ------------------------------------------------------------------------------------------------------------------------
def _raw(tol, min_iters, check, iters_out, period=-1, it0=0):
    from jstsp19_amd import solvers as SV
    arrs, _, prm = _args("R1", False, "host")
    N, M, Gr, G2 = P.SHAPES["R1"]
    a = [SV._Arg(x, np.float64 if k == 1 else np.complex128, "arg") for k, x in enumerate(arrs)]
    c = SV._ctx_for(a, None)[0]
    sc = [SV._scalars(v, P.BATCH, "s")[1] for v in prm]
    outs = [SV._out(False, P.BATCH, r, cc, np.complex128) for r, cc in ((Gr, G2), (N, M))]
    ptol = None if tol is None else SV._scalars(tol, P.BATCH, "tol")[1]
    ptr = lambda s: None if s is None else s.ctypes.data
    return c._lib.jstsp_proposed_until_f64(c.handle, N, M, Gr, G2, P.BATCH, a[0].ptr, a[1].ptr, a[2].ptr, 0, a[3].ptr, G2 * M, 2, *sc,
                                           None, 0, 0, period, ptol, min_iters, check, outs[0][0], outs[1][0], None, it0, None, None, None,
                                           ptr(iters_out), None, 0)


def test_refusals():
    import jstsp19_amd as J
    last = lambda: J.load().jstsp_last_error().decode()
    it = np.full(P.BATCH, -7, np.int32)
    prefix = "proposed_algorithm until (float64): "
    assert _raw(1e-3, 0, 4, it) == E_ARG and last().startswith(prefix) and "min_iters = 0" in last()
    assert _raw(1e-3, 2, 0, it) == E_ARG and "check = 0" in last()
    assert _raw(1e-3, 2, 4, None) == E_NULL and last().startswith(prefix)
    assert _raw(None, 2, 4, it) == E_NULL
    assert _raw(1e-3, 2, 4, it, it0=3) == E_ARG and "without state_in" in last()                # the siblings' refusals
    assert np.all(it == -7)                                     # nothing was written
    assert _raw(1e-3, 2, 4, it) == 0 and it.tolist() == [2, 2, 2]                               # Imax = 2: and the context goes on
    arrs, ix, prm = _args("R1", False, "host")
    for kw in (dict(min_iters=0), dict(check=0), dict(type="std"), dict(refresh=(-1, 1)), dict(refresh=(0, -1)), dict(it0=3),
               dict(tol=(1e-3, 1e-3)), dict(indx_S=ix[:, :0])):
        with pytest.raises(ValueError):
            J.proposed_algorithm_until_f64(*arrs, 4, *prm, **{"tol": 1e-3, **kw})
    with pytest.raises(TypeError):                              # tol is required
        J.proposed_algorithm_until_f64(*arrs, 4, *prm)
