"""jstsp_proposed_resume_f64 / jstsp_proposed_std_resume_f64 (csrc/proposed64.hip): the float64 ADMM resumed from a saved state,
on the problems of tests/resume_problems.py (Gram order 32: in-LDS Jacobi; 72: global Jacobi; batch 3, per-trial scalars, shared
and per-trial B, both memspaces; Alg. 2, Alg. 2 with indx_S, Alg. 1).

Bits: the float64 solver carries nothing between iterations but the state, so legs (1, 5), (2, 4) and (3, 1, 2) return S, Y and
the convergence_error rows of the sibling entry at Imax = 6, and a call without a state returns the sibling's bits.
Bounds (not derived from this code): from an arbitrary state S and Y within 1e-10 of max|ref| and convergence_error within 1e-8 of
tests/resume_ref.py - the bounds include/jstsp.h asserts for the float64 solver against its float64 restatement."""
import ctypes as C
import functools

import numpy as np
import pytest

import resume_problems as P
import resume_ref as R
from conftest import check_below, ce_rel, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

TOL64_S, TOL64_CE = 1e-10, 1e-8
E_ARG, E_UNSUPPORTED = -4, -3
KINDS = ("approx", "angles", "std")
CASES = [(n, sh, mem) for n in ("R1", "R2") for sh in (False, True) for mem in ("host", "device")]


def _eq(a, b):
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()


def _np(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _inputs(name, shared_B, mem):
    """(subY, Omega, A, B, indx_S) as numpy (host path) or column-major torch CUDA tensors (device path), and the scalars."""
    p = P.problem(name, shared_B)
    arrs = [p["subY"], p["Omega"], p["A"], p["B"]]
    ix = p["indx_S"]
    if mem == "device":
        import torch
        import jstsp19_amd as J
        dev = torch.device("cuda:0")
        arrs = [J.colmajor(torch.from_numpy(np.ascontiguousarray(a)).to(dev)) for a in arrs]
        ix = torch.from_numpy(ix).to(dev)
    return arrs, ix, (p["tau_Y"], p["tau_S"], p["rho"])


def _sibling(kind, name, shared_B, mem, Imax):
    import jstsp19_amd as J
    arrs, ix, prm = _inputs(name, shared_B, mem)
    if kind == "std":
        return J.proposed_algorithm_std_f64(*arrs, Imax, *prm)
    return J.proposed_algorithm_f64(*arrs, Imax, *prm, indx_S=ix if kind == "angles" else None)


def _resume(kind, name, shared_B, mem, Imax, state=None, it0=0, **kw):
    import jstsp19_amd as J
    arrs, ix, prm = _inputs(name, shared_B, mem)
    if kind == "std":
        return J.proposed_algorithm_std_resume_f64(*arrs, Imax, *prm, state=state, it0=it0, **kw)
    return J.proposed_algorithm_resume_f64(*arrs, Imax, *prm, indx_S=ix if kind == "angles" else None, state=state, it0=it0, **kw)


def _legs(kind, name, shared_B, mem, legs, it0_of=lambda done: done):
    state, done, rows = None, 0, []
    for n in legs:
        S, Y, ce, state = _resume(kind, name, shared_B, mem, n, state=state, it0=it0_of(done) if state is not None else 0)
        rows.append(_np(ce))
        done += n
    return _np(S), _np(Y), np.concatenate(rows, axis=1), _np(state)


@functools.lru_cache(maxsize=None)
def _whole(kind, name, shared_B):
    """The sibling entry at Imax = 6 on the host path, once per session: what every split must return."""
    return tuple(_np(x) for x in _sibling(kind, name, shared_B, "host", 6))


# ---- 1. bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,shared_B,mem", CASES)
def test_splits_and_the_call_without_a_state_return_the_bits_of_the_sibling(kind, name, shared_B, mem):
    whole = _whole(kind, name, shared_B)
    _eq([_np(x) for x in _sibling(kind, name, shared_B, mem, 6)], whole)           # (the memspaces agree to begin with)
    out = _resume(kind, name, shared_B, mem, 6)
    _eq([_np(x) for x in out[:3]], whole)
    N, M, Gr, G2 = P.SHAPES[name]
    assert tuple(out[3].shape) == (P.BATCH, 4 * N * M + 2 * Gr * G2)
    for legs in ((1, 5), (2, 4), (3, 1, 2)):
        S, Y, ce, state = _legs(kind, name, shared_B, mem, legs)
        _eq((S, Y, ce), whole)
        _eq((state,), (_np(out[3]),))
    # the block is [X | V1 | V2 | C | v | S], column-major
    st = _np(out[3])
    for t in range(P.BATCH):
        assert np.array_equal(R.unpack_state(st[t], N, M, Gr, G2)[5], whole[0][t])
    S, Y, ce, none = _resume(kind, name, shared_B, mem, 6, want_ce=False, return_state=False)
    assert ce is None and none is None
    _eq((_np(S), _np(Y)), whole[:2])


@pytest.mark.parametrize("name", ["R1", "R2"])
def test_it0_sets_the_mask_of_a_resumed_leg(name):
    """Negative control: the second leg of (2, 4) with it0 = 0 masks the support of S0 away (ranks 31 ... 34 need 10 + 5 i >= 35)."""
    whole = _whole("angles", name, False)
    S = _legs("angles", name, False, "host", (2, 4), it0_of=lambda done: 0)[0]
    p = P.problem(name, False)
    for t in range(P.BATCH):
        sup = p["indx_S"][t][list(P.SUPPORT_RANKS)] - 1
        assert np.all(S[t].reshape(-1, order="F")[sup] == 0) and np.any(whole[0][t].reshape(-1, order="F")[sup] != 0)
        assert not np.array_equal(S[t], whole[0][t])


# ---- 2. from an arbitrary state, against the restatement ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mid_state(kind, name, shared_B):
    """The state after 3 iterations (host path)."""
    return _np(_resume(kind, name, shared_B, "host", 3)[3])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,shared_B", [("R1", False), ("R1", True), ("R2", False)])
def test_from_the_halved_state_of_another_trial(kind, name, shared_B):
    """Trial t starts from 0.5 x the state of trial t + 1: no iterate of its own problem.  Also with v = 0 and X != 0."""
    p = P.problem(name, shared_B)
    N, M, Gr, G2 = P.SHAPES[name]
    st = 0.5 * np.roll(_mid_state(kind, name, shared_B), -1, axis=0)
    st0 = st.copy()
    st0[:, 4 * N * M:4 * N * M + Gr * G2] = 0                                       # v = 0
    for tag, s_in in (("", st), (".v0", st0)):
        keep = s_in.copy()
        S, Y, ce, s_out = _resume(kind, name, shared_B, "host", 3, state=s_in, it0=3)
        assert np.array_equal(s_in, keep)                                          # state_in is not modified
        for t in range(P.BATCH):
            m, prm, ix = P.trial(p, t)
            So, Yo, ceo, sto = R.solve(*m, 3, *prm, "std" if kind == "std" else "approximate", indx_S=ix if kind == "angles" else None,
                                       state=s_in[t], it0=3)
            check_below("resume64.%s.%s%s.S" % (name, kind, tag), rel_err(S[t], So), TOL64_S)
            check_below("resume64.%s.%s%s.Y" % (name, kind, tag), rel_err(Y[t], Yo), TOL64_S)
            check_below("resume64.%s.%s%s.state" % (name, kind, tag), rel_err(s_out[t], sto), TOL64_S)
            if kind == "std":
                check_below("resume64.%s.%s%s.ce" % (name, kind, tag), ce_rel(ce[t][:, :2], ceo[:, :2]), TOL64_CE)
                assert np.all(ce[t][:, 2] == 0)
            else:
                check_below("resume64.%s.%s%s.ce" % (name, kind, tag), ce_rel(ce[t], ceo), TOL64_CE)      # (the Inf pattern is equal)
                assert np.isinf(ce[t][0, 2]) == (tag == ".v0")                     # :51: finite with the loaded v != 0, Inf with v = 0


# ---- 3. aliasing, NaN, refusals: the C ABI itself ------------------------------------------------------------------------------------
def _raw(kind, name, shared_B, mem, Imax, it0, state_in, state_out):
    """One call of the C entry with the caller's own state pointers (the Python wrapper never aliases): (rc, S, Y, ce)."""
    import jstsp19_amd as J
    from jstsp19_amd import solvers as SV
    arrs, ix, prm = _inputs(name, shared_B, mem)
    N, M, Gr, G2 = P.SHAPES[name]
    a = [SV._Arg(x, np.float64 if k == 1 else np.complex128, "arg") for k, x in enumerate(arrs)]
    a_ix = SV._indx_arg(ix if kind == "angles" else None, P.BATCH, Gr * G2)
    c, memc, dev = SV._ctx_for(a, None)
    sc = [SV._scalars(v, P.BATCH, "s")[1] for v in prm]
    outs = [SV._out(mem == "device", P.BATCH, r, cc, dt, dev) for r, cc, dt in ((Gr, G2, np.complex128), (N, M, np.complex128), (Imax, 3, np.float64))]
    ptr = lambda s: None if s is None else (s.ctypes.data if isinstance(s, np.ndarray) else s.data_ptr())
    head = (c.handle, N, M, Gr, G2, P.BATCH, a[0].ptr, a[1].ptr, a[2].ptr, 0, a[3].ptr, 0 if shared_B else G2 * M)
    tail = (it0, ptr(state_in), ptr(state_out), memc)
    if kind == "std":
        rc = c._lib.jstsp_proposed_std_resume_f64(*head, None, None, Imax, *sc, a_ix.ptr, *[o[0] for o in outs], None, *tail)
    else:
        rc = c._lib.jstsp_proposed_resume_f64(*head, Imax, *sc, 0, a_ix.ptr, *[o[0] for o in outs], *tail)
    if mem == "device":
        import torch
        torch.cuda.synchronize()
    return (rc,) + tuple(_np(o[1](False)) for o in outs)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mem", ["host", "device"])
def test_state_out_may_be_state_in(kind, mem):
    whole = _whole(kind, "R1", False)
    st = _mid_state(kind, "R1", False).copy()
    if mem == "device":
        import torch
        st = torch.from_numpy(st).to("cuda:0")
    rc, S, Y, ce = _raw(kind, "R1", False, mem, 3, 3, st, st)
    assert rc == 0
    _eq((S, Y, ce), (whole[0], whole[1], whole[2][:, 3:]))
    _eq((_np(st),), (_np(_resume(kind, "R1", False, "host", 6)[3]),))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["R1", "R2"])
def test_a_nan_in_one_trials_state_stays_in_that_trial(kind, name):
    N, M, Gr, G2 = P.SHAPES[name]
    whole = _whole(kind, name, False)
    st = _mid_state(kind, name, False).copy()
    st[1, 5] = np.nan                                                              # X(6, 1) of trial 1
    S, Y, ce, s_out = _resume(kind, name, False, "host", 3, state=st, it0=3)
    assert not np.isfinite(Y[1]).all() and not np.isfinite(s_out[1]).all()
    for t in (0, 2):
        assert np.isfinite(S[t]).all() and np.isfinite(Y[t]).all() and np.isfinite(ce[t]).all() and np.isfinite(s_out[t]).all()
        if min(N, M) <= 64:
            _eq((S[t], Y[t], ce[t]), (whole[0][t], whole[1][t], whole[2][t][3:]))
        else:           # the global Jacobi sweeps the batch together (include/jstsp.h): the last bits may depend on the batch mates
            check_below("resume64.%s.%s.nan_mates" % (name, kind), max(rel_err(S[t], whole[0][t]), rel_err(Y[t], whole[1][t])), TOL64_S)


def test_refusals():
    import jstsp19_amd as J
    st = _mid_state("approx", "R1", False)
    for kind in ("approx", "std"):
        assert _raw(kind, "R1", False, "host", 2, -1, st, None)[0] == E_ARG                     # it0 < 0
        assert "it0" in J.load().jstsp_last_error().decode()
        assert _raw(kind, "R1", False, "host", 2, 2 ** 31 - 2, st, None)[0] == E_ARG            # it0 + Imax beyond int
        assert _raw(kind, "R1", False, "host", 2, 3, None, None)[0] == E_ARG                    # from zero, it0 != 0
        assert _raw(kind, "R1", False, "host", 2, 2 ** 31 - 3, st, None)[0] == 0                # the last it0 that fits
    # a bad call names the entry that was called, and the 'std' refusal of each Alg. 2 entry points to its own way out
    last = lambda: J.load().jstsp_last_error().decode()
    for kind, nmf in (("approx", "proposed_algorithm resume (float64)"), ("std", "proposed_algorithm 'std' resume (float64)")):
        assert _raw(kind, "R1", False, "host", 2, -1, st, None)[0] == E_ARG
        assert last().startswith(nmf + ": it0 = -1")
    from jstsp19_amd import solvers as SV
    N, M, Gr, G2 = P.SHAPES["R1"]
    arrs, _, prm = _inputs("R1", False, "host")
    a = [SV._Arg(x, np.float64 if k == 1 else np.complex128, "arg") for k, x in enumerate(arrs)]
    c = SV._ctx_for(a, None)[0]
    sc = [SV._scalars(v, P.BATCH, "s")[1] for v in prm]
    outs = [SV._out(False, P.BATCH, r, cc, np.complex128) for r, cc in ((Gr, G2), (N, M))]
    args = (c.handle, N, M, Gr, G2, P.BATCH, a[0].ptr, a[1].ptr, a[2].ptr, 0, a[3].ptr, G2 * M, 2, *sc, 1, None, outs[0][0], outs[1][0],
            None)                                                                           # type = 1: 'std'; then memspace 0: host
    assert c._lib.jstsp_proposed_algorithm_f64(*args, 0) == E_UNSUPPORTED
    assert last().startswith("proposed_algorithm (float64): 'std' has no float64 path") and last().endswith(": use jstsp_proposed_algorithm_c64")
    assert c._lib.jstsp_proposed_resume_f64(*args, 0, None, None, 0) == E_UNSUPPORTED
    assert last().startswith("proposed_algorithm resume (float64): 'std' has no float64 path")
    assert last().endswith(": use jstsp_proposed_std_resume_f64")


# ---- 4. the sweep that paid for its iterations twice ------------------------------------------------------------------------------
def test_the_resumed_sweep_returns_the_bits_of_the_default():
    import torch
    from jstsp19_amd import montecarlo as MC
    from jstsp19_amd.system_model import TrainingParams
    base = TrainingParams(Nt=4, Nr=32, L=4, T=140, ratio=0.75)
    assert base.solver_shape == P.SHAPES["R1"]
    snrs, nt = [0.0, 10.0], 4
    for imax in ([2, 3, 5], [5, 2, 3, 3]):                                          # (unsorted, one Imax twice: the list's order is kept)
        a = MC.run_approx_sweep(base, snrs, imax, nt, precision="f64")
        b = MC.run_approx_sweep(base, snrs, imax, nt, precision="f64", resume=True)
        assert a.shape == (len(imax), 2, 2) and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert not torch.equal(a[0], a[1])                                              # (the columns do depend on Imax)
