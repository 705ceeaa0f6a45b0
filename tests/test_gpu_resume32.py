"""jstsp_proposed_resume_c32 (csrc/proposed.hip, csrc/resume.hip): the fp32 ADMM resumed from a saved state, on shapes that reach
each branch of the loop - the branch is confirmed, not assumed (jstsp_last_dictionary_block, the "fused_pass" profile count):

  a  N = 64, M = 256, Gr = 64, G2 = 128, block-Toeplitz B of block height 64     the window kernel of the fused pass
  b  the same shape with a generic B                                             the general fused pass
  c  b with JSTSP_FUSED=0                                                        no pass: the three-kernel iteration
  d  N = 32, M = 140, Gr = 32, G2 = 16                                           no pass (the shape does not take it)

(a - c under JSTSP_H2=2, see ENV below), each with and without convergence_error (the two-output call takes a different window), batch 3.

Bounds: TOL_S / TOL_CE of tests/conftest.py - the bounds of the uninterrupted fp32 solve against its float64 restatement - against
tests/resume_ref.py on the same complex64 values.  A split solve is not bit-identical to the whole one (the Jacobi basis, the Ritz
vectors and the phase of the R v refresh start cold): max|S_split - S_whole| / max|S| is recorded and held to TOL_S as well."""
import functools
import os

import numpy as np
import pytest

import resume_ref as R
from conftest import TOL_CE, TOL_S, ce_rel, check_below, rel_err
from test_mex_gateway import call, mex  # noqa: F401  (the gateway built against the MEX stand-in and the real library)

pytestmark = pytest.mark.gpu

BATCH, IMAX = 3, 6
CASES = ("a", "b", "c", "d")
# N G2 M = 2^21 of shape a - c is under the 2^22 from which the contractions go to the split-f16 pipe by default, and the fused pass
# exists on that pipe only: JSTSP_H2=2 (every contraction on it) is what makes this shape take the pass
ENV = {"a": {"JSTSP_H2": "2"}, "b": {"JSTSP_H2": "2"}, "c": {"JSTSP_H2": "2", "JSTSP_FUSED": "0"}}


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """numpy inputs (host path) of a case: dict(subY, Omega, A, B, tau_Y, tau_S, rho)."""
    from jstsp19_amd.system_model import SweepParams, build_trials
    if case == "d":
        p, shape = SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4, snr_db=5.0), (32, 140, 32, 16)
    else:
        p, shape = SweepParams(Nt=64, Nr=64, L=2, T=4, Mr=8, snr_db=5.0), (64, 256, 64, 128)
    assert p.solver_shape == shape
    inp = build_trials(p, 0, BATCH, seed=47)
    o = {k: inp[k].cpu().numpy() for k in ("subY", "Omega", "A", "B")}
    o.update(tau_Y=inp["tau_Y"].numpy(), tau_S=inp["tau_Z"].numpy(), rho=inp["rho"].numpy())
    if case in ("b", "c"):              # a generic dictionary of the same scale: no block-Toeplitz structure to find
        rng = np.random.default_rng(48)
        B = rng.standard_normal(o["B"].shape) + 1j * rng.standard_normal(o["B"].shape)
        o["B"] = (B * np.sqrt(np.mean(np.abs(o["B"]) ** 2) / 2)).astype(np.complex64)
    return o


def _call(case, Imax, want_ce=True, state=None, it0=0, env=None, sibling=False, mem="host"):
    """(S, Y, ce, state) as numpy, fallbacks, fused passes launched, dictionary block - of one call under the case's switches"""
    import jstsp19_amd as J
    o = _inputs(case)
    if mem == "device":
        import torch
        o = dict(o, **{k: J.colmajor(torch.from_numpy(np.ascontiguousarray(o[k])).to("cuda:0")) for k in ("subY", "Omega", "A", "B")})
        state = None if state is None else torch.from_numpy(np.ascontiguousarray(state)).to("cuda:0")
    env = dict(ENV.get(case, {}), **(env or {}))
    for k, v in env.items():
        os.environ[k] = v
    c = J.default_context(0)
    try:
        c.set_profiling(True)
        args = (o["subY"], o["Omega"], o["A"], o["B"], Imax, o["tau_Y"], o["tau_S"], o["rho"], "approximate")
        if sibling:
            r = J.proposed_algorithm(*args, want_ce=want_ce) + (None,)
        else:
            r = J.proposed_algorithm_resume(*args, want_ce=want_ce, state=state, it0=it0)
        passes = c.get_profile("fused_pass")[0]
        c.set_profiling(False)
        if mem == "device":
            r = tuple(None if x is None else x.cpu().numpy() for x in r)
        return r, c.last_fused_fallbacks(), passes, c.last_dictionary_block()
    finally:
        for k in env:
            os.environ.pop(k, None)


@functools.lru_cache(maxsize=None)
def _reference(case, t, Imax=IMAX):
    o = _inputs(case)
    return R.solve(o["subY"][t], o["Omega"][t], o["A"], o["B"][t], Imax, float(o["tau_Y"][t]), float(o["tau_S"][t]), float(o["rho"][t]))


def _ref_from(case, t, Imax, state, it0):
    o = _inputs(case)
    return R.solve(o["subY"][t], o["Omega"][t], o["A"], o["B"][t], Imax, float(o["tau_Y"][t]), float(o["tau_S"][t]), float(o["rho"][t]),
                   state=np.asarray(state, dtype=np.complex128), it0=it0)


def _bounds(tag, out, ref, want_ce=True):
    S, Y, ce = out
    check_below(tag + ".S", rel_err(S.astype(np.complex128), ref[0]), TOL_S)
    check_below(tag + ".Y", rel_err(Y.astype(np.complex128), ref[1]), TOL_S)
    if want_ce:
        check_below(tag + ".ce", ce_rel(ce, ref[2]), TOL_CE)


@pytest.mark.parametrize("want_ce", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_the_branch_the_call_without_a_state_and_the_splits(case, want_ce):
    (S0, Y0, c0, _), _, _, _ = _call(case, IMAX, want_ce, sibling=True)
    (S, Y, ce, st), nfb, passes, block = _call(case, IMAX, want_ce)
    # the branch this case is meant to reach
    assert nfb == 0 and (passes > 0) == (case in ("a", "b")) and block == (64 if case == "a" else 0), (passes, block)
    # without a state: the sibling's bits
    assert S.tobytes() == S0.tobytes() and Y.tobytes() == Y0.tobytes() and (not want_ce or ce.tobytes() == c0.tobytes())
    N, M = _inputs(case)["subY"].shape[1:]
    assert st.shape == (BATCH, 4 * N * M + 2 * S.shape[1] * S.shape[2]) and st.dtype == np.complex64
    for t in range(BATCH):
        _bounds("resume32.%s.whole" % case, (S[t], Y[t], ce[t] if want_ce else None), _reference(case, t), want_ce)
    for legs in ((1, 5), (3, 3)):
        state, it0, rows = None, 0, []
        for n in legs:
            (Sl, Yl, cl, state), nfb, _, _ = _call(case, n, want_ce, state=state, it0=it0)
            assert nfb == 0
            rows.append(cl)
            it0 += n
        for t in range(BATCH):
            ref = _reference(case, t)
            _bounds("resume32.%s.split" % case, (Sl[t], Yl[t], np.concatenate([r[t] for r in rows]) if want_ce else None), ref, want_ce)
            check_below("resume32.%s.state" % case, rel_err(state[t].astype(np.complex128), ref[3]), TOL_S)
            check_below("resume32.%s.split_vs_whole" % case, rel_err(Sl[t], S[t]), TOL_S)


@pytest.mark.parametrize("case", CASES)
def test_from_the_halved_state_of_another_trial_and_with_v_zero(case):
    (_, _, _, st3), _, _, _ = _call(case, 3)
    st = (0.5 * np.roll(st3, -1, axis=0)).astype(np.complex64)
    o = _inputs(case)
    nm, g = o["subY"].shape[1] * o["subY"].shape[2], o["A"].shape[1] * o["B"].shape[1]
    st0 = st.copy()
    st0[:, 4 * nm:4 * nm + g] = 0                                                    # v = 0 with X != 0
    for tag, s_in in (("", st), (".v0", st0)):
        keep = s_in.copy()
        (S, Y, ce, s_out), nfb, _, _ = _call(case, 3, state=s_in, it0=3)
        assert nfb == 0 and np.array_equal(s_in, keep)
        for t in range(BATCH):
            ref = _ref_from(case, t, 3, s_in[t], 3)
            _bounds("resume32.%s.arbitrary%s" % (case, tag), (S[t], Y[t], ce[t]), ref)
            check_below("resume32.%s.arbitrary%s.state" % (case, tag), rel_err(s_out[t].astype(np.complex128), ref[3]), TOL_S)
            assert np.isinf(ce[t][0, 2]) == (tag == ".v0")


def test_an_overflowed_trial_is_solved_again_from_its_state():
    """JSTSP_FUSED_KBACK=-20 makes every pass overflow (the value tests/test_gpu_overflow_recovery.py forces the re-solve with: the k
    scale 2^20 above what its previous maximum allows; at -1 a pass overflows only where k doubles between two iterations, which
    it does not on these trials - measured: 0 fallbacks).  The call must re-solve every trial from state_in at it0, not from zero."""
    (_, _, _, st3), _, _, _ = _call("b", 3)
    (S, Y, ce, s_out), nfb, passes, _ = _call("b", 3, state=st3, it0=3, env={"JSTSP_FUSED_KBACK": "-20"})
    assert nfb == BATCH and passes > 0
    for t in range(BATCH):
        ref = _reference("b", t)
        _bounds("resume32.b.resolve", (S[t], Y[t], ce[t]), (ref[0], ref[1], ref[2][3:]))
        check_below("resume32.b.resolve.state", rel_err(s_out[t].astype(np.complex128), ref[3]), TOL_S)


def test_device_memspace_the_mask_and_refusals():
    import torch
    import jstsp19_amd as J
    o = _inputs("d")
    dev = torch.device("cuda:0")
    cm = lambda a: J.colmajor(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    args = (cm(o["subY"]), cm(o["Omega"]), cm(o["A"]), cm(o["B"]))
    prm = (o["tau_Y"], o["tau_S"], o["rho"])
    S3, Y3, c3, st = J.proposed_algorithm_resume(*args, 3, *prm)
    S6, Y6, c6, st6 = J.proposed_algorithm_resume(*args, 3, *prm, state=st, it0=3)
    torch.cuda.synchronize()
    assert st.is_cuda and st.dtype == torch.complex64
    (Sh, Yh, ch, sth), _, _, _ = _call("d", 3)
    (Sh6, Yh6, ch6, sth6), _, _, _ = _call("d", 3, state=sth, it0=3)
    assert np.array_equal(st6.cpu().numpy(), sth6) and np.array_equal(S6.cpu().numpy(), Sh6)       # host and device memspace: the same bits
    with pytest.raises(ValueError):
        J.proposed_algorithm_resume(*args, 3, *prm, it0=2)
    with pytest.raises(ValueError):
        J.proposed_algorithm_resume(*args, 3, *prm, state=st.to(torch.complex128))
    Sa, _, _, _ = J.proposed_algorithm_angles_resume(args[0], args[1], torch.arange(1, 513, dtype=torch.int32, device=dev).repeat(BATCH, 1), args[2],
                                                     args[3], 3, *prm, state=st, it0=3)
    Sb, _, _, _ = J.proposed_algorithm_angles_resume(args[0], args[1], torch.arange(1, 513, dtype=torch.int32, device=dev).repeat(BATCH, 1), args[2],
                                                     args[3], 3, *prm, state=st, it0=0)
    torch.cuda.synchronize()
    # it0 sets the mask: 10 + 5 (it0 + 3) = 40 against 25 leading entries may be non-zero
    na, nb = (Sa.cpu().numpy().transpose(0, 2, 1).reshape(BATCH, -1) != 0), (Sb.cpu().numpy().transpose(0, 2, 1).reshape(BATCH, -1) != 0)
    assert not na[:, 40:].any() and not nb[:, 25:].any() and na[:, 25:40].any()


# ---- state_out == state_in, the _c64 form and the MEX command ------------------------------------------------------------------------
def _raw_aliased(case, mem, Imax, it0, state, env):
    """jstsp_proposed_resume_c32 with state_out == state_in (the Python wrapper never aliases): `state` is overwritten.
    Returns (S, Y, ce, fallbacks)."""
    import jstsp19_amd as J
    from jstsp19_amd import solvers as SV
    o = _inputs(case)
    arrs = [o["subY"], o["Omega"], o["A"], o["B"]]
    if mem == "device":
        import torch
        arrs = [J.colmajor(torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")) for a in arrs]
    a = [SV._Arg(x, np.float32 if k == 1 else np.complex64, "arg") for k, x in enumerate(arrs)]
    N, M, Gr, G2 = a[0].R, a[0].C, a[2].C, a[3].R
    c, memc, dev = SV._ctx_for(a, None)
    sc = [SV._scalars(o[k], BATCH, k)[1] for k in ("tau_Y", "tau_S", "rho")]
    outs = [SV._out(mem == "device", BATCH, r, cc, dt, dev) for r, cc, dt in ((Gr, G2, np.complex64), (N, M, np.complex64), (Imax, 3, np.float64))]
    ptr = state.ctypes.data if isinstance(state, np.ndarray) else state.data_ptr()
    for k, v in env.items():
        os.environ[k] = v
    try:
        rc = c._lib.jstsp_proposed_resume_c32(c.handle, N, M, Gr, G2, BATCH, a[0].ptr, a[1].ptr, a[2].ptr, 0, a[3].ptr, G2 * M, Imax, *sc, 0, None,
                                              *[x[0] for x in outs], it0, ptr, ptr, memc)
        if mem == "device":
            import torch
            torch.cuda.synchronize()
        nfb = c.last_fused_fallbacks()
    finally:
        for k in env:
            os.environ.pop(k, None)
    assert rc == 0
    return tuple(x[1](False) if mem == "host" else x[1](False).cpu().numpy() for x in outs) + (nfb,)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_state_out_may_be_state_in_also_when_every_trial_is_solved_again(mem):
    """Under JSTSP_FUSED_KBACK=-20 every trial of case b is re-solved from state_in AFTER the first solve has written state_out: with
    the two aliased, the entry must have kept a copy.  The result is the one of the call with separate arrays, bit for bit."""
    import torch
    env = dict(ENV["b"], JSTSP_FUSED_KBACK="-20")
    (_, _, _, st3), _, _, _ = _call("b", 3)
    (S, Y, ce, s_out), nfb, _, _ = _call("b", 3, state=st3, it0=3, env={"JSTSP_FUSED_KBACK": "-20"}, mem=mem)
    assert nfb == BATCH
    st = st3.copy() if mem == "host" else torch.from_numpy(st3.copy()).to("cuda:0")
    Sa, Ya, cea, nfa = _raw_aliased("b", mem, 3, 3, st, env)
    sta = st if mem == "host" else st.cpu().numpy()
    assert nfa == BATCH
    assert Sa.tobytes() == S.tobytes() and Ya.tobytes() == Y.tobytes() and cea.tobytes() == ce.tobytes() and sta.tobytes() == s_out.tobytes()
    # and without the re-solve
    (S1, Y1, c1, s1), _, _, _ = _call("b", 3, state=st3, it0=3, mem=mem)
    st = st3.copy() if mem == "host" else torch.from_numpy(st3.copy()).to("cuda:0")
    Sb, Yb, ceb, nfb2 = _raw_aliased("b", mem, 3, 3, st, ENV["b"])
    assert nfb2 == 0 and Sb.tobytes() == S1.tobytes() and (st if mem == "host" else st.cpu().numpy()).tobytes() == s1.tobytes()


def test_the_c64_form_and_the_mex_command_round_trip_on_shape_d(mex):
    """'proposed_algorithm_resume' (mex/jstsp_mex.cpp) -> jstsp_proposed_resume_c64 -> the fp32 solver, legs (3, 3) on shape d with the
    state handed from one MEX call to the next as doubles: what the fp32 entry returns on the same complex64 values, exactly (the
    narrowing of a double that holds a float is exact, and so is the widening back)."""
    m = mex
    o = _inputs("d")
    pg = lambda x: np.ascontiguousarray(np.moveaxis(x, 0, -1)).astype(np.complex128 if np.iscomplexobj(x) else np.float64)      # pages last
    subY, Om, A, B = pg(o["subY"]), pg(o["Omega"]), o["A"].astype(np.complex128), pg(o["B"])
    prm = (o["tau_Y"], o["tau_S"], o["rho"])
    S1, Y1, c1, st = call(m, 4, "proposed_algorithm_resume", subY, Om, A, B, 3, *prm, "approximate")
    N, M, Gr, G2 = 32, 140, 32, 16
    assert st.shape == (4 * N * M + 2 * Gr * G2, BATCH) and np.iscomplexobj(st)
    S2, Y2, c2, st2 = call(m, 4, "proposed_algorithm_resume", subY, Om, A, B, 3, *prm, "approximate", np.zeros((0, 0)), st, 3)
    (Sh, Yh, ch, sth), _, _, _ = _call("d", 3)
    (Sh6, Yh6, ch6, sth6), _, _, _ = _call("d", 3, state=sth, it0=3)
    assert np.array_equal(st.T, sth.astype(np.complex128)) and np.array_equal(st2.T, sth6.astype(np.complex128))
    assert np.array_equal(np.moveaxis(S2, -1, 0), Sh6.astype(np.complex128)) and np.array_equal(np.moveaxis(Y2, -1, 0), Yh6.astype(np.complex128))
    assert np.array_equal(np.moveaxis(c2, -1, 0), ch6) and np.array_equal(np.moveaxis(c1, -1, 0), ch)
    for t in range(BATCH):
        _bounds("resume32.d.mex", (S2[:, :, t], Y2[:, :, t], np.concatenate([c1[:, :, t], c2[:, :, t]])), _reference("d", t))
