"""jstsp_refit_f64 (csrc/refit64.hip): the float64 least-squares re-fit of an estimate on its support, on the problems of
tests/refit_problems.py - R1 (32, 140, 32, 16) and R2 (72, 80, 24, 20) of tests/resume_problems.py, batch 3, B per trial and shared,
both memspaces, S_in the estimate of tests/resume_ref.py after 6 iterations; K in {4, 40, g}, iters in {1, 6}, lam in {0, 0.1}; and
one 64 x 256, 64 x 128 trial at K = 4096 (g = 8192 exceeds the selection list, the products span several tiles).

Bounds (not derived from this code): S_out within TOL64_S = 1e-10 of max|ref| and resid within TOL64_CE = 1e-8 relative of
tests/refit_ref.py - the float64 family's bounds of tests/test_gpu_resume64.py - with iters_out equal.  tests/test_refit_ref.py
shows that the reference moves by at most 1.5e-15 of max|S| under a rounding-level perturbation of S_in on these problems, so the
bounds test the device arithmetic and not the problem.

Every resid entry is held to 1e-8 of ITSELF (the per-entry relative check of ce_rel), with one exception that is asserted to
occur at K = 4 only: an entry whose reference value lies below RESID_FLOOR gamma_0, RESID_FLOOR = 1e-10, is held to 1e-8 of that
floor.  Why: on K = 4 complex unknowns conjugate gradients end after 4 steps, and gamma_4 .. gamma_6 are rounding noise (1e-35 of
gamma_0 in the reference): no implementation reproduces them to 1e-8 of themselves.  r carries an absolute rounding error of some
eps |r_0|, so gamma = |r|^2 has a relative error of about 2 eps |r_0| / |r|; that stays below 1e-8 with two decades to spare down
to |r| = 1e-5 |r_0|, which is gamma = 1e-10 gamma_0.  Every test that compares resid passes K to _resid_rel, which refuses a
floored entry at any other K.

To the bit: a repeated call, a trial alone against the same trial in the batch, host against device, and indx_S =
support_order_f64(S_in) with n_indx = K against the NULL route."""
import functools

import numpy as np
import pytest

import refit_problems as Q
import refit_ref as F
import resume_problems as P
from conftest import check_below, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

TOL64_S, TOL64_CE = 1e-10, 1e-8
RESID_FLOOR = 1e-10
E_NULL, E_SHAPE, E_UNSUPPORTED, E_ARG = -1, -2, -3, -4
GRID = [(K, it, lam) for K in Q.KS for it in Q.ITERS for lam in Q.LAMS]
CASES = [(n, sh, mem) for n in Q.NAMES for sh in (False, True) for mem in ("host", "device")]


def _np(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _eq(a, b):
    for x, y in zip(a, b):
        x, y = _np(x), _np(y)
        assert x.shape == y.shape and np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()


def _dev(a):
    import torch
    import jstsp19_amd as J
    return J.colmajor(torch.from_numpy(np.array(a)).to("cuda:0"))


def _arrays(name, shared_B, mem, trials=None):
    """[subY, Omega, A, B, S_in] (numpy, or column-major CUDA tensors); trials: a slice of the batch."""
    p = P.problem(name, shared_B)
    sl = slice(None) if trials is None else trials
    B = p["B"] if shared_B else p["B"][sl]
    arrs = [p["subY"][sl], p["Omega"][sl], p["A"], B, Q.s_in(name, shared_B)[sl]]
    return [_dev(a) for a in arrs] if mem == "device" else arrs


def _call(name, shared_B, mem, K, iters, lam, tol=0.0, trials=None, indx_S=None, arrays=None):
    import jstsp19_amd as J
    arrs = arrays if arrays is not None else _arrays(name, shared_B, mem, trials)
    if indx_S is not None and mem == "device":
        import torch
        indx_S = torch.from_numpy(np.ascontiguousarray(indx_S)).to("cuda:0")
    S, n, res = J.refit_f64(*arrs, Q.k_of(name, K), iters, lam, tol, indx_S=indx_S, return_resid=True)
    return _np(S), _np(n), _np(res)


@functools.lru_cache(maxsize=None)
def _ref(name, shared_B, K, iters, lam, tol=0.0):
    out = [F.refit(*Q.trial(name, shared_B, t), Q.k_of(name, K), iters, lam, tol) for t in range(P.BATCH)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out]), np.stack([o[2] for o in out])


def _resid_rel(res, ref, K):
    """largest |res_k - ref_k| / |ref_k| over the finite entries of one trial; the NaN pattern must be equal.  Only at K = 4 may a
    reference entry lie below RESID_FLOOR gamma_0 (asserted); such an entry is held against the floor instead of itself."""
    fin = np.isfinite(ref)
    assert res.shape == ref.shape and np.array_equal(np.isfinite(res), fin)
    r, d = np.abs(ref[fin]), np.abs(res[fin] - ref[fin])
    low = r < RESID_FLOOR * ref[0]
    assert K == 4 or not low.any(), ("a resid entry of the reference is at rounding level", K, ref)
    den = np.where(low, RESID_FLOOR * ref[0], r)
    return float(np.max(d / den))


# ---- 1. against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shared_B,mem", CASES)
def test_against_the_restatement(name, shared_B, mem):
    arrs = _arrays(name, shared_B, mem)
    for K, iters, lam in GRID:
        S, n, res = _call(name, shared_B, mem, K, iters, lam, arrays=arrs)
        So, no, reso = _ref(name, shared_B, K, iters, lam)
        assert res.shape == (P.BATCH, iters + 1) and n.dtype == np.int32
        # (at K = 4, iters = 6 the steps after the fourth run on rounding-level gamma: that both sides take all six rests on neither
        #  gamma being exactly 0 and on delta staying positive there, which holds on these problems - gamma_4 .. gamma_6 are 1e-35
        #  to 1e-44 of gamma_0 on both sides - but is a property of the problems, not of the method; the step a trial freezes at
        #  is tested with a margin in test_tol_freezes_each_trial_at_the_step_of_the_restatement)
        assert np.array_equal(n, no) and np.all(no == iters)
        tag = "refit64.%s.K%s" % (name, "g" if K is None else K)
        for t in range(P.BATCH):
            print("%s it=%d lam=%g t=%d S %.3g resid %.3g" % (tag, iters, lam, t, rel_err(S[t], So[t]), _resid_rel(res[t], reso[t], K)))
            check_below(tag + ".S", rel_err(S[t], So[t]), TOL64_S)
            check_below(tag + ".resid", _resid_rel(res[t], reso[t], K), TOL64_CE)
            if K is not None:
                assert np.count_nonzero(S[t]) <= K and np.array_equal(S[t] != 0, So[t] != 0)       # exact zeros off the support


# ---- 2. bits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shared_B", [(n, sh) for n in Q.NAMES for sh in (False, True)])
def test_bits_do_not_depend_on_the_run_the_batch_the_memspace_or_the_route(name, shared_B):
    import jstsp19_amd as J
    N, M, Gr, G2 = P.SHAPES[name]
    order = _np(J.support_order_f64(Q.s_in(name, shared_B)))
    for K, iters, lam in [(K, 6, 0.1) for K in Q.KS] + [(40, 1, 0.0)]:
        k = Q.k_of(name, K)
        whole = _call(name, shared_B, "host", K, iters, lam)
        _eq(_call(name, shared_B, "host", K, iters, lam), whole)                               # a repeated call
        _eq(_call(name, shared_B, "device", K, iters, lam), whole)                             # the other memspace
        _eq(_call(name, shared_B, "device", K, iters, lam), whole)
        for t in range(P.BATCH):                                                               # a trial alone
            for mem in ("host", "device"):
                alone = _call(name, shared_B, mem, K, iters, lam, trials=slice(t, t + 1))
                _eq(alone, [w[t:t + 1] for w in whole])
        for mem in ("host", "device"):                                                         # the order handed in: n_indx = K
            _eq(_call(name, shared_B, mem, K, iters, lam, indx_S=order[:, :k]), whole)
        if K is not None:                                                                      # ... and a longer list: its first K
            _eq(_call(name, shared_B, "host", K, iters, lam, indx_S=order), whole)


def test_indx_S_is_honoured_and_out_of_range_entries_are_ignored():
    """A list that is NOT the order of S_in: the reference on the same list; entries outside 1 .. g take a place and select nothing."""
    name, K = "R1", 40
    N, M, Gr, G2 = P.SHAPES[name]
    g = Gr * G2
    rng = np.random.default_rng(11)
    ix = np.stack([rng.permutation(g)[:50] + 1 for _ in range(P.BATCH)]).astype(np.int32)
    ix[:, 3], ix[:, 7] = 0, g + 1
    S, n, res = _call(name, False, "host", K, 6, 0.0, indx_S=ix)
    for t in range(P.BATCH):
        So, no, reso = F.refit(*Q.trial(name, False, t), K, 6, indx_S=ix[t])
        assert n[t] == no and np.count_nonzero(S[t]) == K - 2
        check_below("refit64.indx.S", rel_err(S[t], So), TOL64_S)
        check_below("refit64.indx.resid", _resid_rel(res[t], reso, K), TOL64_CE)


# ---- 3. the objective --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Q.NAMES)
def test_the_objective_of_the_result_does_not_exceed_that_of_the_masked_input(name):
    for K, iters, lam in GRID:
        S, _, _ = _call(name, False, "host", K, iters, lam)
        for t in range(P.BATCH):
            subY, Om, A, B, S_in = Q.trial(name, False, t)
            start = np.where(F.support_mask(S_in, Q.k_of(name, K)) != 0, S_in, 0)
            assert F.objective(subY, Om, A, B, S[t], lam) <= F.objective(subY, Om, A, B, start, lam)


# ---- 4. edge cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
def test_the_zero_problem_takes_no_step(mem):
    arrs = _arrays("R1", False, "host")
    arrs[0], arrs[4] = np.zeros_like(arrs[0]), np.zeros_like(arrs[4])
    if mem == "device":
        arrs = [_dev(a) for a in arrs]
    for K in (40, None):
        S, n, res = _call("R1", False, mem, K, 6, 0.0, arrays=arrs)
        assert not S.any() and not n.any()
        assert np.all(res[:, 0] == 0) and np.isnan(res[:, 1:]).all()


@pytest.mark.parametrize("name", Q.NAMES)
def test_a_nan_in_one_trial_leaves_its_mates_bits_alone(name):
    clean = _call(name, False, "host", 40, 6, 0.1)
    for which in (4, 0):                                                                       # S_in, then subY
        arrs = [np.array(a) for a in _arrays(name, False, "host")]
        arrs[which][1, 2, 3] = np.nan
        S, n, res = _call(name, False, "host", 40, 6, 0.1, arrays=arrs)
        assert n[1] == 0 and np.isnan(res[1]).all() and np.isnan(S[1]).any() == (which == 4)       # (x stays m .* S_in)
        for t in (0, 2):
            _eq([S[t], n[t:t + 1], res[t]], [clean[0][t], clean[1][t:t + 1], clean[2][t]])


@pytest.mark.parametrize("mem", ["host", "device"])
def test_tol_freezes_each_trial_at_the_step_of_the_restatement(mem):
    """tol^2 = 0.012 keeps a margin of 20 % from every gamma_k / gamma_0 of every trial (10 % is asserted on the reference), so the
    step at which a trial freezes is decided, not drawn: 4, 4 and 5 steps."""
    name, K, iters, lam, tol = "R1", 40, 6, 0.0, np.sqrt(0.012)
    So, no, reso = _ref(name, False, K, iters, lam, tol)
    full = _ref(name, False, K, iters, lam)[2]
    ratio = full / full[:, :1]
    assert np.all(np.abs(ratio / tol ** 2 - 1) > 0.1) and no.tolist() == [4, 4, 5]
    S, n, res = _call(name, False, mem, K, iters, lam, tol)
    assert np.array_equal(n, no)
    for t in range(P.BATCH):
        check_below("refit64.tol.S", rel_err(S[t], So[t]), TOL64_S)
        check_below("refit64.tol.resid", _resid_rel(res[t], reso[t], K), TOL64_CE)
        assert np.isnan(res[t, n[t] + 1:]).all() and np.isfinite(res[t, :n[t] + 1]).all()
    # a frozen trial keeps the bits of the call that ran exactly its steps
    for t in range(P.BATCH):
        S1, n1, _ = _call(name, False, mem, K, int(no[t]), lam, trials=slice(t, t + 1))
        _eq([S1[0]], [S[t]])


# ---- 5. the larger shape -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
def test_the_larger_shape(mem):
    import jstsp19_amd as J
    b = Q.big()
    arrs = [b[k] for k in ("subY", "Omega", "A", "B", "S_in")]
    if mem == "device":
        arrs = [_dev(a) for a in arrs]
    S, n, res = J.refit_f64(*arrs, Q.BIG_K, Q.BIG_ITERS, return_resid=True)
    S, n, res = _np(S), _np(n), _np(res)
    So, no, reso = F.refit(b["subY"][0], b["Omega"][0], b["A"], b["B"], b["S_in"][0], Q.BIG_K, Q.BIG_ITERS)
    assert n[0] == no == Q.BIG_ITERS and np.count_nonzero(S[0]) == Q.BIG_K and np.array_equal(S[0] != 0, So != 0)
    check_below("refit64.big.S", rel_err(S[0], So), TOL64_S)
    check_below("refit64.big.resid", _resid_rel(res[0], reso, Q.BIG_K), TOL64_CE)


# ---- 6. the C ABI itself: aliasing, NULL outputs, refusals ----------------------------------------------------------------------------
def _raw(mem="host", **kw):
    """One call of the C entry on R1 (B per trial) with arguments replaced by name; returns (rc, S_out, resid, iters_out) - the
    three outputs pre-filled with a sentinel so that an untouched output shows."""
    from jstsp19_amd import solvers as SV
    N, M, Gr, G2 = P.SHAPES["R1"]
    g = Gr * G2
    arrs = _arrays("R1", False, mem)
    a = [SV._Arg(x, np.float64 if k == 1 else np.complex128, "arg") for k, x in enumerate(arrs)]
    c, memc, dev = SV._ctx_for(a, None)
    iters = kw.get("iters", 3)
    rows = max(iters, 1) + 1
    if mem == "device":
        import torch
        outs = [torch.full((P.BATCH, G2, Gr), -7.0, dtype=torch.complex128, device=dev), torch.full((P.BATCH, rows), -7.0, dtype=torch.float64, device=dev),
                torch.full((P.BATCH,), -7, dtype=torch.int32, device=dev)]
        ptr = [o.data_ptr() for o in outs]
    else:
        outs = [np.full((P.BATCH, G2, Gr), -7.0, complex), np.full((P.BATCH, rows), -7.0), np.full(P.BATCH, -7, np.int32)]
        ptr = [o.ctypes.data for o in outs]
    v = dict(ctx=c.handle, N=N, M=M, Gr=Gr, G2=G2, batch=P.BATCH, subY=a[0].ptr, Omega=a[1].ptr, A=a[2].ptr, strideA=0, B=a[3].ptr,
             strideB=G2 * M, S_in=a[4].ptr, indx_S=None, n_indx=0, K=40, iters=3, lam=0.0, tol=0.0, S_out=ptr[0], resid=ptr[1],
             iters_out=ptr[2], memspace=memc)
    keep = []
    if "indx_S" in kw and kw["indx_S"] is not None:
        ix = np.ascontiguousarray(kw["indx_S"], dtype=np.int32)
        if mem == "device":
            import torch
            ix = torch.from_numpy(ix).to(dev)
            kw["indx_S"] = ix.data_ptr()
        else:
            kw["indx_S"] = ix.ctypes.data
        keep.append(ix)
    if kw.pop("alias", False):
        v["S_out"] = v["S_in"]
    v.update(kw)
    rc = c._lib.jstsp_refit_f64(*[v[k] for k in ("ctx", "N", "M", "Gr", "G2", "batch", "subY", "Omega", "A", "strideA", "B", "strideB", "S_in", "indx_S",
                                                 "n_indx", "K", "iters", "lam", "tol", "S_out", "resid", "iters_out", "memspace")])
    if mem == "device":
        import torch
        torch.cuda.synchronize()
    return (rc, np.swapaxes(_np(outs[0]), 1, 2), _np(outs[1]), _np(outs[2]), a[4])


def test_S_out_may_be_S_in_and_the_optional_outputs_may_be_null():
    want = _call("R1", False, "host", 40, 3, 0.0)
    for mem in ("host", "device"):
        rc, S, res, n, _ = _raw(mem)
        assert rc == 0
        _eq([S, n, res], want)
        rc, S, res, n, a_S = _raw(mem, alias=True)
        assert rc == 0 and np.all(S == -7)
        _eq([_np(a_S.keep) if mem == "device" else np.swapaxes(a_S.keep, 1, 2), n, res], want)
        rc, S, res, n, _ = _raw(mem, resid=None, iters_out=None)
        assert rc == 0 and np.all(res == -7) and np.all(n == -7)
        _eq([S], want[:1])


def test_refusals_leave_the_outputs_untouched():
    import jstsp19_amd as J
    N, M, Gr, G2 = P.SHAPES["R1"]
    g = Gr * G2
    order = _np(J.support_order_f64(Q.s_in("R1", False)))
    bad = [
        (dict(K=0), E_ARG), (dict(K=g + 1), E_ARG),
        (dict(indx_S=order[:, :40], n_indx=39), E_ARG), (dict(indx_S=order, n_indx=g + 1), E_ARG), (dict(n_indx=40), E_ARG),
        (dict(iters=0), E_ARG), (dict(iters=-1), E_ARG),
        (dict(lam=-0.5), E_ARG), (dict(lam=float("nan")), E_ARG), (dict(tol=-1e-3), E_ARG), (dict(tol=float("nan")), E_ARG),
        (dict(subY=None), E_NULL), (dict(Omega=None), E_NULL), (dict(A=None), E_NULL), (dict(B=None), E_NULL), (dict(S_in=None), E_NULL),
        (dict(S_out=None), E_NULL), (dict(ctx=None), E_NULL),
        (dict(memspace=2), E_ARG), (dict(memspace=-1), E_ARG),
        (dict(N=0), E_SHAPE), (dict(batch=0), E_SHAPE), (dict(strideB=G2 * M - 1), E_SHAPE),
    ]
    for kw, code in bad:
        rc, S, res, n, _ = _raw("host", **kw)
        assert rc == code, (kw, rc, J.load().jstsp_last_error().decode())
        assert np.all(S == -7) and np.all(res == -7) and np.all(n == -7), kw
    assert J.load().jstsp_last_error().decode().startswith("refit (float64): ")
    # K above the selection list without indx_S: only a shape with g > 4096 can ask for it
    b = Q.big()
    arrs = [b[k] for k in ("subY", "Omega", "A", "B", "S_in")]
    with pytest.raises(ValueError):
        J.refit_f64(*arrs, 4097, 1)
    from jstsp19_amd import solvers as SV
    a = [SV._Arg(x, np.float64 if k == 1 else np.complex128, "arg") for k, x in enumerate(arrs)]
    c = SV._ctx_for(a, None)[0]
    Nb, Mb, Grb, G2b = Q.BIG_SHAPE
    out = np.full((1, G2b, Grb), -7.0, complex)
    head = (c.handle, Nb, Mb, Grb, G2b, 1, a[0].ptr, a[1].ptr, a[2].ptr, 0, a[3].ptr, 0, a[4].ptr)
    assert c._lib.jstsp_refit_f64(*head, None, 0, 4097, 1, 0.0, 0.0, out.ctypes.data, None, None, 0) == E_ARG
    assert np.all(out == -7)
    # ... and the same K through a list, or K = g without one, is served
    ix = np.arange(1, Grb * G2b + 1, dtype=np.int32)
    assert c._lib.jstsp_refit_f64(*head, ix.ctypes.data, Grb * G2b, 4097, 1, 0.0, 0.0, out.ctypes.data, None, None, 0) == 0
    assert np.count_nonzero(out) == 4097
    assert c._lib.jstsp_refit_f64(*head, None, 0, Grb * G2b, 1, 0.0, 0.0, out.ctypes.data, None, None, 0) == 0
    assert np.count_nonzero(out) == Grb * G2b
