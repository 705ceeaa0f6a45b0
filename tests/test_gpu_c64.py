"""The _c64 entry points of include/jstsp.h (MATLAB's own element type at the boundary): called through ctypes with
float64 numpy arrays / float64 device tensors.  Two checks each: (1) against the float64 oracle on genuinely double
inputs, to the fp32 tolerance of the path; (2) bit-for-bit against the _c32 entry point when the doubles are
float-representable (narrowing and widening are then exact, so any difference is a staging bug)."""
import ctypes as C

import numpy as np
import pytest

import jstsp19_amd
from jstsp19_amd import _lib
from conftest import rel_err, check_below, ce_rel
from capi_calls import _f, _unf, _p, _dp, _proposed  # noqa: F401

pytestmark = pytest.mark.gpu
HOST, DEVICE = 0, 1


def _problem(rng, batch, N, M, Gr, G2, dtype):
    A = (rng.standard_normal((N, Gr)) + 1j * rng.standard_normal((N, Gr))) / np.sqrt(2 * N)
    B = (rng.standard_normal((batch, G2, M)) + 1j * rng.standard_normal((batch, G2, M))) / np.sqrt(2 * G2)
    Om = (rng.random((batch, N, M)) < 0.4).astype(np.float64)
    S0 = np.zeros((batch, Gr, G2), complex)
    for t in range(batch):
        ix = rng.choice(Gr * G2, 6, replace=False)
        S0[t].flat[ix] = rng.standard_normal(6) + 1j * rng.standard_normal(6)
    Y = np.einsum("ng,tgh,thm->tnm", A, S0, B) + 0.05 * (rng.standard_normal((batch, N, M)) + 1j * rng.standard_normal((batch, N, M)))
    subY = Om * Y
    if dtype == np.complex64:     # float-representable doubles
        A, B, subY = (x.astype(np.complex64).astype(complex) for x in (A, B, subY))
    return A, B, Om, subY


@pytest.mark.parametrize("type_", [0, 1])
def test_proposed_algorithm_c64(type_):
    from oracle import solvers as O
    lib, ctx = jstsp19_amd.load(), jstsp19_amd.Context(0)
    rng = np.random.default_rng(31 + type_)
    batch, N, M, Gr, G2, Imax = 3, 16, 48, 16, 24, 20
    A, B, Om, subY = _problem(rng, batch, N, M, Gr, G2, np.complex128)
    S, Y, ce = _proposed(lib, ctx, "c64", A, B, Om, subY, Imax, 0.02, 0.01, 0.4, type_)
    assert S.dtype == np.complex128 and ce.dtype == np.float64
    for t in range(batch):
        So, Yo, ceo = O.proposed_algorithm(subY[t], Om[t], A, B[t], Imax, 0.02, 0.01, 0.4, "approximate" if type_ == 0 else "std")
        check_below("c64.%d.S" % type_, rel_err(S[t], So), 2e-5)                 # (measured 3.0e-6)
        check_below("c64.%d.Y" % type_, rel_err(Y[t], Yo), 2e-5)
        check_below("c64.%d.ce12" % type_, ce_rel(ce[t][1:, :2], ceo[1:, :2]), 1e-4)  # (measured 1.4e-5)
        np.testing.assert_allclose(ce[t][1:], ceo[1:], rtol=3e-3)
    # float-representable inputs: identical to the _c32 entry point, bit for bit
    A, B, Om, subY = _problem(rng, batch, N, M, Gr, G2, np.complex64)
    indx = np.stack([rng.permutation(Gr * G2) + 1 for _ in range(batch)]).astype(np.int32)
    for ix in (None, indx):
        S64, Y64, ce64 = _proposed(lib, ctx, "c64", A, B, Om, subY, Imax, 0.02, 0.01, 0.4, type_, ix)
        S32, Y32, ce32 = _proposed(lib, ctx, "c32", A, B, Om, subY, Imax, 0.02, 0.01, 0.4, type_, ix)
        assert np.array_equal(S64, S32.astype(complex)) and np.array_equal(Y64, Y32.astype(complex))
        assert np.array_equal(ce64, ce32, equal_nan=True)
    # outputs that are not wanted
    S64b, _, _ = _proposed(lib, ctx, "c64", A, B, Om, subY, Imax, 0.02, 0.01, 0.4, type_, indx, want_ce=False)
    assert np.array_equal(S64b, S64)


def test_kernel_level_and_svt_c64():
    from oracle import solvers as O
    lib, ctx = jstsp19_amd.load(), jstsp19_amd.Context(0)
    rng = np.random.default_rng(5)
    batch, N, M, Gr, G2 = 4, 12, 40, 10, 18
    A, B, _, K = _problem(rng, batch, N, M, Gr, G2, np.complex128)
    a, b, k = _f(A), _f(B), _f(K)
    out = np.empty(batch * Gr * G2, complex)
    _lib.check(lib.jstsp_correlate_c64(ctx.handle, N, M, Gr, G2, batch, _p(k), _p(a), 0, _p(b), G2 * M, _p(out), HOST))
    ref = np.einsum("ng,tnm,thm->tgh", A.conj(), K, B.conj())
    assert rel_err(_unf(out, (batch, Gr, G2)), ref) < 2e-6
    S = rng.standard_normal((batch, Gr, G2)) + 1j * rng.standard_normal((batch, Gr, G2))
    out2 = np.empty(batch * N * M, complex)
    _lib.check(lib.jstsp_synthesize_c64(ctx.handle, N, M, Gr, G2, batch, _p(_f(S)), _p(a), 0, _p(b), G2 * M, _p(out2), HOST))
    assert rel_err(_unf(out2, (batch, N, M)), np.einsum("ng,tgh,thm->tnm", A, S, B)) < 2e-6
    tau = np.full(batch, 0.3)
    X = np.empty(batch * N * M, complex)
    _lib.check(lib.jstsp_svt_c64(ctx.handle, N, M, batch, _p(k), _dp(tau), _p(X), HOST))
    X = _unf(X, (batch, N, M))
    for t in range(batch):
        assert rel_err(X[t], O.svt(K[t], 0.3)) < 2e-5
    # NULL / shape errors come back as codes, not crashes
    assert lib.jstsp_svt_c64(ctx.handle, N, M, batch, None, _dp(tau), _p(X), HOST) == -1
    assert lib.jstsp_svt_c64(ctx.handle, 0, M, batch, _p(k), _dp(tau), _p(X), HOST) == -2
    assert lib.jstsp_svt_c64(ctx.handle, N, M, batch, _p(k), _dp(tau), _p(X), 7) == -4


def test_benchmark_algorithms_c64():
    from oracle import solvers as O
    lib, ctx = jstsp19_amd.load(), jstsp19_amd.Context(0)
    rng = np.random.default_rng(9)
    # OMP.m
    meas, size_d, batch, m = 24, 40, 3, 5
    Ad = (rng.standard_normal((meas, size_d)) + 1j * rng.standard_normal((meas, size_d))) / np.sqrt(2 * meas)
    x0 = np.zeros((batch, size_d), complex)
    for t in range(batch):
        x0[t, rng.choice(size_d, m, replace=False)] = rng.standard_normal(m) + 1j * rng.standard_normal(m)
    v = x0 @ Ad.T + 0.01 * rng.standard_normal((batch, meas))
    xh = np.empty(batch * size_d, complex)
    idx = np.empty(batch * m, np.int32)
    tgt = np.empty(batch * meas * m, complex)
    _lib.check(lib.jstsp_omp_c64(ctx.handle, meas, size_d, batch, _p(_f(Ad)), 0, _p(np.ascontiguousarray(v)), m, _p(xh), _p(idx),
                                 _p(tgt), HOST))
    for t in range(batch):
        xo, io, _, To = O.omp_literal(Ad, v[t], m)
        assert np.array_equal(idx.reshape(batch, m)[t], io)
        assert rel_err(xh.reshape(batch, size_d)[t], xo) < 1e-4
        assert rel_err(_unf(tgt, (batch, meas, m))[t], To) < 1e-6
    # mc_svt.m, mc_admm.m, sparse_admm.m
    Mr = Mt = 16
    H = (rng.standard_normal((batch, Mr, 3)) + 1j * rng.standard_normal((batch, Mr, 3))) @ \
        (rng.standard_normal((batch, 3, Mt)) + 1j * rng.standard_normal((batch, 3, Mt)))
    Om = (rng.random((batch, Mr, Mt)) < 0.6).astype(float)
    OH = Om * H
    tau, rho = np.full(batch, 0.5), np.full(batch, 0.3)
    X = np.empty(batch * Mr * Mt, complex)
    _lib.check(lib.jstsp_mc_svt_c64(ctx.handle, Mr, Mt, batch, _p(_f(OH)), _p(_f(Om)), 15, _dp(tau), _dp(rho), _p(X), HOST))
    for t in range(batch):
        assert rel_err(_unf(X, (batch, Mr, Mt))[t], O.mc_svt(OH[t], Om[t], 15, 0.5, 0.3)) < 1e-4
    ce = np.empty(batch * 15)
    _lib.check(lib.jstsp_mc_admm_c64(ctx.handle, Mr, Mt, batch, _p(_f(H)), _p(_f(OH)), _p(_f(Om)), 15, _dp(tau), _dp(rho), _p(X),
                                     _p(ce), HOST))
    for t in range(batch):
        Xo, ceo = O.mc_admm(H[t], OH[t], Om[t], 15, 0.5, 0.3)
        assert rel_err(_unf(X, (batch, Mr, Mt))[t], Xo) < 1e-4
        np.testing.assert_allclose(ce.reshape(batch, 15)[t], np.ravel(ceo), rtol=2e-3)
    F = np.fft.fft(np.eye(Mr)) / np.sqrt(Mr)
    S = np.empty(batch * Mr * Mt, complex)
    _lib.check(lib.jstsp_sparse_admm_c64(ctx.handle, Mr, Mt, Mr, Mt, batch, _p(_f(H)), _p(_f(OH)), _p(_f(F)), _p(_f(F)), 12, _p(S),
                                         _p(ce[:batch * 12]), HOST))
    for t in range(batch):
        So, ceo = O.sparse_admm(H[t], OH[t], F, F, 12)
        assert rel_err(_unf(S, (batch, Mr, Mt))[t], So) < 2e-4
    # vamp.m
    Mv, Nv = 24, 48
    Av = (rng.standard_normal((Mv, Nv)) + 1j * rng.standard_normal((Mv, Nv))) / np.sqrt(2 * Mv)
    xs = np.zeros((batch, Nv), complex)
    for t in range(batch):
        xs[t, rng.choice(Nv, 4, replace=False)] = 3 * (rng.standard_normal(4) + 1j * rng.standard_normal(4))
    yv = xs @ Av.T + 0.05 * (rng.standard_normal((batch, Mv)) + 1j * rng.standard_normal((batch, Mv)))
    from oracle import vamp as V
    xo = np.empty(batch * Nv, complex)
    _lib.check(lib.jstsp_vamp_c64(ctx.handle, Mv, Nv, batch, _p(np.ascontiguousarray(yv)), _p(_f(Av)), 0, 1.0, 4.0, 5, _p(xo), HOST))
    for t in range(batch):
        assert rel_err(xo.reshape(batch, Nv)[t], V.vamp_literal(yv[t], Av, 1.0, 4.0, nit=5)) < 1e-10      # (float64 on the device since round 6)
    # the reference's operating point, nit = 100: the _c64 entry computes in float64 (csrc/vamp64.hip) and follows the literal
    # float64 restatement per trial; the _c32 entry on the same (float-representable) inputs agrees statistically only
    _lib.check(lib.jstsp_vamp_c64(ctx.handle, Mv, Nv, batch, _p(np.ascontiguousarray(yv)), _p(_f(Av)), 0, 1.0, 4.0, 100, _p(xo), HOST))
    for t in range(batch):
        assert rel_err(xo.reshape(batch, Nv)[t], V.vamp_literal(yv[t], Av, 1.0, 4.0, nit=100)) < 1e-8      # (this small system is not chaotic)


def test_c64_device_memory_stays_asynchronous_and_matches_host():
    import torch
    lib, ctx = jstsp19_amd.load(), jstsp19_amd.Context(0)
    rng = np.random.default_rng(77)
    batch, N, M, Gr, G2, Imax = 2, 16, 48, 16, 24, 10
    A, B, Om, subY = _problem(rng, batch, N, M, Gr, G2, np.complex128)
    S_h, Y_h, ce_h = _proposed(lib, ctx, "c64", A, B, Om, subY, Imax, 0.02, 0.01, 0.4, 0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    _lib.check(lib.jstsp_set_stream(ctx.handle, C.c_void_p(stream.cuda_stream)))
    with torch.cuda.stream(stream):
        t = lambda a: torch.from_numpy(_f(a)).to(dev)
        a, b, om, sy = t(A), t(B), t(Om), t(subY)
        S = torch.empty(batch * Gr * G2, dtype=torch.complex128, device=dev)
        Y = torch.empty(batch * N * M, dtype=torch.complex128, device=dev)
        ce = torch.empty(batch * 3 * Imax, dtype=torch.float64, device=dev)
        ty, ts, rh = (np.full(batch, v) for v in (0.02, 0.01, 0.4))
        _lib.check(lib.jstsp_proposed_algorithm_c64(ctx.handle, N, M, Gr, G2, batch, sy.data_ptr(), om.data_ptr(), a.data_ptr(), 0,
                                                    b.data_ptr(), G2 * M, Imax, _dp(ty), _dp(ts), _dp(rh), 0, None, S.data_ptr(),
                                                    Y.data_ptr(), ce.data_ptr(), DEVICE))
    stream.synchronize()
    _lib.check(lib.jstsp_use_own_stream(ctx.handle))
    assert np.array_equal(_unf(S.cpu().numpy(), (batch, Gr, G2)), S_h)
    assert np.array_equal(_unf(Y.cpu().numpy(), (batch, N, M)), Y_h)
    assert np.array_equal(np.transpose(ce.cpu().numpy().reshape(batch, 3, Imax), (0, 2, 1)), ce_h, equal_nan=True)


# ------------------------------------------------------------------------------------------------ the baselines' _c64 entries
def _entry(name, suffix, mem, ins, outs, args):
    """one call of jstsp_<name>_<suffix>: ``ins`` flat complex128 arrays in the C ABI's layout (narrowed to complex64 for
    _c32), ``outs`` a list of (elements, 'c' complex | 'd' double | 'i' int32), ``args(in_ptrs, out_ptrs)`` the argument
    list between ctx and memspace.  Returns the outputs as numpy arrays (complex outputs as complex128)."""
    lib, ctx = jstsp19_amd.load(), jstsp19_amd.default_context(0)
    cdt = np.complex128 if suffix == "c64" else np.complex64
    odt = {"c": cdt, "d": np.float64, "i": np.int32}
    ins = [np.ascontiguousarray(a, cdt) for a in ins]
    fn = getattr(lib, "jstsp_%s_%s" % (name, suffix))
    if mem == DEVICE:
        import torch
        ctx.use_torch_stream()
        dev = torch.device("cuda:0")
        tin = [torch.from_numpy(a).to(dev) for a in ins]
        tout = [torch.from_numpy(np.full(n, -7, odt[k])).to(dev) for n, k in outs]
        _lib.check(fn(ctx.handle, *args([t.data_ptr() for t in tin], [t.data_ptr() for t in tout]), DEVICE), name)
        torch.cuda.synchronize()
        res = [t.cpu().numpy() for t in tout]
    else:
        res = [np.full(n, -7, odt[k]) for n, k in outs]
        _lib.check(fn(ctx.handle, *args([_p(a) for a in ins], [_p(a) for a in res]), HOST), name)
    return [r.astype(np.complex128) if k == "c" else r for r, (n, k) in zip(res, outs)]


def _both_widths(name, ins, outs, args):
    """float-representable doubles: the _c64 entry returns the bits of the _c32 entry (widened), from host and from device
    memory.  Returns the outputs."""
    ins = [np.asarray(a).astype(np.complex64).astype(np.complex128) for a in ins]
    ref = _entry(name, "c32", HOST, ins, outs, args)
    for suffix, mem in (("c64", HOST), ("c64", DEVICE), ("c32", DEVICE)):
        got = _entry(name, suffix, mem, ins, outs, args)
        for r, g in zip(ref, got):
            assert r.dtype == g.dtype and r.tobytes() == g.tobytes(), (name, suffix, mem)
    return ref


def _cn(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def test_mmv_omp_c64():
    """jstsp_mmv_omp_c64 on the decisive engineered problems of tests/mmv_problems.py (per-problem dictionaries, both row
    scores): the _c32 bits on those complex64 values, and the float64 reference on doubles that are not float-representable
    (the values plus a relative 1e-9: the narrowing returns the engineered problem, whose selections are decisive)."""
    import mmv_problems as P
    pr = P.problems()
    rows = [P.by_name(n) for n in pr["own"]]
    N, Gr = rows[0]["A"].shape
    S, K, b = rows[0]["Y"].shape[1], rows[0]["K"], len(rows)
    a = np.concatenate([r["A"].T.reshape(-1) for r in rows]).astype(np.complex128)
    y = np.concatenate([r["Y"].T.reshape(-1) for r in rows]).astype(np.complex128)
    outs = [(b * Gr * S, "c"), (b * K, "i"), (b, "i")]
    for norm, pnorm in (("l2", 2), ("l1", 1)):
        args = lambda i, o: (N, Gr, S, b, i[0], N * Gr, i[1], K, pnorm, o[0], o[1], o[2])
        z32, ix32, cn32 = _both_widths("mmv_omp", [a, y], outs, args)
        for mem in (HOST, DEVICE):
            z, ix, cn = _entry("mmv_omp", "c64", mem, [a * (1 + 1e-9), y * (1 - 1e-9)], outs, args)
            assert np.array_equal(ix, ix32) and np.array_equal(cn, cn32)
            for t, r in enumerate(rows):
                ref = r["ref"][norm]
                assert cn[t] == ref["count"] and np.array_equal(ix.reshape(b, K)[t, :cn[t]], ref["sup"]), (norm, mem, t)
                check_below("c64.mmv_omp.Z", rel_err(_unf(z, (b, Gr, S))[t], ref["Z"]), 1e-4)
    # index_out / count_out are optional here as well
    z, = _entry("mmv_omp", "c64", HOST, [a, y], outs[:1], lambda i, o: (N, Gr, S, b, i[0], N * Gr, i[1], K, 2, o[0], None, None))
    assert np.array_equal(z, _entry("mmv_omp", "c64", HOST, [a, y], outs, lambda i, o: (N, Gr, S, b, i[0], N * Gr, i[1], K, 2, o[0], o[1], o[2]))[0])


def test_pinv_c64():
    """jstsp_pinv_c64: bits of _c32 on float-representable doubles (shapes of the _c32 test); against numpy's float64 pinv on
    genuine doubles at the _c32 test's 2e-6, on the rectangular shapes: narrowing the input costs eps32 * cond(A), and cond is
    below 8 there (a square Gaussian matrix has no such bound)."""
    rng = np.random.default_rng(17)
    for rows, cols in [(32, 32), (16, 140), (140, 16), (64, 64), (5, 3), (1, 7), (33, 17)]:
        A = _cn(rng, 3, rows, cols)
        outs = [(3 * rows * cols, "c")]
        args = lambda i, o: (rows, cols, 3, i[0], o[0])
        p32, = _both_widths("pinv", [_f(A).reshape(-1)], outs, args)
        A32 = A.astype(np.complex64).astype(complex)
        for t in range(3):
            assert rel_err(_unf(p32, (3, cols, rows))[t], np.linalg.pinv(A32[t])) < 2e-6, (rows, cols)
        if rows == cols:
            continue
        assert max(np.linalg.cond(A[t]) for t in range(3)) < 8
        for mem in (HOST, DEVICE):
            p, = _entry("pinv", "c64", mem, [_f(A).reshape(-1)], outs, args)
            for t in range(3):
                check_below("c64.pinv.P", rel_err(_unf(p, (3, cols, rows))[t], np.linalg.pinv(A[t])), 2e-6)


def test_rate_and_nmse_spectral_c64():
    """jstsp_rate_c64 / jstsp_nmse_spectral_c64 on the inputs of the _c32 tests (tests/test_gpu_baselines.py,
    tests/test_gpu_kernels.py), at their relative 2e-5."""
    from oracle import solvers as O
    rng = np.random.default_rng(43)
    for R, Cc in ((32, 16), (40, 12)):
        Zb = _cn(rng, 4, R, Cc)
        Sx = Zb + np.array([0.01, 0.1, 1.0, 5.0])[:, None, None] * _cn(rng, 4, R, Cc)
        ins, outs = [_f(Sx).reshape(-1), _f(Zb).reshape(-1)], [(4, "d")]
        rate_args = lambda i, o: (R, Cc, 4, i[0], i[1], 0.3, o[0])
        nmse_args = lambda i, o: (R, Cc, 4, i[0], i[1], o[0])
        _both_widths("rate", ins, outs, rate_args)
        n32, = _both_widths("nmse_spectral", ins, outs, nmse_args)
        assert n32[3] == 1.0                                                   # clipped (plot_errorVSsnr.m:139-141)
        for mem in (HOST, DEVICE):
            rate, = _entry("rate", "c64", mem, ins, outs, rate_args)
            nmse, = _entry("nmse_spectral", "c64", mem, ins, outs, nmse_args)
            for t in range(4):
                check_below("c64.rate.rel", abs(rate[t] - O.rate(Sx[t], Zb[t], 0.3)) / abs(O.rate(Sx[t], Zb[t], 0.3)), 2e-5)
                ref = O.nmse_capped(Sx[t], Zb[t])
                check_below("c64.nmse_spectral.rel", abs(nmse[t] - ref) / ref, 2e-5)


def test_ls_c64():
    """jstsp_ls_c64 = pinv(A)*Y*pinv(B) (plot_errorVSsnr.m:83), shared A and per-problem B, on both routes of B.
    Gram route (G2 = 150): the _c32 bits, and numpy's float64 pinv on the doubles of
    tests/test_gpu_baselines.py::test_ls_baseline_matches_pinv (the same generator and seed) at that test's 2.5e-5.
    Float64-pinv route (G2 = 16): the _c32 bits on Gaussian factors, and numpy's float64 pinv on genuine doubles of known
    conditioning, the cases and the bound (64 * 6e-8 * (cond A + cond B)) of
    tests/test_gpu_std_parity.py::test_ls_and_std_on_the_pinv_route_scale_with_cond.  Narrowing the doubles costs at most
    eps32 * (cond A + cond B), one unit of that bound; a square Gaussian A has no known conditioning, which is why the
    Gaussian factors of this route are compared on their bits only."""
    import std_problems as Q
    rng = np.random.default_rng(5)
    for N, M, Gr, G2, b in ((32, 200, 32, 150, 3), (32, 64, 32, 16, 3)):
        A = _cn(rng, N, Gr) / np.sqrt(N)
        B = _cn(rng, b, G2, M) / np.sqrt(M)
        Y = _cn(rng, b, N, M)
        ins, outs = [_f(Y).reshape(-1), _f(A).reshape(-1), _f(B).reshape(-1)], [(b * Gr * G2, "c")]
        args = lambda i, o: (N, M, Gr, G2, b, i[0], i[1], 0, i[2], G2 * M, o[0])
        _both_widths("ls", ins, outs, args)
        for mem in (HOST, DEVICE) if G2 == 150 else ():
            s, = _entry("ls", "c64", mem, ins, outs, args)
            for t in range(b):
                ref = np.linalg.pinv(A) @ Y[t] @ np.linalg.pinv(B[t])
                check_below("c64.ls.S", rel_err(_unf(s, (b, Gr, G2))[t], ref), 2.5e-5)
    rng = np.random.default_rng(404)
    N, M, Gr, G2 = 32, 70, 32, 16
    assert Q.route(N, M, Gr, G2) == ("pinv", "pinv")
    for cA, cB in ((10, 1e3), (1e3, 10), (1e4, 1e4), (1e2, 1e2)):
        A, B, Y = Q.factor(rng, N, Gr, cA), Q.factor(rng, G2, M, cB), _cn(rng, N, M)
        assert not np.array_equal(A, A.astype(np.complex64)) and not np.array_equal(B, B.astype(np.complex64))
        ref = np.linalg.pinv(A) @ Y @ np.linalg.pinv(B)
        ins, outs = [_f(Y[None]).reshape(-1), _f(A).reshape(-1), _f(B[None]).reshape(-1)], [(Gr * G2, "c")]
        args = lambda i, o: (N, M, Gr, G2, 1, i[0], i[1], 0, i[2], G2 * M, o[0])
        for mem in (HOST, DEVICE):
            s, = _entry("ls", "c64", mem, ins, outs, args)
            check_below("c64.ls.pinv_route.k", rel_err(_unf(s, (1, Gr, G2))[0], ref) / (6e-8 * (cA + cB)), 64)
