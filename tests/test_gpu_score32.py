"""The fp32 scorers jstsp_nmse_spectral_c32 / jstsp_rate_c32 (csrc/api_misc.hip) on every Gram and eigen-solver route behind them,
against score64_problems' float64 reference evaluated on the complex64 operand values the device sees
(tests/score32_problems.py: shapes, route labels, generators).

Error measure: P.rel, |x - ref| / max(|ref|, tiny) per trial, for the NMSE and for the rate; on the block route (n > 128)
|x - ref| / max(1, ref), the form of the bound the project already asserts there.  One condition was fixed before anything was
measured: for the routes with n <= 128 every bound <= 2e-5 relative (the rtol the project already asserts for these two entries),
for the block route every bound <= the existing 2e-6 * max(1, nmse) absolute.  The asserts are about 5 x the largest value measured
on MI355X over this file (profiles/score32_measured_tolerances.json), per lambda_max route and per metric, and never above the cap:

    NMSE_TOL["h32"]    score32_h32_nmse_rel     measured 3.98e-07
    NMSE_TOL["h64"]    score32_h64_nmse_rel     measured 3.48e-07
    NMSE_TOL["h128"]   score32_h128_nmse_rel    measured 3.33e-07
    NMSE_TOL["block"]  score32_block_nmse_rel   measured 9.12e-08
    RATE_TOL["h32"]    score32_h32_rate_rel     measured 3.50e-07
    RATE_TOL["h64"]    score32_h64_rate_rel     measured 3.54e-06 (33 x 4097, 16 partials, rank-4 Zbar)
    RATE_TOL["h128"]   score32_h128_rate_rel    measured 1.72e-06

Two routes exceeded their caps when first measured, on the parent commit's library and on the bits of this one alike, and were
fixed in the library rather than in the bound: the block route on an NMSE near 1 (up to 1.05e-5 against
2e-6: lambda_max is now the double Rayleigh quotient of the leading column of the block Jacobi's basis) and the rate with a
rank-4 Zbar (2.61e-5 at 128 x 600 against 2e-5: the eigenvalues are now double Rayleigh quotients of jacobi_kernel's basis, and
small negative ones are summed instead of clamped).

The scaled operands (2^s) are held to the same names and bounds: the reference NMSE is unchanged by an exact power of two.  The
rate of scaled operands is compared with the reference's closed form (score32_problems.ref_rate_sigma): its determinant
overflows float64 at 2^40 and, for R > C, is ill-conditioned from 2^20 on.  The rank-4 Zbar is scaled by 2^-8 only: at 2^20
each of its noise-level eigenvalues (1e-6 lambda_max, of which an fp32 Gram resolves 1e-7 lambda_max n) is 1e5 times the noise
variance and carries 17 bits of rate, so no fp32 Gram route can score it (0.09 - 0.23 relative when first measured; recorded here, not a case).
The error-code test found jstsp_last_error() not naming the call for a NULL context or a bad memspace: fixed in the library."""
import numpy as np
import pytest
import torch

import score32_problems as P
from conftest import check_below

pytestmark = pytest.mark.gpu

NMSE_TOL = {"h32": 2.0e-6, "h64": 1.8e-6, "h128": 1.7e-6, "block": 4.6e-7}
RATE_TOL = {"h32": 1.8e-6, "h64": 1.8e-5, "h128": 8.7e-6}
assert all(v <= 2e-5 for v in list(NMSE_TOL.values()) + list(RATE_TOL.values())) and NMSE_TOL["block"] <= 2e-6
NV = P.NOISE_VAR
OTHER = (40, 70, 2, 2)                      # a call of another shape (another Gram order, another workspace layout) between two calls


def _dev(X):
    import jstsp19_amd as J
    return J.colmajor(torch.from_numpy(np.array(X, np.complex64)).to("cuda:0"))


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _lmax(R, C, batch=3):
    return P.route(R, C, batch)[2]


def _check_nmse(R, C, e, ref, what):
    route = _lmax(R, C)
    err = P.rel(e, ref)
    if route == "block":
        err = float(np.max(np.abs(np.asarray(e) - ref) / np.maximum(1.0, ref)))
    print("score32 %s nmse %s: %.3g (rel %.3g)" % (route, what, err, P.rel(e, ref)))
    check_below("score32_%s_nmse_rel" % route, err, NMSE_TOL[route])


def _check_rate(R, C, r, ref, what):
    route = _lmax(R, C)
    err = P.rel(r, ref)
    print("score32 %s rate %s: rel %.3g" % (route, what, err))
    check_below("score32_%s_rate_rel" % route, err, RATE_TOL[route])


def _other_call(rate):
    import jstsp19_amd as J
    So, Zo = P.operands(*OTHER)
    J.rate(So, Zo, NV) if rate else J.nmse_spectral(So, Zo)


def _one_case(R, C, batch, gen):
    import jstsp19_amd as J
    want_rate = P.has_rate(R, C)
    S, Z, e_ref, r_ref = P.case(R, C, batch, gen, want_rate)
    what = "%dx%d batch %d gen %s %s" % (R, C, batch, gen, P.route(R, C, batch))
    e = J.nmse_spectral(S, Z)
    assert e.dtype == np.float64 and e.shape == (batch,)
    _check_nmse(R, C, e, e_ref, what)
    if gen == 0:
        assert np.array_equal(e == 1.0, e_ref == 1.0), what                          # the capped trials are the reference's
    Sd, Zd = _dev(S), _dev(Z)
    ed = J.nmse_spectral(Sd, Zd)
    torch.cuda.synchronize()
    assert ed.is_cuda and ed.dtype == torch.float64 and _same(ed.cpu().numpy(), e), what      # both memspaces: the same bits
    t = batch // 2
    e1 = J.nmse_spectral(S[t], Z[t])                                                 # a 2-D operand: trial t of the batch
    assert np.ndim(e1) == 0 and _same(e1, e[t]), (what, float(e1), float(e[t]))
    if batch > 3 and not want_rate:
        return          # (block route at 300 trials: two batched block Jacobis per call; the two repeats below run at batches 1 and 3)
    assert _same(J.nmse_spectral(S, Z), e), what                                     # a repeated call
    _other_call(False)
    assert _same(J.nmse_spectral(S, Z), e), what                                     # right after another shape: no stale workspace
    if not want_rate:
        return
    r = J.rate(S, Z, NV)
    assert r.dtype == np.float64 and r.shape == (batch,)
    _check_rate(R, C, r, r_ref, what)
    rd = J.rate(Sd, Zd, NV)
    torch.cuda.synchronize()
    assert rd.is_cuda and rd.dtype == torch.float64 and _same(rd.cpu().numpy(), r), what
    r1 = J.rate(S[t], Z[t], NV)
    assert np.ndim(r1) == 0 and _same(r1, r[t]), (what, float(r1), float(r[t]))
    assert _same(J.rate(S, Z, NV), r), what
    _other_call(True)
    assert _same(J.rate(S, Z, NV), r), what
    _other_call(False)                                                               # the NMSE entry leaves another layout behind
    assert _same(J.rate(S, Z, NV), r), what


@pytest.mark.parametrize("R,C", P.SHAPES)
def test_every_route_both_orientations_batches_and_memspaces(R, C):
    failed = []                                                                      # (every case is measured, then all must have held)
    for batch in P.batches((R, C)):
        for gen in P.generators(batch):
            try:
                _one_case(R, C, batch, gen)
            except AssertionError as ex:
                failed.append((batch, gen, str(ex)[:200]))
    assert not failed, failed


def test_more_entries_than_one_pass_of_the_elementwise_grid():
    (R, C), batch = P.STRIDING
    _one_case(R, C, batch, 2)


def _c64_layout(X):
    return np.ascontiguousarray(np.swapaxes(np.asarray(X, np.complex128), 1, 2))      # [t][c][r], doubles


@pytest.mark.parametrize("R,C", P.ONE_PER_ROUTE)
def test_the_c64_entries_on_float_representable_doubles_give_the_c32_bits(R, C):
    import jstsp19_amd as J
    lib, h = J.load(), J.default_context(0).handle
    for gen in (2, 0):
        S, Z = P.operands(R, C, 3, gen)
        Sc, Zc = _c64_layout(S), _c64_layout(Z)
        out = np.full(3, -7.0)
        assert lib.jstsp_nmse_spectral_c64(h, R, C, 3, Sc.ctypes.data, Zc.ctypes.data, out.ctypes.data, J.HOST) == 0
        assert _same(out, J.nmse_spectral(S, Z)), (R, C, gen)
        Sd, Zd = (torch.from_numpy(x).to("cuda:0") for x in (Sc, Zc))
        outd = torch.full((3,), -7.0, dtype=torch.float64, device="cuda:0")
        assert lib.jstsp_nmse_spectral_c64(h, R, C, 3, Sd.data_ptr(), Zd.data_ptr(), outd.data_ptr(), J.DEVICE) == 0
        torch.cuda.synchronize()
        assert _same(outd.cpu().numpy(), out), (R, C, gen)
        if P.has_rate(R, C):
            out = np.full(3, -7.0)
            assert lib.jstsp_rate_c64(h, R, C, 3, Sc.ctypes.data, Zc.ctypes.data, NV, out.ctypes.data, J.HOST) == 0
            assert _same(out, J.rate(S, Z, NV)), (R, C, gen)
            assert lib.jstsp_rate_c64(h, R, C, 3, Sd.data_ptr(), Zd.data_ptr(), NV, outd.data_ptr(), J.DEVICE) == 0
            torch.cuda.synchronize()
            assert _same(outd.cpu().numpy(), out), (R, C, gen)


@pytest.mark.parametrize("R,C", P.ONE_PER_ROUTE)
def test_the_nmse_of_operands_scaled_by_a_power_of_two(R, C):
    """S and Zbar scaled by 2^s, s = -40, -16, 16, 40: the NMSE is a ratio and holds the bound it holds at s = 0 (the reference is
    unchanged by an exact power of two); S == Zbar at 2^0 and 2^-40 scores exactly 0."""
    import jstsp19_amd as J
    for gen in (2, 4, "lowrank"):
        S, Z, e_ref, _ = P.case(R, C, 3, gen)
        for s in P.SCALES:
            e = J.nmse_spectral(P.scaled(S, s), P.scaled(Z, s))
            _check_nmse(R, C, e, e_ref, "%dx%d gen %s scale 2^%d" % (R, C, gen, s))
    _, Z = P.operands(R, C, 3, 2)
    for s in (0, -40):
        Zs = P.scaled(Z, s)
        e = J.nmse_spectral(Zs, Zs)
        assert np.array_equal(e, np.zeros(3)) and not np.any(np.signbit(e)), (R, C, s, e)


@pytest.mark.parametrize("R,C", P.RATE_ROUTES)
def test_the_rate_of_operands_scaled_by_a_power_of_two(R, C):
    import jstsp19_amd as J
    for gen in (2, "lowrank"):
        S, Z = P.operands(R, C, 3, gen)
        for s in (P.RATE_SCALES if gen == 2 else P.RATE_SCALES[:1]):                  # (the rank-4 Zbar at 2^-8 only: see the top)
            Ss, Zs = P.scaled(S, s), P.scaled(Z, s)
            ref = P.ref_rate_sigma(Ss, Zs, NV)
            assert np.all(ref > 1e-6)
            _check_rate(R, C, J.rate(Ss, Zs, NV), ref, "%dx%d gen %s scale 2^%d" % (R, C, gen, s))


@pytest.mark.parametrize("R,C", P.ONE_PER_ROUTE)
def test_conventions_equal_tripled_zero_and_non_finite(R, C):
    """What tests/test_gpu_score64.py asserts for the float64 twin: S == Zbar is exactly 0, 3 Zbar is exactly 1 (raw 4, capped),
    0/0 is NaN, x/0 is Inf (capped to 1; no signal: rate 0), a non-finite entry makes its trial NaN and leaves its neighbours'
    bits alone."""
    import jstsp19_amd as J
    rate = P.has_rate(R, C)
    _, Z = P.operands(R, C, 3, 2)
    sig = [np.linalg.svd(Z[t], compute_uv=False) for t in range(3)]
    e = J.nmse_spectral(Z, Z)
    assert np.array_equal(e, np.zeros(3)) and not np.any(np.signbit(e)), e
    if rate:
        _check_rate(R, C, J.rate(Z, Z, NV), [P.rate_from_sigma(sig[t], R, NV, 0.0) for t in range(3)], "%dx%d S == Zbar" % (R, C))
    assert np.array_equal(J.nmse_spectral(3 * Z, Z), np.ones(3))                      # raw 4, capped: exactly 1.0
    zero = np.zeros_like(Z)
    assert np.isnan(J.nmse_spectral(zero, zero)).all()                                # 0/0, as on the host
    assert np.array_equal(J.nmse_spectral(Z, zero), np.ones(3))                       # x/0 = Inf, capped
    if rate:
        assert np.isnan(J.rate(zero, zero, NV)).all()
        assert np.array_equal(J.rate(Z, zero, NV), np.zeros(3))                       # no signal: log2 det(I) = 0
    S, Z = P.operands(R, C, 3, 2)
    clean_e = J.nmse_spectral(S, Z)
    clean_r = J.rate(S, Z, NV) if rate else None
    for bad in (np.nan, np.inf):
        for which in ("S", "Zbar"):
            Sb, Zb = S.copy(), Z.copy()
            (Sb if which == "S" else Zb)[1, R // 2, C // 2] = bad
            for dev in (False, True):
                a, b = (_dev(Sb), _dev(Zb)) if dev else (Sb, Zb)
                eb = J.nmse_spectral(a, b)
                eb = eb.cpu().numpy() if dev else eb
                assert np.isnan(eb[1]), (bad, which, dev, eb)
                assert _same(eb[[0, 2]], clean_e[[0, 2]]), (bad, which, dev)
                if rate:
                    rb = J.rate(a, b, NV)
                    rb = rb.cpu().numpy() if dev else rb
                    assert np.isnan(rb[1]), (bad, which, dev, rb)
                    assert _same(rb[[0, 2]], clean_r[[0, 2]]), (bad, which, dev)


def test_error_codes_name_the_call():
    import jstsp19_amd as J
    from jstsp19_amd import _lib
    lib, h = J.load(), J.default_context(0).handle
    Z = np.zeros((2, 4, 6), np.complex64)
    out = np.zeros(2)
    z, o = Z.ctypes.data, out.ctypes.data
    nm = lambda *a: (lib.jstsp_nmse_spectral_c32(*a), lib.jstsp_last_error())
    rt = lambda *a: (lib.jstsp_rate_c32(*a[:6], 0.1, *a[6:]), lib.jstsp_last_error())
    for fn, name in ((nm, b"nmse"), (rt, b"rate")):
        for args in ((None, 6, 4, 2, z, z, o, J.HOST), (h, 6, 4, 2, None, z, o, J.HOST), (h, 6, 4, 2, z, None, o, J.HOST),
                     (h, 6, 4, 2, z, z, None, J.HOST)):
            rc, msg = fn(*args)
            assert rc == -1 and name in msg, (name, args, rc, msg)                    # JSTSP_E_NULL
        for shape in ((6, 4, 0), (0, 4, 2), (6, -1, 2), (6, 4, -3)):
            rc, msg = fn(h, *shape, z, z, o, J.HOST)
            assert rc == -2 and name in msg, (name, shape, rc, msg)                   # JSTSP_E_SHAPE
        rc, msg = fn(h, 6, 4, 2, z, z, o, 7)
        assert rc == -4 and name in msg and b"memspace" in msg, (name, rc, msg)        # JSTSP_E_ARG
    rc, msg = nm(h, 2049, 2050, 1, z, z, o, J.HOST)                                   # (refused before an operand is read)
    assert rc == _lib.E_UNSUPPORTED and b"nmse" in msg and b"2049" in msg, (rc, msg)
    rc, msg = rt(h, 129, 130, 1, z, z, o, J.HOST)
    assert rc == _lib.E_UNSUPPORTED and b"rate" in msg and b"129" in msg, (rc, msg)
    rc, msg = rt(h, 130, 129, 1, z, z, o, J.HOST)
    assert rc == _lib.E_UNSUPPORTED and b"rate" in msg, (rc, msg)
    assert out.tolist() == [0.0, 0.0]                                                 # nothing was written
