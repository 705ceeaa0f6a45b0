"""Scoring float64 estimates on the device (jstsp_nmse_spectral_f64 / jstsp_rate_f64, csrc/svdvals.hip) against
montecarlo._score_f64's two formulas in numpy float64 (tests/score64_problems.py) on the operand values the device saw: each of
the three routes in both orientations, batches and memspaces; S = Zbar (1 + 1e-9 eps), which no fp32 or Gram route can score;
the conventions; and the sweep runner with score="device" against score="host" on the same estimates.

Error measure: |x - ref| / max(|ref|, tiny) per trial, for the NMSE and for the rate.  One condition was fixed before anything
was measured: every bound <= 1e-10 (the project's bound for anything derived from singular values).  The
asserts are about 5 x the largest value measured on MI355X (profiles/score64_measured_tolerances.json):

    NMSE_TOL["lds"]     score64_lds_nmse_rel       measured 5.94e-15
    NMSE_TOL["qr"]      score64_qr_nmse_rel        measured 1.55e-14
    NMSE_TOL["global"]  score64_global_nmse_rel    measured 1.49e-14
    RATE_TOL["lds"]     score64_lds_rate_rel       measured 1.05e-14 (the sweep columns included)
    RATE_TOL["qr"]      score64_qr_rate_rel        measured 1.86e-14
    RATE_TOL["global"]  score64_global_rate_rel    measured 1.97e-14

The sweep comparison uses the same names and bounds: the estimates' shapes take the same routes.

Zbar == 0: the entries return what _score_f64's quotient gives - NaN for S == 0 (0/0), and x/0 = Inf capped to 1 for any other
S (numpy.linalg.norm returns 0 there, not an error); both are asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import score64_problems as P
from conftest import check_below

pytestmark = pytest.mark.gpu

NMSE_TOL = {"lds": 3.0e-14, "qr": 7.8e-14, "global": 7.5e-14}
RATE_TOL = {"lds": 5.3e-14, "qr": 9.3e-14, "global": 9.9e-14}
assert all(v <= 1e-10 for v in list(NMSE_TOL.values()) + list(RATE_TOL.values()))
NOISE_VAR = 0.1
ONE_PER_ROUTE = [(32, 16), (64, 129), (65, 65)]


def _on_device(Y):
    import jstsp19_amd as J
    return J.colmajor(torch.from_numpy(np.ascontiguousarray(Y)).to("cuda:0"))


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _check(route, S, Z, e, r, what):
    en, rn = P.rel(e, P.ref_nmse(S, Z)), P.rel(r, P.ref_rate(S, Z, NOISE_VAR))
    print("score64 %s %s: nmse rel %.3g, rate rel %.3g" % (route, what, en, rn))
    check_below("score64_%s_nmse_rel" % route, en, NMSE_TOL[route])
    check_below("score64_%s_rate_rel" % route, rn, RATE_TOL[route])


@pytest.mark.parametrize("rows,cols", P.LDS_SHAPES + P.QR_SHAPES + P.GLOBAL_SHAPES)
def test_each_route_both_orientations_batches_and_memspaces(rows, cols):
    import jstsp19_amd as J
    rng = np.random.default_rng(rows * 100003 + cols)
    route = P.route(rows, cols)
    for batch in ((1, 3, 300) if (rows, cols) in P.MANY else (3,)):
        for k in (0, 3):
            S, Z = P.pair(rng, batch, rows, cols, k)
            e, r = J.nmse_spectral_f64(S, Z), J.rate_f64(S, Z, NOISE_VAR)
            assert e.dtype == np.float64 and e.shape == (batch,) and r.dtype == np.float64 and r.shape == (batch,)
            _check(route, S, Z, e, r, "%dx%d batch %d k %d" % (rows, cols, batch, k))
            Sd, Zd = _on_device(S), _on_device(Z)
            ed, rd = J.nmse_spectral_f64(Sd, Zd), J.rate_f64(Sd, Zd, NOISE_VAR)
            torch.cuda.synchronize()
            assert ed.is_cuda and ed.dtype == torch.float64 and rd.is_cuda and rd.dtype == torch.float64
            assert _same(ed.cpu().numpy(), e) and _same(rd.cpu().numpy(), r)          # both memspaces give the same bits
            t = batch // 2                                                            # a 2-D operand; and no dependence on the batch
            e1, r1 = J.nmse_spectral_f64(S[t], Z[t]), J.rate_f64(S[t], Z[t], NOISE_VAR)
            assert np.ndim(e1) == 0 and _same(e1, e[t]) and _same(r1, r[t])
            assert _same(J.nmse_spectral_f64(S, Z), e) and _same(J.rate_f64(S, Z, NOISE_VAR), r)      # a repeated call


@pytest.mark.parametrize("rows,cols", ONE_PER_ROUTE)
def test_an_error_of_1e_minus_9_of_zbar_keeps_its_digits(rows, cols):
    """NMSE of the order 1e-18: the relative error against the reference is held to the route's bound.  What the fp32 entry
    (jstsp_nmse_spectral_c64 narrows to the Gram/Lanczos kernels) returns there is recorded, not asserted."""
    import jstsp19_amd as J
    rng = np.random.default_rng(31 + rows)
    route = P.route(rows, cols)
    S, Z = P.close_pair(rng, 3, rows, cols)
    ref = P.ref_nmse(S, Z)
    assert np.all(ref > 1e-20) and np.all(ref < 1e-15)
    e = J.nmse_spectral_f64(S, Z)
    en = P.rel(e, ref)
    print("score64 %s %dx%d close pair: ref %s, nmse rel %.3g" % (route, rows, cols, ref.tolist(), en))
    check_below("score64_%s_nmse_rel" % route, en, NMSE_TOL[route])
    lib, ctx = J.load(), J.default_context(0)
    Sc, Zc = (np.ascontiguousarray(np.swapaxes(x, 1, 2)) for x in (S, Z))
    narrow = np.empty(3)
    rc = lib.jstsp_nmse_spectral_c64(ctx.handle, rows, cols, 3, Sc.ctypes.data, Zc.ctypes.data, narrow.ctypes.data, J.HOST)
    with np.errstate(all="ignore"):
        fr = float(np.max(np.abs(narrow - ref) / ref)) if rc == 0 else float("inf")
    print("score64 %s %dx%d close pair: jstsp_nmse_spectral_c64 rc %d returns %s (recorded, not asserted): rel %.3g"
          % (route, rows, cols, rc, narrow.tolist() if rc == 0 else None, fr))
    check_below("score64_%s_close_pair_fp32_entry_rel_recorded" % route, fr if np.isfinite(fr) else 1e300, np.inf)


@pytest.mark.parametrize("rows,cols", ONE_PER_ROUTE)
def test_conventions_equal_tripled_zero_and_nan(rows, cols):
    import jstsp19_amd as J
    rng = np.random.default_rng(53 + cols)
    route = P.route(rows, cols)
    Z = P.rand(rng, 3, rows, cols) * 0.3
    sig = [np.linalg.svd(Z[t], compute_uv=False) for t in range(3)]
    e, r = J.nmse_spectral_f64(Z, Z), J.rate_f64(Z, Z, NOISE_VAR)
    assert np.array_equal(e, np.zeros(3)) and not np.any(np.signbit(e))                # S == Zbar: exactly 0.0
    check_below("score64_%s_rate_rel" % route, P.rel(r, [P.rate_from_sigma(sig[t], rows, NOISE_VAR, 0.0) for t in range(3)]), RATE_TOL[route])
    e, r = J.nmse_spectral_f64(3 * Z, Z), J.rate_f64(3 * Z, Z, NOISE_VAR)
    assert np.array_equal(e, np.ones(3))                                               # raw 4, capped: exactly 1.0
    check_below("score64_%s_rate_rel" % route, P.rel(r, [P.rate_from_sigma(sig[t], rows, NOISE_VAR, 4.0) for t in range(3)]), RATE_TOL[route])
    zero = np.zeros_like(Z)
    assert np.isnan(J.nmse_spectral_f64(zero, zero)).all() and np.isnan(J.rate_f64(zero, zero, NOISE_VAR)).all()     # 0/0, as on the host
    assert np.array_equal(J.nmse_spectral_f64(Z, zero), np.ones(3))                    # x/0 = Inf, capped, as on the host
    assert np.array_equal(J.rate_f64(Z, zero, NOISE_VAR), np.zeros(3))                 # and no signal: log2 det(I) = 0
    S = Z + 1e-3 * P.rand(rng, 3, rows, cols)
    clean_e, clean_r = J.nmse_spectral_f64(S, Z), J.rate_f64(S, Z, NOISE_VAR)
    for bad in (np.nan, np.inf):
        for which in ("S", "Zbar"):
            Sb, Zb = S.copy(), Z.copy()
            (Sb if which == "S" else Zb)[1, rows // 2, cols // 2] = bad
            for dev in (False, True):
                a, b = (_on_device(Sb), _on_device(Zb)) if dev else (Sb, Zb)
                eb, rb = J.nmse_spectral_f64(a, b), J.rate_f64(a, b, NOISE_VAR)
                if dev:
                    eb, rb = eb.cpu().numpy(), rb.cpu().numpy()
                assert np.isnan(eb[1]) and np.isnan(rb[1]), (bad, which, dev)
                assert _same(eb[[0, 2]], clean_e[[0, 2]]) and _same(rb[[0, 2]], clean_r[[0, 2]]), (bad, which, dev)


@pytest.mark.parametrize("rows,cols", ONE_PER_ROUTE)
def test_powers_of_two_the_spectrum_entry_and_a_complex64_zbar(rows, cols):
    import jstsp19_amd as J
    rng = np.random.default_rng(71 + rows)
    S, Z = P.pair(rng, 3, rows, cols, 3)
    e = J.nmse_spectral_f64(S, Z)
    for k in (40, -40):
        assert _same(J.nmse_spectral_f64(S * 2.0 ** k, Z * 2.0 ** k), e), k
    # sigma_1 inside is the spectrum entry's: min(1, (spectrum(D, 1) / spectrum(Zbar, 1))^2) with D formed in numpy complex128
    want = np.minimum(1.0, (J.spectrum(S - Z, 1)[:, 0] / J.spectrum(Z, 1)[:, 0]) ** 2)
    ulps = float(np.max(np.abs(e - want) / np.spacing(want)))
    print("score64 %dx%d: NMSE against the spectrum entry, %.1f ulp" % (rows, cols, ulps))
    check_below("score64_vs_spectrum_ulp", ulps, 4.0 + 1e-6)
    # a complex64 CUDA Zbar (what build_trials returns) is widened on the device: the bits of its widened copy
    Z32 = Z.astype(np.complex64)
    Sd, Zd32 = _on_device(S), _on_device(Z32)
    e32, r32 = J.nmse_spectral_f64(Sd, Zd32), J.rate_f64(Sd, Zd32, NOISE_VAR)
    ew, rw = J.nmse_spectral_f64(S, Z32.astype(np.complex128)), J.rate_f64(S, Z32.astype(np.complex128), NOISE_VAR)
    assert e32.dtype == torch.float64 and _same(e32.cpu().numpy(), ew) and _same(r32.cpu().numpy(), rw)


def test_error_codes():
    import jstsp19_amd as J
    from jstsp19_amd import _lib
    lib, h = J.load(), J.default_context(0).handle
    Z = np.zeros((2, 4, 6), np.complex128)
    out = np.zeros(2)
    z, o = Z.ctypes.data, out.ctypes.data
    nm, rt = lib.jstsp_nmse_spectral_f64, lib.jstsp_rate_f64
    assert nm(h, 513, 513, 1, z, z, o, J.HOST) == _lib.E_UNSUPPORTED and b"513 x 513" in lib.jstsp_last_error()
    assert rt(h, 513, 513, 1, z, z, 0.1, o, J.HOST) == _lib.E_UNSUPPORTED
    assert nm(h, 65, 9000, 1, z, z, o, J.HOST) == _lib.E_UNSUPPORTED and nm(h, 2, 70000, 1, z, z, o, J.HOST) == _lib.E_UNSUPPORTED
    for args in ((None, 6, 4, 2, z, z, o, J.HOST), (h, 6, 4, 2, None, z, o, J.HOST), (h, 6, 4, 2, z, None, o, J.HOST), (h, 6, 4, 2, z, z, None, J.HOST)):
        assert nm(*args) == -1, args                                           # JSTSP_E_NULL
        assert rt(*args[:6], 0.1, *args[6:]) == -1, args
    for shape in ((6, 4, 0), (0, 4, 2), (6, -1, 2)):
        assert nm(h, *shape, z, z, o, J.HOST) == -2 and rt(h, *shape, z, z, 0.1, o, J.HOST) == -2, shape      # JSTSP_E_SHAPE
    assert nm(h, 6, 4, 2, z, z, o, 7) == -4 and rt(h, 6, 4, 2, z, z, 0.1, o, 7) == -4                       # JSTSP_E_ARG: memspace
    assert rt(h, 6, 4, 2, z, z, -1.0, o, J.HOST) == -4 and rt(h, 6, 4, 2, z, z, float("nan"), o, J.HOST) == -4      # noise_var
    with pytest.raises(J.JstspError) as e:
        J.nmse_spectral_f64(np.zeros((513, 513), complex), np.zeros((513, 513), complex))
    assert e.value.code == _lib.E_UNSUPPORTED


F64_COLUMNS = ("ls", "omp_mmv", "tssr", "svt")


def _bits(d):
    return {k: v.double().cpu().numpy().tobytes() for k, v in d.items()}


@pytest.fixture(scope="module")
def sweep_inputs():
    from jstsp19_amd.system_model import SweepParams, build_trials
    p = SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4, snr_db=6.0)
    return build_trials(p, 0, 3, seed=616, device=torch.device("cuda", 0), with_hbf=True)


@pytest.mark.parametrize("metric", ["nmse", "rate"])
def test_the_baselines_scored_on_the_device_against_the_host(sweep_inputs, metric):
    from jstsp19_amd import montecarlo as mc
    inp = sweep_inputs
    kw = dict(metric=metric, noise_var=NOISE_VAR, tssr=(10, 0.1), ls_precision="f64", mmv_precision="f64")
    route = P.route(*inp["Zbar"].shape[1:])
    name, tol = ("score64_%s_%s_rel" % (route, metric)), (NMSE_TOL if metric == "nmse" else RATE_TOL)[route]
    before = mc._hip_baselines(inp, 100, **kw)
    dev = mc._hip_baselines(inp, 100, score="device", **kw)
    assert set(dev) == set(before) and set(F64_COLUMNS) <= set(dev)
    for k in F64_COLUMNS:
        assert dev[k].dtype == torch.float64 and not dev[k].is_cuda and dev[k].shape == (3,), (k, dev[k])
        err = P.rel(dev[k].numpy(), before[k].numpy())
        print("score64 sweep %s %s: host %s device %s rel %.3g" % (metric, k, before[k].tolist(), dev[k].tolist(), err))
        check_below(name, err, tol)
    for k in set(before) - set(F64_COLUMNS):                                  # the fp32 columns keep _score: the same bits
        assert _bits({k: dev[k]}) == _bits({k: before[k]}), k
    assert _bits(mc._hip_baselines(inp, 100, **kw)) == _bits(before)            # the default call, before and after


def test_the_approx_sweep_scored_on_the_device_against_the_host():
    from jstsp19_amd import montecarlo as mc
    from jstsp19_amd.system_model import TrainingParams
    base = TrainingParams(Nt=4, Nr=32, L=4, T=140, ratio=0.75)
    args = (base, [10.0], [10], 2)
    host = mc.run_approx_sweep(*args, precision="f64", score="host")
    dev = mc.run_approx_sweep(*args, precision="f64", score="device")
    assert dev.shape == host.shape == (1, 1, 2) and dev.dtype == torch.float64 and not dev.is_cuda
    route = P.route(*base.solver_shape[2:])
    err = P.rel(dev.numpy().ravel(), host.numpy().ravel())
    print("score64 approx sweep: host %s device %s rel %.3g" % (host.ravel().tolist(), dev.ravel().tolist(), err))
    check_below("score64_%s_nmse_rel" % route, err, NMSE_TOL[route])
    assert torch.equal(mc.run_approx_sweep(*args, precision="f64"), host)       # the default is the host scoring, on the bits
