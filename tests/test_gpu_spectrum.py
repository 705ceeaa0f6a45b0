"""Singular values beyond the LDS limit (jstsp_spectrum_c32 / _c64 / jstsp_spectrum_trials_c32, csrc/svdvals.hip): the float64
tall-skinny QR in front of the Jacobi (n <= 64) and the global-memory Jacobi (n <= 512) against numpy.linalg.svd in float64 on
the operand values the device saw, and the sweep against the float64 SVD of the receive signal rebuilt (tests/rank_ref.py)
from jstsp_build_trials_c32's own channel and pilots, drawn or supplied.

The shapes are the smallest at which each piece can go wrong, not the workload's.  Error measure: max_k |sv_k - ref_k| / ref_1.
One condition was fixed before anything was measured: every bound <= 1e-10 (the project's bound for singular values, DESIGN.md
section 9b, which no Gram route meets).  The asserts are about 5 x the largest value measured on MI355X
(profiles/spectrum_measured_tolerances.json):

    QR_TOL       spectrum_qr_abs_over_s1        measured 2.15e-14 (64 x 1000, repeated sigma)
    GLOBAL_TOL   spectrum_global_abs_over_s1    measured 7.20e-14
    SWEEP_TOL    spectrum_sweep_abs_over_s1     measured 1.11e-14

The relative error of the values >= 1e-10 sigma_1 of the graded case is recorded (spectrum_*_graded_rel_recorded) and not
asserted: unpivoted QR promises the absolute bound only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rank_ref as R
import spectrum_problems as P
from conftest import check_below
from measured_channel_ref import cut_and_scale

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QR_TOL = 1.1e-13
GLOBAL_TOL = 3.6e-13
SWEEP_TOL = 5.5e-14
assert QR_TOL <= 1e-10 and GLOBAL_TOL <= 1e-10 and SWEEP_TOL <= 1e-10

# (rows, cols, batches)
QR_SHAPES = [(64, 129, (1, 300)), (129, 64, (3,)), (64, 4096, (3,)), (4097, 33, (3,)), (1, 8193, (3,)), (8193, 1, (3,)),
             (7, 20000, (3,)), (50, 1000, (3,))]
GLOBAL_SHAPES = [(65, 65, (1, 300)), (100, 90, (3,)), (128, 65, (3,)), (128, 128, (3,)), (96, 600, (3,)), (512, 512, (1,))]
OLD_SHAPES = [(32, 50), (64, 50), (128, 50), (50, 128), (64, 64), (128, 64), (1, 7), (7, 1), (5, 5)]


def _route(rows, cols):
    return ("spectrum_qr_abs_over_s1", QR_TOL) if min(rows, cols) <= 64 else ("spectrum_global_abs_over_s1", GLOBAL_TOL)


def _on_device(Y):
    import jstsp19_amd as J
    return J.colmajor(torch.from_numpy(np.ascontiguousarray(Y)).to("cuda:0"))


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("rows,cols,batches", QR_SHAPES + GLOBAL_SHAPES)
def test_shapes_batches_and_memspaces(rows, cols, batches, dtype):
    import jstsp19_amd as J
    rng = np.random.default_rng(rows * 100003 + cols)
    name, tol = _route(rows, cols)
    n = min(rows, cols)
    for batch in batches:
        Y = (P.rand(rng, batch, rows, cols) * 0.3).astype(dtype)
        sv = J.spectrum(Y)
        assert sv.dtype == np.float64 and sv.shape == (batch, n) and P.ordered(sv)
        e = P.err(sv, P.ref(Y))
        print("spectrum %dx%d batch %d %s: %.3g" % (rows, cols, batch, np.dtype(dtype).name, e))
        check_below(name, e, tol)
        svd = J.spectrum(_on_device(Y))
        torch.cuda.synchronize()
        assert svd.is_cuda and svd.dtype == torch.float64
        assert np.array_equal(svd.cpu().numpy(), sv)                       # both memspaces give the same bits
        one = J.spectrum(Y[batch // 2])                                    # a 2-D operand; and no dependence on the batch
        assert one.shape == (n,) and np.array_equal(one, sv[batch // 2])
        assert np.array_equal(J.spectrum(Y), sv)                           # a repeated call
        keep = max(1, n // 3)
        assert np.array_equal(J.spectrum(Y, keep), sv[:, :keep])           # n_keep < n: the leading values, on the bits


@pytest.mark.parametrize("rows,cols", [(64, 1000), (128, 600)])
def test_conditioning_rank_deficient_graded_repeated_and_zero(rows, cols):
    import jstsp19_amd as J
    rng = np.random.default_rng(77 + rows)
    name, tol = _route(rows, cols)
    for case, Y in P.conditioning_cases(rng, rows, cols):
        for dt in (np.complex128, np.complex64):
            Yd = Y.astype(dt)
            ref = P.ref(Yd)
            sv = J.spectrum(Yd)
            e = P.err(sv, ref)
            print("spectrum %dx%d %s %s: %.3g" % (rows, cols, case, np.dtype(dt).name, e))
            check_below(name, e, tol)
            assert P.ordered(sv)
            if case == "rank6" and dt is np.complex128:                    # the tail a Gram cannot give (sqrt(eps) = 1.5e-8)
                check_below(name.replace("abs_over_s1", "rank6_tail_over_s1"), float(np.max(sv[:, 6:] / sv[:, :1])), 1e-10)
            if case == "graded" and dt is np.complex128:
                keep = ref >= 1e-10 * ref[:, :1]
                rel = float(np.max(np.abs(sv - ref)[keep] / ref[keep]))
                print("spectrum %dx%d graded relative, sv_k >= 1e-10 sv_1 (recorded, not asserted): %.3g" % (rows, cols, rel))
                check_below(name.replace("abs_over_s1", "graded_rel_recorded"), rel, np.inf)
    for dt in (np.complex64, np.complex128):
        z = J.spectrum(np.zeros((3, rows, cols), dt))
        assert np.array_equal(z, np.zeros((3, min(rows, cols)))) and not np.any(np.signbit(z))       # exact zeros out


@pytest.mark.parametrize("rows,cols", [(64, 1000), (128, 600)])
def test_scale_by_powers_of_two_on_the_bits(rows, cols):
    import jstsp19_amd as J
    rng = np.random.default_rng(5)
    Y = P.usv(rng, rows, cols, rng.uniform(0.5, 2.0, 6))[None]
    base = J.spectrum(Y)
    for k in (100, -100, 400, -400):
        assert np.array_equal(J.spectrum(Y * 2.0 ** k), base * 2.0 ** k), k
    Y32 = Y.astype(np.complex64)
    base = J.spectrum(Y32)
    for k in (70, -70, 100, -100):
        Ys = (Y32 * np.float32(2.0) ** k).astype(np.complex64)
        assert np.all(np.isfinite(Ys.view(np.float32))) and np.array_equal(Ys.astype(np.complex128), Y32.astype(np.complex128) * 2.0 ** k)
        assert np.array_equal(J.spectrum(Ys), base * 2.0 ** k), k


def test_adjoint_and_permutation():
    import jstsp19_amd as J
    rng = np.random.default_rng(9)
    for rows, cols in ((64, 300), (33, 200), (100, 90)):
        name, tol = _route(rows, cols)
        Y = P.rand(rng, 3, rows, cols)
        sv = J.spectrum(Y)
        svh = J.spectrum(np.ascontiguousarray(np.conj(np.swapaxes(Y, 1, 2))))
        check_below(name.replace("abs", "adjoint_abs"), P.err(svh, sv), tol)
        check_below(name.replace("abs", "permutation_abs"), P.err(J.spectrum(Y[:, :, rng.permutation(cols)]), sv), tol)
        check_below(name.replace("abs", "permutation_abs"), P.err(J.spectrum(Y[:, rng.permutation(rows), :]), sv), tol)


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_the_old_shapes_return_the_bits_of_singular_values(dtype):
    import jstsp19_amd as J
    rng = np.random.default_rng(3)
    for rows, cols in OLD_SHAPES:
        Y = (P.rand(rng, 4, rows, cols) * 0.3).astype(dtype)
        old = J.singular_values(Y)
        assert np.array_equal(J.spectrum(Y), old), (rows, cols)
        assert np.array_equal(J.spectrum(_on_device(Y)).cpu().numpy(), old)
        keep = max(1, min(rows, cols) // 2)
        assert np.array_equal(J.spectrum(Y, keep), old[:, :keep])


@pytest.mark.parametrize("rows,cols", [(64, 300), (70, 90)])
def test_non_finite_entries_give_nan_for_their_own_matrix(rows, cols):
    import jstsp19_amd as J
    rng = np.random.default_rng(4)
    for dt in (np.complex64, np.complex128):
        Y = P.rand(rng, 6, rows, cols).astype(dt)
        clean = J.spectrum(Y)
        Y[1, 7, 2] = np.inf
        Y[3, 0, 0] = complex(np.nan, 0.0)
        Y[4, rows - 1, cols - 1] = complex(0.0, -np.inf)
        sv = J.spectrum(Y)
        assert np.all(np.isnan(sv[[1, 3, 4]]))
        assert np.array_equal(sv[[0, 2, 5]], clean[[0, 2, 5]])               # ... for that matrix only


def test_argument_errors():
    import jstsp19_amd as J
    from jstsp19_amd import _lib
    rng = np.random.default_rng(4)
    for rows, cols in ((513, 513), (65, 8193), (1, 65537)):
        with pytest.raises(J.JstspError) as e:
            J.spectrum(np.zeros((rows, cols), np.complex64))
        assert e.value.code == -3, (rows, cols)
    Y = P.rand(rng, 2, 7, 300).astype(np.complex64)
    assert isinstance(J.spectrum(Y), np.ndarray)
    assert J.spectrum(_on_device(Y)).device == torch.device("cuda:0")
    with pytest.raises(ValueError):
        J.spectrum(torch.from_numpy(Y))
    c = _lib.default_context(0)
    out = np.zeros(20)
    Yc = np.ascontiguousarray(np.swapaxes(Y, 1, 2))
    for f in (c._lib.jstsp_spectrum_c32, c._lib.jstsp_spectrum_c64):
        assert f(None, 7, 300, 2, Yc.ctypes.data, 7, out.ctypes.data, _lib.HOST) == -1
        assert f(c.handle, 7, 300, 2, None, 7, out.ctypes.data, _lib.HOST) == -1
        assert f(c.handle, 7, 300, 2, Yc.ctypes.data, 7, None, _lib.HOST) == -1
        assert f(c.handle, 0, 300, 2, Yc.ctypes.data, 7, out.ctypes.data, _lib.HOST) == -2
        assert f(c.handle, 7, 300, 0, Yc.ctypes.data, 7, out.ctypes.data, _lib.HOST) == -2
        assert f(c.handle, 7, 300, 2, Yc.ctypes.data, 8, out.ctypes.data, _lib.HOST) == -2
        assert f(c.handle, 7, 300, 2, Yc.ctypes.data, 0, out.ctypes.data, _lib.HOST) == -2
        assert f(c.handle, 513, 513, 1, Yc.ctypes.data, 1, out.ctypes.data, _lib.HOST) == -3
        assert f(c.handle, 7, 300, 2, Yc.ctypes.data, 7, out.ctypes.data, 5) == -4
    assert np.all(out == 0)


# ---------------------------------------------------------------------------------------------- the device-built sweep
def _sp(Nr, Nt, L, Tp, **kw):
    from jstsp19_amd import montecarlo as M
    return M.SweepParams(Nt=Nt, Nr=Nr, L=L, T=Tp, Mr=4, Mr_e=32, T_prop=Tp, **kw)


SWEEP_SHAPES = [(64, 4, 4, 160), (32, 4, 8, 300), (128, 4, 4, 100)]


def _rebuilt(p, trial0, batch, seed, sweep_idx, **kw):
    """Y per trial in float64 from the H and pilot symbols the trial builder returns (the fp32 values, widened)."""
    from jstsp19_amd.system_model import build_trials
    pil = {k: v for k, v in kw.items() if k in ("pilots", "shared_pilots")}
    inp = build_trials(p, trial0, batch, seed=seed, sweep_idx=sweep_idx, want_H=True, want_draws=True, **kw)
    torch.cuda.synchronize()
    ps = inp["pilot_sym"].cpu().numpy()
    if pil.get("pilots") == "gauss":
        ps = ps * np.float32(0.70710678)
    H = inp["H"].cpu().numpy().astype(complex)
    return [R.received(H[t], ps[t].astype(complex)) for t in range(batch)], inp


@pytest.mark.parametrize("Nr,Nt,L,Tp", SWEEP_SHAPES)
def test_sweep_against_float64_of_build_trials(Nr, Nt, L, Tp):
    from jstsp19_amd import _lib
    from jstsp19_amd.system_model import spectrum_trials
    p = _sp(Nr, Nt, L, Tp)
    n = min(Nr, Tp)
    sv = spectrum_trials(p, 3, 12, seed=20190913, sweep_idx=5, n_keep=n)
    torch.cuda.synchronize()
    sv = sv.cpu().numpy()
    assert sv.shape == (12, n) and P.ordered(sv) and np.all(np.isfinite(sv))
    Ys, _ = _rebuilt(p, 3, 12, 20190913, 5)
    e = P.err(sv, np.array([R.spectrum(Y) for Y in Ys]))
    print("spectrum_trials %dx%d L %d: %.3g" % (Nr, Tp, L, e))
    check_below("spectrum_sweep_abs_over_s1", e, SWEEP_TOL)
    # batch and trial offset, n_keep, the memspace: the same bits
    small = spectrum_trials(p, 8, 5, seed=20190913, sweep_idx=5, n_keep=n).cpu().numpy()
    assert np.array_equal(small, sv[5:10])
    assert np.array_equal(spectrum_trials(p, 3, 12, seed=20190913, sweep_idx=5, n_keep=7).cpu().numpy(), sv[:, :7])
    c = _lib.default_context(0)
    model = _lib.Model(p.Nt, p.Nr, p.L, p.T_prop, p.Mr, p.Mr_e, p.Gr, p.Gt, p.clusters, p.rays, 0, 0, p.noise_var,
                       _lib.BF_ZC, _lib.RHO_MIN6, 1.0, _lib.PILOTS_QAM4)
    host = np.full((5, n), -1.0)
    f = c._lib.jstsp_spectrum_trials_c32
    _lib.check(f(c.handle, C.byref(model), C.c_uint64(20190913), 5, 8, 5, None, 0, 0, 0, 0, n, host.ctypes.data, None, _lib.HOST),
               "jstsp_spectrum_trials_c32")
    assert np.array_equal(host, small)
    for bad_keep in (0, n + 1):
        assert f(c.handle, C.byref(model), C.c_uint64(1), 5, 8, 5, None, 0, 0, 0, 0, bad_keep, host.ctypes.data, None, _lib.HOST) == -2
    assert f(c.handle, C.byref(model), C.c_uint64(1), 5, 8, 5, None, 0, 0, 0, 0, n, None, None, _lib.HOST) == -1
    assert f(c.handle, C.byref(model), C.c_uint64(1), 5, 8, 5, None, 0, 0, 0, 0, n, host.ctypes.data, None, 7) == -4
    model.T_prop = 8193 if Nr > 64 else 65537
    assert f(c.handle, C.byref(model), C.c_uint64(1), 5, 8, 5, None, 0, 0, 0, 0, 1, host.ctypes.data, None, _lib.HOST) == -3


@pytest.mark.parametrize("pilots,shared", [("gauss", False), ("qam4", True)])
def test_sweep_follows_the_pilot_options_of_build_trials(pilots, shared):
    from jstsp19_amd.system_model import spectrum_trials
    for Nr, Nt, L, Tp in SWEEP_SHAPES[:1] + SWEEP_SHAPES[2:]:
        p = _sp(Nr, Nt, L, Tp)
        n = min(Nr, Tp)
        sv = spectrum_trials(p, 2, 6, seed=5, sweep_idx=6, n_keep=n, pilots=pilots, shared_pilots=shared)
        torch.cuda.synchronize()
        Ys, inp = _rebuilt(p, 2, 6, 5, 6, pilots=pilots, shared_pilots=shared)
        if shared:
            ps = inp["pilot_sym"].cpu().numpy()
            assert np.array_equal(ps[0], ps[-1])
        check_below("spectrum_sweep_abs_over_s1", P.err(sv.cpu().numpy(), np.array([R.spectrum(Y) for Y in Ys])), SWEEP_TOL)


def test_the_figure_shapes_return_the_bits_of_rank_trials():
    from jstsp19_amd import montecarlo as M
    from jstsp19_amd.system_model import rank_trials, spectrum_trials
    p = [q for q in M.rank_points(2) if q.L == 4][0]
    a = rank_trials(p, 3, 9, seed=8, sweep_idx=2)
    b = spectrum_trials(p, 3, 9, seed=8, sweep_idx=2)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(rank_trials(p, 3, 9, seed=8, sweep_idx=2, n_keep=50), spectrum_trials(p, 3, 9, seed=8, sweep_idx=2, n_keep=50))


def test_the_statement_of_the_figure_at_the_first_shape_past_the_limit():
    """Over 64 trials at 64 x 160 (Nt = 4, L = 4, 2 x 3 paths) sv_{r+1} / sv_1, r = min(Np, L*Nt, Nr, T), of the device sweep stays
    within 10 x the largest value the float64 reference gives for the same trials.  Every trial counts."""
    from jstsp19_amd.system_model import spectrum_trials
    Nr, Nt, L, Tp = SWEEP_SHAPES[0]
    p = _sp(Nr, Nt, L, Tp)
    r = R.rank_bound(p.clusters * p.rays, L, Nt=Nt, Nr=Nr, Tf=Tp)
    assert r == 6
    sv = spectrum_trials(p, 0, 64, seed=777, sweep_idx=3, n_keep=r + 1)
    torch.cuda.synchronize()
    sv = sv.cpu().numpy()
    assert sv.shape == (64, r + 1) and P.ordered(sv) and np.all(np.isfinite(sv))
    Ys, _ = _rebuilt(p, 0, 64, 777, 3)
    ref = np.array([R.spectrum(Y, r + 1) for Y in Ys])
    d, f = float(np.max(sv[:, r] / sv[:, 0])), float(np.max(ref[:, r] / ref[:, 0]))
    print("tail 64x160 r %d: device %.3g float64 %.3g" % (r, d, f))
    check_below("spectrum_tail_float64_reference", f, 1.0)
    check_below("spectrum_tail_device", d, 10.0 * f)


# ---------------------------------------------------------------------------------------------- a supplied channel
@pytest.mark.parametrize("Nr,Nt,L,Tp", SWEEP_SHAPES)
def test_the_drawn_channel_passed_back_asis_returns_the_bits(Nr, Nt, L, Tp):
    from jstsp19_amd.system_model import build_trials, spectrum_trials
    p = _sp(Nr, Nt, L, Tp)
    n = min(Nr, Tp)
    drawn = spectrum_trials(p, 2, 5, seed=31, sweep_idx=4, n_keep=n)
    H = build_trials(p, 2, 5, seed=31, sweep_idx=4, want_H=True)["H"]
    torch.cuda.synchronize()
    ch = H.cpu().numpy().reshape(5, Nr, L, Nt).transpose(0, 1, 3, 2)        # [H_1 .. H_L] -> (batch, Nr, Nt, L)
    given = spectrum_trials(p, 2, 5, seed=31, sweep_idx=4, n_keep=n, channel=ch, channel_normalize="asis")
    torch.cuda.synchronize()
    assert torch.equal(drawn, given)


@pytest.mark.parametrize("normalize", ["reference", "unit"])
def test_a_supplied_channel_against_float64_of_the_cut_and_scaled_one(normalize):
    from jstsp19_amd.system_model import build_trials, spectrum_trials
    Nr, Nt, L, Tp = SWEEP_SHAPES[1]
    p = _sp(Nr, Nt, L, Tp)
    rng = np.random.default_rng(12)
    src = (P.rand(rng, 3, 40, 6, L) * 0.7).astype(np.complex64)             # larger than the cut: ld 40 x 6 against 32 x 4
    for ch in (src[0], src):                                                # one for every trial; one per trial
        sv, sig = spectrum_trials(p, 4, 3, seed=9, sweep_idx=1, n_keep=Nr, channel=ch, channel_normalize=normalize, want_sigma=True)
        inp = build_trials(p, 4, 3, seed=9, sweep_idx=1, want_draws=True, channel=ch, channel_normalize=normalize)
        torch.cuda.synchronize()
        assert np.array_equal(sig.numpy(), inp["sigma_max"].numpy())        # on the bits
        ps = inp["pilot_sym"].cpu().numpy().astype(complex)
        ref = []
        for t in range(3):
            Hc, _ = cut_and_scale(p, ch if ch.ndim == 3 else ch[t], normalize)
            ref.append(R.spectrum(R.received(Hc.astype(np.complex64).astype(complex), ps[t])))
        # (the library stores the scaled channel as fp32, so numpy's cut and scaled channel is rounded to fp32 as well); and on
        # the library's own H, where nothing but the arithmetic of the spectrum differs
        H = build_trials(p, 4, 3, seed=9, sweep_idx=1, want_H=True, channel=ch, channel_normalize=normalize)["H"].cpu().numpy()
        own = [R.spectrum(R.received(H[t].astype(complex), ps[t])) for t in range(3)]
        e = P.err(sv.cpu().numpy(), np.array(own))
        print("spectrum_trials supplied %s %s: %.3g (fp32-rounded reference channel: %.3g)"
              % (normalize, "shared" if ch.ndim == 3 else "per trial", e, P.err(sv.cpu().numpy(), np.array(ref))))
        check_below("spectrum_sweep_abs_over_s1", e, SWEEP_TOL)
        check_below("spectrum_sweep_abs_over_s1", P.err(sv.cpu().numpy(), np.array(ref)), SWEEP_TOL)


def test_a_nan_in_the_used_block_is_illcond_and_nothing_is_written():
    from jstsp19_amd import _lib
    Nr, Nt, L, Tp = SWEEP_SHAPES[0]
    p = _sp(Nr, Nt, L, Tp)
    rng = np.random.default_rng(2)
    src = P.rand(rng, Nr + 2, Nt, L).astype(np.complex64)
    src[Nr + 1, 0, 0] = np.nan                                               # outside the used block: never read
    flat = np.ascontiguousarray(np.concatenate([src[:, :, l].reshape(-1, order="F") for l in range(L)]))
    c = _lib.default_context(0)
    model = _lib.Model(p.Nt, p.Nr, p.L, p.T_prop, p.Mr, p.Mr_e, p.Gr, p.Gt, 0, 0, 0, 0, p.noise_var, _lib.BF_ZC, _lib.RHO_MIN6, 1.0,
                       _lib.PILOTS_QAM4)
    f = c._lib.jstsp_spectrum_trials_c32
    out, sig = np.full((2, 64), -7.0), np.full(L, -7.0)
    call = lambda buf, mode=_lib.CHAN_REFERENCE, ldr=Nr + 2: f(c.handle, C.byref(model), C.c_uint64(1), 0, 0, 2, buf.ctypes.data, ldr, Nt, 0,
                                                                mode, 64, out.ctypes.data, sig.ctypes.data_as(C.POINTER(C.c_double)), _lib.HOST)
    assert call(flat) == 0 and np.all(np.isfinite(out)) and np.all(sig > 0)
    out[:], sig[:] = -7.0, -7.0
    src[5, 1, 2] = np.nan
    flat = np.ascontiguousarray(np.concatenate([src[:, :, l].reshape(-1, order="F") for l in range(L)]))
    assert call(flat) == _lib.E_ILLCOND
    assert "tap 2" in c._lib.jstsp_last_error().decode()
    assert np.all(out == -7.0) and np.all(sig == -7.0)
    assert call(flat, mode=9) == -4 and call(flat, ldr=Nr - 1) == -2


# ---------------------------------------------------------------------------------------------- the drivers
def _run_tool(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_rank.py")] + list(args), cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_run_rank_with_a_channel_is_the_mean_of_the_per_trial_calls():
    from jstsp19_amd import montecarlo as M
    from jstsp19_amd.system_model import spectrum_trials
    Nr, Nt, L, Tp = SWEEP_SHAPES[0]
    pts = [_sp(Nr, Nt, L, Tp)]
    rng = np.random.default_rng(6)
    ch = P.rand(rng, 5, Nr, Nt, L).astype(np.complex64)
    mean, marker = M.run_rank(pts, 5, batch=2, seed=11, sweep0=40, channel=ch, channel_normalize="unit")
    assert mean.shape == (1, 32) and list(marker) == [L * Nt]
    sv = spectrum_trials(pts[0], 0, 5, seed=11, sweep_idx=40, channel=ch, channel_normalize="unit").cpu().numpy()
    assert np.max(np.abs(mean[0] - sv.mean(axis=0))) <= 1e-14 * sv[:, 0].mean()


def test_run_rank_tool_shape_channel_and_panel(tmp_path):
    out = _run_tool("--shape", "64,4,4,160")
    curves = [l.split() for l in out.splitlines() if l.startswith("L=")]
    assert [c[0] for c in curves] == ["L=4"]
    v = np.array([float(x) for x in curves[0][1:]])
    assert v.size == 32 and P.ordered(v) and v[0] > 0 and v[6] < 1e-4 * v[0]
    rng = np.random.default_rng(3)
    path = str(tmp_path / "chan.npy")
    np.save(path, P.usv(rng, 40, 6, [1.0, 0.5])[:, :, None] * np.array([1.0, 0.3, 0.1])[None, None, :])
    out = _run_tool("--shape", "32,4,3,300", "--channel", path, "--channel-normalize", "unit", "--trials", "2")
    curves = [l.split() for l in out.splitlines() if l.startswith("L=")]
    assert [c[0] for c in curves] == ["L=3"]
    v = np.array([float(x) for x in curves[0][1:]])
    assert v.size == 32 and P.ordered(v) and v[0] > 0
    assert v[2] < 1e-5 * v[0]                      # every tap is the same rank-2 matrix: Y has rank 2
    out = _run_tool("--panel", "1")
    curves = [l.split() for l in out.splitlines() if l.startswith("L=")]
    assert [c[0] for c in curves] == ["L=1", "L=4", "L=8"] and "min(Np, L*Nt)" in out
    for c in curves:
        v = np.array([float(x) for x in c[1:]])
        assert v.size == 32 and P.ordered(v) and v[0] > 0
