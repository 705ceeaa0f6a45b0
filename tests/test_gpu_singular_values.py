"""Singular values on the device (csrc/svdvals.hip): the float64 one-sided Jacobi kernel on given matrices against
numpy.linalg.svd in float64 on the same operand values, and the spectrum sweep of plot_rankR.m against the float64 SVD of the
receive signal rebuilt (tests/rank_ref.py) from jstsp_build_trials_c32's own channel and pilots for the same trials.

Accuracy bounds (the project's ~5 x the largest value measured on MI355X; what was measured is in
profiles/rank_measured_tolerances.json):

    SV_TOL       max_k |sv_k - ref_k| / ref_1, given matrices          measured 1.81e-14 (128 x 50, sigma graded)
    SWEEP_TOL    the same quantity for jstsp_rank_trials_c32            measured 9.7e-15
    GRADED_REL   |sv_k - ref_k| / ref_k over sv_k >= 1e-10 sv_1,        measured 6.3e-8
                 sigma graded over 12 decades

One condition on SV_TOL and SWEEP_TOL was fixed before anything was measured: <= 1e-10.  A route through a Gram matrix cannot
go below sqrt(eps) = 1.5e-8 on the rank-deficient cases, so a bound of 1e-10 shows that the one-sided kernel is what runs.
GRADED_REL compares two backward-stable algorithms on a matrix with a dense V: each is within a few eps sigma_1 of the exact
value ABSOLUTELY, which at sv_k = 1e-10 sigma_1 allows a relative 1e-6 to 1e-5 for either (the measured value is lower); it
says that the small values are resolved at all (a float64 Gram loses everything below 1e-8 sigma_1), not that they carry 16
digits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rank_ref as R
from conftest import check_below

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SV_TOL = 9e-14
SWEEP_TOL = 5e-14
GRADED_REL = 3.2e-7
assert SV_TOL <= 1e-10 and SWEEP_TOL <= 1e-10

SHAPES = [(32, 50), (64, 50), (128, 50), (50, 128), (64, 64), (128, 64), (1, 7), (7, 1), (5, 5)]
FILL = 300           # more matrices than the chip has compute units


def _rand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _ref(Y):
    """float64 singular values per matrix on the operand values the device saw."""
    return np.linalg.svd(np.asarray(Y, dtype=np.complex128), compute_uv=False)


def _err(sv, ref):
    """max_k |sv_k - ref_k| / ref_1, the largest over the batch."""
    sv, ref = np.atleast_2d(sv), np.atleast_2d(ref)
    assert sv.shape == ref.shape, (sv.shape, ref.shape)
    return float(np.max(np.abs(sv - ref) / ref[:, :1]))


def _ordered(sv):
    sv = np.atleast_2d(sv)
    return bool(np.all(sv >= 0) and np.all(np.diff(sv, axis=1) <= 0))


def _on_device(Y):
    import jstsp19_amd as J
    return J.colmajor(torch.from_numpy(np.ascontiguousarray(Y)).to("cuda:0"))


def _orth(rng, n, k):
    q, _ = np.linalg.qr(_rand(rng, n, k))
    return q


def _usv(rng, rows, cols, sigma):
    """U diag(sigma) V^H in float64 with random orthonormal U (rows x k) and V (cols x k)."""
    sigma = np.asarray(sigma, dtype=np.float64)
    return (_orth(rng, rows, sigma.size) * sigma) @ _orth(rng, cols, sigma.size).conj().T


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_shapes_batches_and_memspaces(rows, cols, dtype):
    import jstsp19_amd as J
    rng = np.random.default_rng(rows * 1000 + cols)
    for batch in (1, FILL):
        Y = (_rand(rng, batch, rows, cols) * 0.3).astype(dtype)
        sv = J.singular_values(Y)
        assert sv.dtype == np.float64 and sv.shape == (batch, min(rows, cols)) and _ordered(sv)
        e = _err(sv, _ref(Y))
        print("svdvals %dx%d batch %d %s: %.3g" % (rows, cols, batch, np.dtype(dtype).name, e))
        check_below("svdvals_abs_over_s1", e, SV_TOL)
        svd = J.singular_values(_on_device(Y))
        torch.cuda.synchronize()
        assert svd.is_cuda and svd.dtype == torch.float64
        assert np.array_equal(svd.cpu().numpy(), sv)                       # both memspaces give the same bits
        assert np.array_equal(J.singular_values(Y[0]), sv[0])               # a 2-D operand; and no dependence on the batch


def test_conditioning_rank_deficient_graded_repeated_and_zero():
    import jstsp19_amd as J
    rng = np.random.default_rng(77)
    cases = {
        "rank6": np.stack([_usv(rng, 32, 50, rng.uniform(0.5, 2.0, 6)) for _ in range(8)]),
        "graded": np.stack([_usv(rng, 32, 50, np.logspace(0, -12, 32)) for _ in range(8)]),
        "graded_tall": np.stack([_usv(rng, 128, 50, 3.0 * np.logspace(0, -12, 50)) for _ in range(4)]),
        "repeated": np.stack([_usv(rng, 64, 50, np.repeat([2.0, 1.0, 1.0, 0.25, 0.25], 10)) for _ in range(4)]),
        "identity": np.eye(64, dtype=complex)[None],
    }
    for name, Y in cases.items():
        ref = _ref(Y)
        sv = J.singular_values(Y)                                            # complex128: the constructed values themselves
        e = _err(sv, ref)
        print("svdvals %s c64: %.3g" % (name, e))
        check_below("svdvals_abs_over_s1", e, SV_TOL)
        assert _ordered(sv)
        Y32 = Y.astype(np.complex64)
        e = _err(J.singular_values(Y32), _ref(Y32))
        print("svdvals %s c32: %.3g" % (name, e))
        check_below("svdvals_abs_over_s1", e, SV_TOL)
        if name == "rank6":                                                  # the tail a Gram cannot give (sqrt(eps) = 1.5e-8)
            check_below("svdvals_rank6_tail_over_s1", float(np.max(sv[:, 6:] / sv[:, :1])), 1e-10)
        if name.startswith("graded"):
            keep = ref >= 1e-10 * ref[:, :1]
            rel = float(np.max(np.abs(sv - ref)[keep] / ref[keep]))
            print("svdvals %s relative, sv_k >= 1e-10 sv_1: %.3g" % (name, rel))
            check_below("svdvals_graded_rel", rel, GRADED_REL)
    for dt in (np.complex64, np.complex128):
        z = J.singular_values(np.zeros((3, 32, 50), dt))
        assert np.array_equal(z, np.zeros((3, 32))) and not np.any(np.signbit(z))         # exact zeros out
    # scale: the operand is brought to O(1) by a power of two, so huge and tiny matrices lose nothing
    Y = cases["rank6"][0]
    base = J.singular_values(Y)
    for s in (2.0 ** 400, 2.0 ** -400):
        assert np.array_equal(J.singular_values(Y * s), base * s)


def test_order_sign_adjoint_and_permutation():
    import jstsp19_amd as J
    rng = np.random.default_rng(9)
    for rows, cols in ((32, 50), (128, 64), (5, 5)):
        Y = _rand(rng, 6, rows, cols)
        sv = J.singular_values(Y)
        assert _ordered(sv)
        svh = J.singular_values(np.ascontiguousarray(np.conj(np.swapaxes(Y, 1, 2))))
        check_below("svdvals_adjoint_abs_over_s1", _err(svh, sv), SV_TOL)
        perm = rng.permutation(cols)
        check_below("svdvals_permutation_abs_over_s1", _err(J.singular_values(Y[:, :, perm]), sv), SV_TOL)
        check_below("svdvals_permutation_abs_over_s1", _err(J.singular_values(-1j * Y), sv), SV_TOL)


def test_bad_input():
    import jstsp19_amd as J
    rng = np.random.default_rng(4)
    for dt in (np.complex64, np.complex128):
        Y = _rand(rng, 6, 32, 50).astype(dt)
        clean = J.singular_values(Y)
        Y[1, 7, 2] = np.inf
        Y[3, 0, 0] = complex(np.nan, 0.0)
        Y[4, 31, 49] = complex(0.0, -np.inf)
        sv = J.singular_values(Y)
        assert np.all(np.isnan(sv[[1, 3, 4]]))
        assert np.array_equal(sv[[0, 2, 5]], clean[[0, 2, 5]])               # ... for that matrix only
    for rows, cols in ((65, 65), (128, 65), (100, 90), (8193, 1), (1, 8193)):
        with pytest.raises(J.JstspError) as e:
            J.singular_values(_rand(rng, rows, cols).astype(np.complex64))
        assert e.value.code == -3, (rows, cols)                              # JSTSP_E_UNSUPPORTED, no Gram fall-back
    assert J.singular_values(_rand(rng, 8192, 1)).shape == (1,)               # the limit itself
    # the values are returned where Y lives: the Python entry allocates them there, as solvers.ase does; a CPU torch tensor
    # is refused like everywhere else in the package
    Y = _rand(rng, 2, 7, 5).astype(np.complex64)
    assert isinstance(J.singular_values(Y), np.ndarray)
    assert J.singular_values(_on_device(Y)).device == torch.device("cuda:0")
    with pytest.raises(ValueError):
        J.singular_values(torch.from_numpy(Y))
    # and the C entry refuses what its neighbours refuse
    from jstsp19_amd import _lib
    c = _lib.default_context(0)
    out = np.zeros(10)
    f = c._lib.jstsp_singular_values_c32
    assert f(c.handle, 7, 5, 2, None, out.ctypes.data, _lib.HOST) == -1
    assert f(c.handle, 7, 5, 2, Y.ctypes.data, None, _lib.HOST) == -1
    assert f(c.handle, 0, 5, 2, Y.ctypes.data, out.ctypes.data, _lib.HOST) == -2
    assert f(c.handle, 7, 5, 2, Y.ctypes.data, out.ctypes.data, 5) == -4


def test_largest_value_agrees_with_lambda_max():
    """sv_1^2 against lambda_max of Y Y^H from the Lanczos kernel (jstsp_lambda_max_sequence_c32), within that entry's stated
    2e-5 relative (include/jstsp.h)."""
    import jstsp19_amd as J
    rng = np.random.default_rng(12)
    for rows, cols in ((32, 50), (64, 64), (128, 64)):
        Y = (_rand(rng, 5, rows, cols) * 0.3).astype(np.complex64)
        Yd = Y.astype(np.complex128)
        G = (Yd @ np.conj(np.swapaxes(Yd, 1, 2))).astype(np.complex64)
        lam = J.lambda_max_sequence(G[None])[0].astype(np.float64)
        sv = J.singular_values(Y)
        check_below("svdvals_vs_lambda_max_rel", float(np.max(np.abs(sv[:, 0] ** 2 - lam) / lam)), 2e-5)


# ---------------------------------------------------------------------------------------------- the device-built sweep
def _point(panel, L):
    from jstsp19_amd import montecarlo as M
    return [p for p in M.rank_points(panel) if p.L == L][0]


def _rebuilt(p, trial0, batch, seed, sweep_idx, **kw):
    """Y per trial in float64 from the H and pilot symbols jstsp_build_trials_c32 returns (the fp32 values, widened)."""
    from jstsp19_amd.system_model import build_trials
    inp = build_trials(p, trial0, batch, seed=seed, sweep_idx=sweep_idx, want_H=True, want_draws=True, **kw)
    torch.cuda.synchronize()
    ps = inp["pilot_sym"].cpu().numpy()
    if kw.get("pilots") == "gauss":
        ps = ps * np.float32(0.70710678)                 # ...training.m:20, in fp32 as the pilot kernels scale them
    H = inp["H"].cpu().numpy().astype(complex)
    return [R.received(H[t], ps[t].astype(complex)) for t in range(batch)], ps


@pytest.mark.parametrize("panel", [1, 2, 3, 4, 5, 6])
def test_device_sweep_against_float64_of_build_trials(panel):
    from jstsp19_amd.system_model import rank_trials
    for L in R.L_RANGE:
        p = _point(panel, L)
        sv = rank_trials(p, 3, 12, seed=20190913, sweep_idx=5)
        torch.cuda.synchronize()
        sv = sv.cpu().numpy()
        assert sv.shape == (12, 32) and _ordered(sv) and np.all(np.isfinite(sv))
        Ys, _ = _rebuilt(p, 3, 12, 20190913, 5)
        ref = np.array([R.spectrum(Y, 32) for Y in Ys])
        e = _err(sv, ref)
        print("rank_trials panel %d L %d: %.3g" % (panel, L, e))
        check_below("rank_trials_abs_over_s1", e, SWEEP_TOL)
        full = rank_trials(p, 3, 12, seed=20190913, sweep_idx=5, n_keep=min(p.Nr, 50)).cpu().numpy()
        assert np.array_equal(full[:, :32], sv)
        check_below("rank_trials_abs_over_s1", _err(full, np.array([R.spectrum(Y) for Y in Ys])), SWEEP_TOL)


def test_device_sweep_does_not_depend_on_the_batch_nor_on_the_memspace():
    from jstsp19_amd import _lib
    from jstsp19_amd.system_model import rank_trials
    p = _point(5, 4)
    big = rank_trials(p, 0, 40, seed=3, sweep_idx=2)
    small = rank_trials(p, 5, 7, seed=3, sweep_idx=2)
    torch.cuda.synchronize()
    assert torch.equal(big[5:12], small)
    c = _lib.Context(0)
    model = _lib.Model(p.Nt, p.Nr, p.L, p.T_prop, p.Mr, p.Mr_e, p.Gr, p.Gt, p.clusters, p.rays, 0, 0, p.noise_var,
                       _lib.BF_ZC, _lib.RHO_MIN6, 1.0, _lib.PILOTS_QAM4)
    host = np.full((7, 32), -1.0)
    _lib.check(c._lib.jstsp_rank_trials_c32(c.handle, C.byref(model), C.c_uint64(3), 2, 5, 7, 32, host.ctypes.data, _lib.HOST),
               "jstsp_rank_trials_c32")
    assert np.array_equal(host, small.cpu().numpy())
    for bad_keep in (0, 51):
        assert c._lib.jstsp_rank_trials_c32(c.handle, C.byref(model), C.c_uint64(3), 2, 5, 7, bad_keep, host.ctypes.data,
                                            _lib.HOST) == -2
    model.T_prop = 200                                                       # 64 x 200 does not fit
    assert c._lib.jstsp_rank_trials_c32(c.handle, C.byref(model), C.c_uint64(3), 2, 5, 7, 32, host.ctypes.data, _lib.HOST) == -3
    c.close()


@pytest.mark.parametrize("pilots,shared", [("gauss", False), ("qam4", True)])
def test_device_sweep_follows_the_pilot_options_of_build_trials(pilots, shared):
    from jstsp19_amd.system_model import rank_trials
    p = _point(2, 4)
    sv = rank_trials(p, 2, 16, seed=5, sweep_idx=6, pilots=pilots, shared_pilots=shared)
    torch.cuda.synchronize()
    Ys, ps = _rebuilt(p, 2, 16, 5, 6, pilots=pilots, shared_pilots=shared)
    if shared:
        assert np.array_equal(ps[0], ps[-1])
    check_below("rank_trials_abs_over_s1", _err(sv.cpu().numpy(), np.array([R.spectrum(Y, 32) for Y in Ys])), SWEEP_TOL)


def test_the_statement_of_the_figure():
    """Over 256 trials of each of the 18 points sv_{r+1} / sv_1, r = min(Np, L*Nt, Nr, T), of the device sweep stays within 10 x
    the largest value the float64 reference gives for the same trials (numpy SVD of Y rebuilt from build_trials' H and pilot
    symbols).  H reaches either of them as float32, so that tail is of order 6e-8 sqrt(Nr Nt L), not zero.  Every trial
    counts.  (Panel 4 at L = 8: r = 32 = Nr, Y has no 33rd singular value - for the device and the reference alike - so the
    point contributes the bound only through its 32 existing values being finite and ordered.)"""
    from jstsp19_amd.system_model import rank_trials
    n = 256
    dev_max, ref_max = 0.0, 0.0
    for panel in range(1, 7):
        for i, L in enumerate(R.L_RANGE):
            p = _point(panel, L)
            r = R.rank_bound(p.clusters * p.rays, L, Nr=p.Nr)
            n_all = min(p.Nr, p.T_prop)
            keep = min(r + 1, n_all)
            sv = rank_trials(p, 0, n, seed=777, sweep_idx=10 * panel + i, n_keep=keep)
            torch.cuda.synchronize()
            sv = sv.cpu().numpy()
            assert sv.shape == (n, keep) and _ordered(sv) and np.all(np.isfinite(sv))
            if r >= n_all:
                continue
            Ys, _ = _rebuilt(p, 0, n, 777, 10 * panel + i)
            ref = np.array([R.spectrum(Y, keep) for Y in Ys])
            d, f = float(np.max(sv[:, r] / sv[:, 0])), float(np.max(ref[:, r] / ref[:, 0]))
            print("tail panel %d L %d r %d: device %.3g float64 %.3g" % (panel, L, r, d, f))
            dev_max, ref_max = max(dev_max, d), max(ref_max, f)
    check_below("rank_tail_float64_reference", ref_max, 1.0)          # recorded; a ratio of singular values is below 1
    check_below("rank_tail_device", dev_max, 10.0 * ref_max)


def test_run_rank_is_the_mean_of_the_per_trial_calls():
    from jstsp19_amd import montecarlo as M
    from jstsp19_amd.system_model import rank_trials
    pts = M.rank_points(4)
    mean, marker = M.run_rank(pts, 8, batch=3, seed=11, sweep0=40)
    assert mean.shape == (3, 32) and list(marker) == [4, 16, 32]
    for i, p in enumerate(pts):
        sv = rank_trials(p, 0, 8, seed=11, sweep_idx=40 + i).cpu().numpy()
        assert np.max(np.abs(mean[i] - sv.mean(axis=0))) <= 1e-14 * sv[:, 0].mean()
    one, _ = M.run_rank(pts, seed=11, sweep0=40)                               # the reference's single realisation
    assert np.array_equal(one[2], rank_trials(pts[2], 0, 1, seed=11, sweep_idx=42).cpu().numpy()[0])


def test_run_rank_driver():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_rank.py"), "--panel", "1"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    curves = [l.split() for l in r.stdout.splitlines() if l.startswith("L=")]
    assert [c[0] for c in curves] == ["L=1", "L=4", "L=8"]
    for c, rank in zip(curves, (4, 6, 6)):
        v = np.array([float(x) for x in c[1:]])
        assert v.size == 32 and _ordered(v) and v[0] > 0
        assert v[rank] < 1e-4 * v[0] < v[0]                                    # the drop the figure marks
    assert "min(Np, L*Nt)" in r.stdout
