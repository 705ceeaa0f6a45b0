"""The TSSR / SVT-based recipe in float64, ``tssr_f64`` (jstsp_mc_svt_f64, jstsp_pinv_f64, jstsp_synthesize_f64, jstsp_ls_f64,
jstsp_mmv_omp_f64), and ``mmv_precision="f64"`` of the sweep runner.

(a) the committed fixture tests/golden/baselines2.npz: Y_svt within 1e-10, S_tssr and S_svt within 1e-9 of the fixture's (every
    selection gap of that fixture is >= 3.3e-2, the support condition is 3.3, cond(B_t) = 2.6);
(b) a shape the fp32 chain refuses - B 16 x 700: (700 * 16 + 16^2) * 16 B = 179 KiB is above the in-LDS pinv limit - against
    oracle/solvers.py tssr for both row scores with the bounds of (a) (asserted in the test on the oracle alone: every selection gap is >= 0.17 (l2) and
    >= 0.08 (l1), the support condition is below 2.3 and cond(B) below 1.3 - the draws are made in the order of the test's lines,
    which fixes these figures), while ``solvers.tssr`` raises JSTSP_E_UNSUPPORTED on the same inputs;
(c) the sweep runner at the BASELINE configs[1] shape: ``mmv_precision="f64"`` returns finite omp_mmv, tssr and svt columns, the
    omp_mmv NMSE is the float64 LS NMSE (numOfnz = 100 >= 64 atoms of a square A: joint OMP is the LS estimate), and the call
    without ``mmv_precision`` returns the same bits before and after;
(d) ``mmv_precision="f64"`` with the default fp32 least squares, at the drivers' own small shape where that path runs: the three
    float64 columns of the ``ls_precision="f64"`` call on the bits, beside the default call's own LS and VAMP columns."""
import time

import numpy as np
import pytest

from conftest import check_below, load_golden, rel_err
from oracle import solvers as O

pytestmark = pytest.mark.gpu

TOL_Y, TOL_S = 1e-10, 1e-9


def c_(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_the_committed_fixture():
    import torch
    import jstsp19_amd as J
    g = load_golden("baselines2")
    args = (g["Y_t"], g["Omega_t"], g["A"], g["B_t"], int(g["Imax_t"]), float(g["tau_t"]), float(g["rho_t"]), int(g["K_t"]))
    S, Y, Ssvt = J.tssr_f64(*args)
    assert all(x.dtype == np.complex128 for x in (S, Y, Ssvt))
    check_below("tssr64.fixture.Y_svt", rel_err(Y, g["Y_svt"]), TOL_Y)
    check_below("tssr64.fixture.S_tssr", rel_err(S, g["S_tssr"]), TOL_S)
    check_below("tssr64.fixture.S_svt", rel_err(Ssvt, g["S_svt"]), TOL_S)
    # device-resident complex64 / float32 tensors: widened exactly, the host call's bits
    dev = torch.device("cuda:0")
    t_ = lambda a, dt: J.colmajor(torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).to(dev))
    a32 = [np.asarray(a).astype(dt) for a, dt in zip(args[:4], (np.complex64, np.float32, np.complex64, np.complex64))]
    host = J.tssr_f64(*a32, *args[4:])
    out = J.tssr_f64(*[t_(a, a.dtype) for a in a32], *args[4:])
    torch.cuda.synchronize()
    for h, d, what in zip(host, out, ("S_tssr", "Y_svt", "S_svt")):
        assert d.dtype == torch.complex128 and same_bits(h, d.cpu().numpy()), what


def test_a_shape_the_fp32_chain_refuses():
    import jstsp19_amd as J
    rng = np.random.default_rng(11)
    N = Gr = G2 = 16
    M = 700
    A, B = c_(rng, N, Gr) / np.sqrt(2 * N), c_(rng, G2, M) / np.sqrt(2 * M)
    Z0 = np.zeros((Gr, G2), complex)
    Z0[rng.choice(Gr, 3, replace=False)] = 3.0 * c_(rng, 3, G2)
    Yfull = A @ Z0 @ B + 0.01 * c_(rng, N, M)
    Omega = np.zeros((N, M))
    for j in range(M):
        Omega[rng.choice(N, 8, replace=False), j] = 1.0
    Yp = Omega * Yfull
    rho, Imax, K = 0.1, 30, 6
    tau = 0.05 * rho * np.linalg.norm(Yp, 2)
    assert (M * G2 + G2 * G2) * 16 > 156 * 1024
    T_ref = O.mc_svt(Yp, Omega, Imax, tau, rho) @ np.linalg.pinv(B)
    for norm, gap_min in (("l2", 0.17), ("l1", 0.08)):
        ref = O.tssr(Yp, Omega, A, B, Imax, tau, rho, K, norm)
        _, sup, gaps = O.mmv_omp_margins(A, T_ref, K, norm)           # facts of the problem, from the oracle alone
        cond_s, cond_b = np.linalg.cond(A[:, sup - 1]), np.linalg.cond(B)
        print("%s: oracle support %s, smallest gap %.3g, cond(A[:, support]) %.3g, cond(B) %.3g" % (norm, sup.tolist(), gaps.min(), cond_s, cond_b))
        assert len(sup) == K and gaps.min() >= gap_min and cond_s < 2.3 and cond_b < 1.3, (norm, gaps, cond_s, cond_b)
        S, Y, Ssvt = J.tssr_f64(Yp, Omega, A, B, Imax, tau, rho, K, norm=norm)
        print("%s: Y_svt %.3g S_tssr %.3g S_svt %.3g, rows of S_tssr %d" % (norm, rel_err(Y, ref[1]), rel_err(S, ref[0]), rel_err(Ssvt, ref[2]),
                                                                          int(np.count_nonzero(np.abs(S).sum(1)))))
        assert np.array_equal(np.abs(S).sum(1) > 0, np.abs(ref[0]).sum(1) > 0), norm
        check_below("tssr64.wideB.Y_svt", rel_err(Y, ref[1]), TOL_Y)
        check_below("tssr64.wideB.S_tssr", rel_err(S, ref[0]), TOL_S)
        check_below("tssr64.wideB.S_svt", rel_err(Ssvt, ref[2]), TOL_S)
    with pytest.raises(J.JstspError) as e:
        J.tssr(Yp.astype(np.complex64), Omega.astype(np.float32), A.astype(np.complex64), B.astype(np.complex64), Imax, tau, rho, K)
    assert e.value.code == -3                                      # JSTSP_E_UNSUPPORTED


def _bits(d):
    return {k: v.double().cpu().numpy().tobytes() for k, v in d.items()}


def test_the_sweep_runner_with_mmv_precision_f64():
    import torch
    from jstsp19_amd import montecarlo as mc
    from jstsp19_amd.system_model import SweepParams, build_trials
    p = SweepParams(Nt=64, Nr=64, L=8, T=64, Mr=8, snr_db=5.0)
    inp = build_trials(p, 0, 2, seed=20190913, sweep_idx=0, device=torch.device("cuda", 0), with_hbf=True)
    before = mc._hip_baselines(inp, 100, tssr=(10, 0.1), ls_precision="f64")
    t0 = time.perf_counter()
    f = mc._hip_baselines(inp, 100, tssr=(10, 0.1), ls_precision="f64", mmv_precision="f64")
    torch.cuda.synchronize()
    print("_hip_baselines(mmv_precision='f64'), 2 trials at configs[1]: %.2f s" % (time.perf_counter() - t0))
    for k in ("omp_mmv", "tssr", "svt"):
        assert k in f and f[k].shape == (2,) and torch.isfinite(f[k]).all(), (k, f.get(k))
    assert same_bits(f["ls"].numpy(), before["ls"].double().cpu().numpy())
    A, B, Y = (inp[k].cpu().numpy().astype(np.complex128) for k in ("A_hbf", "B_hbf", "Y_hbf"))
    zb = inp["Zbar"].cpu().numpy().astype(np.complex128)
    assert A.shape[-2] == A.shape[-1] == 64
    for t in range(2):
        At = A if A.ndim == 2 else A[t]
        ref = O.nmse_capped(np.linalg.pinv(At) @ Y[t] @ np.linalg.pinv(B[t]), zb[t])
        print("trial %d: omp_mmv NMSE %.12g, float64 LS NMSE %.12g, tssr %.6g, svt %.6g" % (t, float(f["omp_mmv"][t]), ref, float(f["tssr"][t]),
                                                                                        float(f["svt"][t])))
        check_below("tssr64.sweep.omp_mmv_vs_ls_dNMSE", abs(float(f["omp_mmv"][t]) - ref), 1e-9)
    after = mc._hip_baselines(inp, 100, tssr=(10, 0.1), ls_precision="f64")
    assert _bits(before) == _bits(after)


def test_mmv_precision_f64_beside_the_default_least_squares():
    """the ``mmv_precision`` branch inside the fp32 path of ``_hip_baselines``, at plot_errorVSsnr.m:8-23's own parameters (B_hbf fits
    the in-LDS pinv: the default path runs)."""
    import torch
    from jstsp19_amd import montecarlo as mc
    from jstsp19_amd.system_model import SweepParams, build_trials
    p = SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4, snr_db=6.0)
    inp = build_trials(p, 0, 3, seed=616, device=torch.device("cuda", 0), with_hbf=True)
    d = mc._hip_baselines(inp, 100, tssr=(10, 0.1))
    g = mc._hip_baselines(inp, 100, tssr=(10, 0.1), mmv_precision="f64")
    f = mc._hip_baselines(inp, 100, tssr=(10, 0.1), ls_precision="f64", mmv_precision="f64")
    assert set(g) == set(d) == set(f) and {"ls", "omp_mmv", "tssr", "svt"} <= set(g), (sorted(d), sorted(g), sorted(f))
    for k in ("omp_mmv", "tssr", "svt"):
        assert g[k].dtype == torch.float64 and torch.isfinite(g[k]).all(), (k, g[k])
        assert same_bits(g[k].numpy(), f[k].numpy()), k
        print("%s: default %s, mmv_precision='f64' %s" % (k, d[k].double().cpu().tolist(), g[k].tolist()))
    for k in set(d) - {"omp_mmv", "tssr", "svt"}:                         # LS, VAMP: the default call's own
        assert _bits({k: g[k]}) == _bits({k: d[k]}), k
    assert _bits(d) == _bits(mc._hip_baselines(inp, 100, tssr=(10, 0.1)))
