"""jstsp_proposed_algorithm_f64 / jstsp_svt_f64 (csrc/proposed64.hip): the float64 evaluation of proposed_algorithm.m:1-73 and
proposed_algorithm_angles.m:1-85 ('approximate') against the committed goldens and oracle/solvers.py.

Bounds (not derived from this code): S, Y max|d| / max|ref| <= 1e-10, convergence_error 1e-8 relative per finite entry with
the finite pattern equal, NMSE 1e-11 - about 2000-4000 x the spread measured between the project's two other float64
restatements (oracle/cpu_port.cpp against the goldens of oracle/solvers.py: 4.3e-14 / 2.4e-12 / 5.1e-15), four orders
below anything a path with an fp32 step in it reaches (2e-6 / 1e-4 / 9e-7).
Measured on MI355X (profiles/f64_measured_tolerances.json): S 6.0e-14, Y 9.0e-14, convergence_error 3.4e-12, NMSE 9.0e-15
(all on the goldens; the oracle cases are below them); svt 2.3e-14; against the narrowing fp32 solver 1.4e-6."""
import numpy as np
import pytest

from conftest import check_below, ce_rel, load_golden, rel_err, TOL_S  # noqa: E402

pytestmark = pytest.mark.gpu

TOL64_S, TOL64_CE, TOL64_NMSE = 1e-10, 1e-8, 1e-11


def _args(g):
    return (g["subY"], g["Omega"], g["A"], g["B"], int(g["Imax"]), float(g["tau_Y"]), float(g["tau_Z"]), float(g["rho"]), "approximate")


@pytest.mark.parametrize("name", ["proposed_small", "proposed_small_lowsnr", "proposed_refnative"])
@pytest.mark.parametrize("angles", [False, True], ids=["approximate", "angles"])
def test_goldens(name, angles):
    import jstsp19_amd as J
    from oracle import solvers as O
    g = load_golden(name)
    a = _args(g)
    if angles:
        S, Y, ce = J.proposed_algorithm_angles_f64(a[0], a[1], g["indx_S"], *a[2:])
    else:
        S, Y, ce = J.proposed_algorithm_f64(*a)
    k = "angles" if angles else "approximate"
    assert S.dtype == np.complex128 and Y.dtype == np.complex128 and ce.dtype == np.float64
    check_below("f64.golden.S", rel_err(S, g["S_" + k]), TOL64_S)
    check_below("f64.golden.Y", rel_err(Y, g["Y_" + k]), TOL64_S)
    check_below("f64.golden.ce", ce_rel(ce, g["ce_" + k]), TOL64_CE)
    check_below("f64.golden.nmse", abs(O.nmse_capped(S, g["Zbar"]) - float(g["nmse_" + k])), TOL64_NMSE)


def _ragged():
    rng = np.random.default_rng(7)
    N, M, Gr, G2 = 7, 13, 5, 9
    A = (rng.standard_normal((N, Gr)) + 1j * rng.standard_normal((N, Gr))) / np.sqrt(N)
    B = (rng.standard_normal((G2, M)) + 1j * rng.standard_normal((G2, M))) / np.sqrt(G2)
    S0 = np.zeros((Gr, G2), complex); S0[1, 2] = 3 + 1j; S0[4, 7] = -2j
    Om = (rng.random((N, M)) < 0.5).astype(float)
    subY = Om * (A @ S0 @ B + 0.05 * (rng.standard_normal((N, M)) + 1j * rng.standard_normal((N, M))))
    return (subY, Om, A, B, 25, 0.01, 0.02, 0.3, "approximate")


def test_ragged_shapes_against_the_oracle():
    import jstsp19_amd as J
    from oracle import solvers as O
    args = _ragged()
    So, Yo, ceo = O.proposed_algorithm(*args)
    S, Y, ce = J.proposed_algorithm_f64(*args)
    check_below("f64.ragged.S", rel_err(S, So), TOL64_S); check_below("f64.ragged.Y", rel_err(Y, Yo), TOL64_S)
    check_below("f64.ragged.ce", ce_rel(ce, ceo), TOL64_CE)


def _batch5(rng):
    N, M, Gr, G2, nb = 16, 40, 12, 24, 5
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    A = c(N, Gr) / np.sqrt(N)
    B = c(nb, G2, M) / np.sqrt(G2)
    S0 = np.zeros((nb, Gr, G2), complex)
    for t in range(nb):
        S0[t].flat[rng.choice(Gr * G2, 4, replace=False)] = 3 * c(4)
    Om = (rng.random((nb, N, M)) < 0.5).astype(float)
    subY = Om * (A @ S0 @ B + 0.05 * c(nb, N, M))
    tY = 0.02 + 0.01 * rng.random(nb); tS = 0.02 + 0.01 * rng.random(nb); rho = 0.2 + 0.3 * rng.random(nb)
    idx = np.stack([rng.permutation(Gr * G2) + 1 for _ in range(nb)])
    return subY, Om, A, B, 20, tY, tS, rho, idx, S0


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_batch_of_five_with_per_trial_B_and_shared_A(device):
    import torch
    import jstsp19_amd as J
    from oracle import solvers as O
    subY, Om, A, B, Imax, tY, tS, rho, idx, S0 = _batch5(np.random.default_rng(31))
    if device:
        dev = torch.device("cuda:0")
        cm = lambda a: J.colmajor(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        out = J.proposed_algorithm_f64(cm(subY), cm(Om), cm(A), cm(B), Imax, tY, tS, rho)
        outa = J.proposed_algorithm_angles_f64(cm(subY), cm(Om), torch.from_numpy(idx).to(dev), cm(A), cm(B), Imax, tY, tS, rho)
        torch.cuda.synchronize()
        assert out[0].dtype == torch.complex128 and out[0].is_cuda
        out, outa = [x.cpu().numpy() for x in out], [x.cpu().numpy() for x in outa]
    else:
        out = J.proposed_algorithm_f64(subY, Om, A, B, Imax, tY, tS, rho)
        outa = J.proposed_algorithm_angles_f64(subY, Om, idx, A, B, Imax, tY, tS, rho)
    for t in range(5):
        for (S, Y, ce), ix in ((out, None), (outa, idx[t])):
            So, Yo, ceo = O.proposed_algorithm(subY[t], Om[t], A, B[t], Imax, tY[t], tS[t], rho[t], "approximate", indx_S=ix)
            check_below("f64.batch5.S", rel_err(S[t], So), TOL64_S); check_below("f64.batch5.Y", rel_err(Y[t], Yo), TOL64_S)
            check_below("f64.batch5.ce", ce_rel(ce[t], ceo), TOL64_CE)
            check_below("f64.batch5.nmse", abs(O.nmse_capped(S[t], S0[t]) - O.nmse_capped(So, S0[t])), TOL64_NMSE)
    # a trial does not depend on the batch around it; a repeated call returns the same bits; no ce -> the same S, Y
    S1, Y1, ce1 = J.proposed_algorithm_f64(subY[3], Om[3], A, B[3], Imax, tY[3], tS[3], rho[3])
    np.testing.assert_array_equal(S1, out[0][3]); np.testing.assert_array_equal(Y1, out[1][3]); np.testing.assert_array_equal(ce1, out[2][3])
    S2, Y2, ce2 = J.proposed_algorithm_f64(subY, Om, A, B, Imax, tY, tS, rho, want_ce=False)
    assert ce2 is None
    np.testing.assert_array_equal(S2, out[0]); np.testing.assert_array_equal(Y2, out[1])


def test_first_iteration_and_agreement_with_the_narrowing_entry():
    import jstsp19_amd as J
    g = load_golden("proposed_refnative")
    a = _args(g)
    S, Y, ce = J.proposed_algorithm_f64(*a[:4], 1, *a[5:])
    assert np.array_equal(Y, np.zeros_like(Y)) and ce.shape == (1, 3) and np.isposinf(ce[0, 2])
    # fp32 generator output is accepted as it is (widened exactly)
    a32 = (a[0].astype(np.complex64), a[1].astype(np.float32), a[2].astype(np.complex64), a[3].astype(np.complex64)) + a[4:]
    Sw, _, _ = J.proposed_algorithm_f64(*a32)
    Sx, _, _ = J.proposed_algorithm_f64(*[x.astype(np.complex128) if np.iscomplexobj(x) else x.astype(np.float64) for x in a32[:4]], *a[4:])
    np.testing.assert_array_equal(Sw, Sx)
    # the _f64 result narrowed to fp32 agrees with the existing (narrowing) solver within its tolerance
    S64, _, _ = J.proposed_algorithm_f64(*a)
    S32, _, _ = J.proposed_algorithm(*a)
    check_below("f64.vs_fp32_solver.S", rel_err(S64.astype(np.complex64), S32), TOL_S)


@pytest.mark.parametrize("shape", [(8, 10), (32, 140), (64, 50), (100, 120)], ids=lambda s: "%dx%d" % s)
def test_svt_against_the_oracle(shape):
    import jstsp19_amd as J
    from oracle import solvers as O
    rng = np.random.default_rng(shape[0])
    Y = rng.standard_normal((3,) + shape) + 1j * rng.standard_normal((3,) + shape)
    tau = np.array([0.5, 2.0, 7.0])
    X = J.svt_f64(Y, tau)
    assert X.dtype == np.complex128
    for t in range(3):
        check_below("f64.svt", rel_err(X[t], O.svt(Y[t], tau[t])), 1e-10)


def test_svt_zero_matrix_and_rank_one_closed_form():
    import jstsp19_amd as J
    X = J.svt_f64(np.zeros((12, 20), complex), 0.3)
    assert np.array_equal(X, np.zeros((12, 20), complex))
    rng = np.random.default_rng(2)
    u = rng.standard_normal(12) + 1j * rng.standard_normal(12)
    v = rng.standard_normal(20) + 1j * rng.standard_normal(20)
    Y = np.outer(u, v.conj())
    s = np.linalg.norm(u) * np.linalg.norm(v)
    for tau in (0.25 * s, 2.0 * s):
        ref = max(0.0, 1.0 - tau / s) * Y                 # svt of a rank-1 matrix: its one singular value shrunk by tau
        X = J.svt_f64(Y, tau)
        check_below("f64.svt.rank1", np.max(np.abs(X - ref)) / np.max(np.abs(Y)), 1e-10)


def test_std_large_orders_and_bad_shapes_are_refused():
    import jstsp19_amd as J
    g = load_golden("proposed_small")
    a = _args(g)
    with pytest.raises(J.JstspError) as e:
        J.proposed_algorithm_f64(*a[:8], "std")
    assert e.value.code == -3 and "jstsp_proposed_algorithm_c64" in str(e.value)
    rng = np.random.default_rng(0)
    N, M = 520, 516
    with pytest.raises(J.JstspError) as e:
        J.proposed_algorithm_f64(np.zeros((N, M), complex), np.ones((N, M)), np.zeros((N, 4), complex), np.zeros((3, M), complex), 2, 1.0, 1.0, 1.0)
    assert e.value.code == -3
    with pytest.raises(J.JstspError) as e:
        J.svt_f64(rng.standard_normal((513, 600)) + 0j, 1.0)
    assert e.value.code == -3
    with pytest.raises(ValueError):
        J.proposed_algorithm_f64(g["subY"], g["Omega"][:, :-1], g["A"], g["B"], 5, 1.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        J.proposed_algorithm_f64(g["subY"], g["Omega"], g["A"][:-1], g["B"], 5, 1.0, 1.0, 1.0)
