"""jstsp_proposed_std_f64 (csrc/proposed64.hip): Alg. 1 - proposed_algorithm.m / proposed_algorithm_angles.m with type 'std' -
in float64 on the device, against oracle/solvers.py on the problems of tests/std64_problems.py.

Bounds (not derived from this code): those of the sibling entry (tests/test_gpu_f64_proposed.py) - S, Y max|d| / max|ref| <= 1e-10,
convergence_error(:, 1:2) 1e-8 relative with the finite pattern equal, convergence_error(:, 3) == 0 exactly - on P1-P5; on P6
(cond(B) = 1e6) max(sibling bound, 100 d), d the distance on P6 itself between the oracle's loop with numpy's pinv(B) and with
the exact pseudo-inverse (std64_problems.p6_bounds: 2.1e-8 / 1.1e-7).  Two float64 statements of Alg. 1 differ by 3.2e-14 /
1.1e-12 on P1, P2 (tests/test_std64_problems.py).
Measured on MI355X: profiles/std64_measured_tolerances.json."""
import numpy as np
import pytest

import std64_problems as P
from conftest import check_below, ce_rel, rel_err, TOL_S  # noqa: E402

pytestmark = pytest.mark.gpu

E_UNSUPPORTED, E_ILLCOND = -3, -6


def _vs(tag, out, ref, tolS=P.TOL64_S, tolce=P.TOL64_CE):
    S, Y, ce = out
    So, Yo, ceo = ref
    assert S.dtype == np.complex128 and Y.dtype == np.complex128
    check_below("std64.%s.S" % tag, rel_err(S, So), tolS)
    check_below("std64.%s.Y" % tag, rel_err(Y, Yo), tolS)
    if ce is not None:
        assert ce.dtype == np.float64 and ce.shape == ceo.shape
        check_below("std64.%s.ce" % tag, ce_rel(ce[..., :2], ceo[..., :2]), tolce)
        assert np.all(ce[..., 2] == 0)


def _eq(a, b):
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
        else:
            np.testing.assert_array_equal(x, y)


@pytest.fixture(scope="module")
def p3():
    """The P3 batch solved once on the host path: (S, Y, ce) without and with indx_S."""
    import jstsp19_amd as J
    p = P.problem("P3")
    return (J.proposed_algorithm_std_f64(*P.args("P3")),
            J.proposed_algorithm_angles_std_f64(p["subY"], p["Omega"], p["indx_S"], *P.args("P3")[2:]))


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P1", "P2", "P4", "P5"])
def test_parity_single_trial_problems(name):
    import jstsp19_amd as J
    _vs(name, J.proposed_algorithm_std_f64(*P.args(name)), P.reference(name))


def test_parity_p3_batch_strides_scalars_and_the_mask(p3):
    import jstsp19_amd as J
    p = P.problem("P3")
    for t in range(5):
        _vs("P3", [x[t] for x in p3[0]], [x[t] for x in P.reference("P3")])
        _vs("P3.angles", [x[t] for x in p3[1]], [x[t] for x in P.reference("P3", True)])
    t, im = P.P3_SATURATE                                   # Imax 60: the mask count 10 + 5 i passes Gr G2 = 288 and saturates
    out = J.proposed_algorithm_angles_std_f64(p["subY"][t], p["Omega"][t], p["indx_S"][t], p["A"], p["B"][t], im, p["tau_Y"][t], p["tau_S"][t],
                                              p["rho"][t])
    _vs("P3.saturated", out, P.reference("P3", True, t, im))


def test_parity_p6_ill_conditioned_factor():
    import jstsp19_amd as J
    bS, bce = P.p6_bounds()
    _vs("P6", J.proposed_algorithm_std_f64(*P.args("P6")), P.reference("P6"), bS, bce)


# ---- 2. closed form ----------------------------------------------------------------------------------------------------------
def test_first_iteration_in_closed_form():
    import jstsp19_amd as J
    from oracle import solvers as O
    subY, Om, A, B, _, tY, tS, rho = P.args("P1")
    S, Y, ce = J.proposed_algorithm_std_f64(subY, Om, A, B, 1, tY, tS, rho)
    X = subY / (Om + 2 * rho)
    Sn = O.soft_threshold_complex(np.linalg.pinv(A) @ X @ np.linalg.pinv(B), tS / rho)
    check_below("std64.closed.S", rel_err(S, Sn), P.TOL64_S)
    assert np.array_equal(Y, np.zeros_like(Y))
    # V1 = rho (Y - X) = -rho X;  C = rho/(rho+1) (X - A S B);  V2 = rho (C - X + A S B)
    Xs = A @ Sn @ B
    C = rho / (rho + 1) * (X - Xs)
    n2 = lambda Z: np.linalg.norm(Z, 2) ** 2
    cen = np.array([[n2(-rho * X) / n2(X), n2(rho * (C - X + Xs)) / n2(X), 0.0]])
    assert ce.shape == (1, 3) and ce[0, 2] == 0
    check_below("std64.closed.ce", ce_rel(ce[:, :2], cen[:, :2]), P.TOL64_CE)


# ---- 3. bits -----------------------------------------------------------------------------------------------------------------
def test_given_factors_return_the_bits_of_the_call_that_computes_them(p3):
    import jstsp19_amd as J
    a = P.args("P3")
    PA, PB = J.pinv_f64(a[2]), J.pinv_f64(a[3])
    assert PA.shape == (12, 16) and PB.shape == (5, 40, 24)
    out = J.proposed_algorithm_std_f64(*a, PA=PA, PB=PB, info=True)
    _eq(out[:3], p3[0])
    assert np.all(np.isnan(out[3]))
    _eq(J.proposed_algorithm_std_f64(*a, PA=PA)[:3], p3[0])                # one side given, the other computed
    rc = J.proposed_algorithm_std_f64(*a, PB=PB, info=True)[3]
    assert np.isfinite(rc[0]) and np.isnan(rc[1])


def test_trial_alone_repeat_no_ce_and_shared_B_return_the_same_bits(p3):
    import jstsp19_amd as J
    subY, Om, A, B, Imax, tY, tS, rho = P.args("P3")
    _eq(J.proposed_algorithm_std_f64(subY[3], Om[3], A, B[3], Imax, tY[3], tS[3], rho[3]), [x[3] for x in p3[0]])
    _eq(J.proposed_algorithm_std_f64(subY, Om, A, B, Imax, tY, tS, rho), p3[0])
    S, Y, ce = J.proposed_algorithm_std_f64(subY, Om, A, B, Imax, tY, tS, rho, want_ce=False)
    assert ce is None
    _eq((S, Y), p3[0][:2])
    shared = J.proposed_algorithm_std_f64(subY, Om, A, B[1], Imax, tY, tS, rho)                     # strideB = 0
    _eq(shared, J.proposed_algorithm_std_f64(subY, Om, A, np.stack([B[1]] * 5), Imax, tY, tS, rho))


def test_host_and_device_memspace_return_the_same_bits(p3):
    import torch
    import jstsp19_amd as J
    p = P.problem("P3")
    dev = torch.device("cuda:0")
    cm = lambda a: J.colmajor(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    a = P.args("P3")
    d = (cm(a[0]), cm(a[1]), cm(a[2]), cm(a[3])) + a[4:]
    out = J.proposed_algorithm_std_f64(*d, info=True)
    outa = J.proposed_algorithm_angles_std_f64(d[0], d[1], torch.from_numpy(p["indx_S"]).to(dev), *d[2:])
    PA, PB = J.pinv_f64(d[2]), J.pinv_f64(d[3])
    outp = J.proposed_algorithm_std_f64(*d, PA=PA, PB=PB, info=True)
    torch.cuda.synchronize()
    assert out[0].dtype == torch.complex128 and out[0].is_cuda and out[3].is_cuda
    _eq([x.cpu().numpy() for x in out[:3]], p3[0])
    _eq([x.cpu().numpy() for x in outa], p3[1])
    _eq([x.cpu().numpy() for x in outp[:3]], p3[0])
    assert torch.isnan(outp[3]).all()
    rc = J.proposed_algorithm_std_f64(*a, info=True)[3]
    np.testing.assert_array_equal(out[3].cpu().numpy(), rc)


# ---- 4. refusals and rcond -----------------------------------------------------------------------------------------------------
def test_refusals_and_rcond():
    import jstsp19_amd as J
    rng = np.random.default_rng(4)
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    subY, Om, A, B, Imax, tY, tS, rho = P.args("P1")
    f = J.proposed_algorithm_std_f64
    # the rank rule of the fp32 entry, with its status
    with pytest.raises(J.JstspError) as e32:
        J.proposed_algorithm(subY, Om, c(7, 8), c(9, 13), 2, tY, tS, rho, "std")
    for Ab, Bb in ((c(7, 8), B), (A, c(14, 13))):                                   # N < Gr; M < G2
        with pytest.raises(J.JstspError) as e:
            f(subY, Om, Ab, Bb, 2, tY, tS, rho)
        assert e.value.code == e32.value.code == E_UNSUPPORTED and "full column rank" in str(e.value)
    B2 = B.copy(); B2[6] = B2[2]                                                    # two equal rows: rank G2 - 1
    with pytest.raises(J.JstspError) as e:
        f(subY, Om, A, B2, 2, tY, tS, rho)
    assert e.value.code == E_ILLCOND and "factor B of trial 0" in str(e.value) and "rank 8 < 9" in str(e.value)
    Bs = np.stack([B, B, B2])                                                       # ... in the third trial of a batch
    with pytest.raises(J.JstspError) as e:
        f(np.stack([subY] * 3), np.stack([Om] * 3), A, Bs, 2, tY, tS, rho)
    assert e.value.code == E_ILLCOND and "factor B of trial 2" in str(e.value)
    A2 = A.copy(); A2[3, 1] = np.nan
    with pytest.raises(J.JstspError) as e:
        f(subY, Om, A2, B, 2, tY, tS, rho)
    assert e.value.code == E_ILLCOND and "factor A" in str(e.value) and "NaN" in str(e.value)
    N, M = 513, 514                                                                 # min(N, M) = 513
    with pytest.raises(J.JstspError) as e:
        f(np.zeros((N, M), complex), np.ones((N, M)), np.zeros((N, 4), complex), np.zeros((3, M), complex), 2, 1.0, 1.0, 1.0)
    assert e.value.code == E_UNSUPPORTED and "513" in str(e.value)
    # rcond against numpy
    out = f(subY, Om, A, B, 2, tY, tS, rho, info=True)
    assert len(out) == 4 and out[3].shape == (2,)
    for k, F in enumerate((A, B)):
        check_below("std64.rcond", abs(out[3][k] * np.linalg.cond(F) - 1), 1e-10)


# ---- 5. the float64 path is the reference of the fp32 'std' branch -------------------------------------------------------------
def test_agreement_with_the_fp32_std_branch_on_p3():
    import jstsp19_amd as J
    subY, Om, A, B, Imax, tY, tS, rho = P.args("P3")
    n = lambda x: x.astype(np.complex64)                                            # both solvers get the values fp32 can hold
    S32, Y32, _ = J.proposed_algorithm(n(subY), Om.astype(np.float32), n(A), n(B), Imax, tY, tS, rho, "std")
    S64, Y64, _ = J.proposed_algorithm_std_f64(n(subY), Om.astype(np.float32), n(A), n(B), Imax, tY, tS, rho)
    for t in range(5):
        check_below("std64.vs_fp32_std.S", rel_err(S32[t].astype(np.complex128), S64[t]), TOL_S)


# ---- 6. the sweep --------------------------------------------------------------------------------------------------------------
def test_approx_sweep_in_float64_and_the_default_unchanged():
    import torch
    from jstsp19_amd import montecarlo as MC
    from jstsp19_amd.system_model import TrainingParams, build_trials_training
    from oracle import solvers as O
    base = TrainingParams(Nt=4, Nr=32, L=4, T=140, ratio=0.75)
    assert base.solver_shape == P.REFNATIVE
    snrs, imax, nt = [0.0, 10.0], [10, 30], 4
    out = MC.run_approx_sweep(base, snrs, imax, nt, precision="f64")
    assert out.shape == (2, 2, 2) and out.dtype == torch.float64 and bool(torch.isfinite(out).all())
    w = lambda x: x.cpu().numpy().astype(np.complex128)
    for si, snr in enumerate(snrs):
        p = TrainingParams(4, 32, 4, 140, 0.75, snr_db=snr)
        inp = build_trials_training(p, 0, nt, sweep_idx=si * len(imax))
        subY, A, B, zb, Om = w(inp["subY"]), w(inp["A"]), w(inp["B"]), w(inp["Zbar"]), inp["Omega"].cpu().numpy().astype(np.float64)
        pA = np.linalg.pinv(A)
        for ii, im in enumerate(imax):
            e = []
            for t in range(nt):
                _, Y, _ = O.proposed_algorithm(subY[t], Om[t], A, B[t], im, float(inp["tau_X"][t]), float(inp["tau_S"][t]), float(inp["rho"][t]),
                                               "std", want_ce=False)
                e.append(O.nmse_capped(pA @ Y @ np.linalg.pinv(B[t]), zb[t]))
            check_below("std64.sweep.alg1_nmse", abs(float(out[ii, si, 0]) - min(1.0, float(np.mean(e)))), 1e-9)
    # the default is the path of before: the same bits as a direct run of it
    f32 = MC.run_approx_sweep(base, snrs, imax, nt, precision="f32")
    direct = torch.zeros(2, 2, 2, dtype=torch.float64)
    for si, snr in enumerate(snrs):
        for ii, im in enumerate(imax):
            p = TrainingParams(4, 32, 4, 140, 0.75, snr_db=snr)
            inp = build_trials_training(p, 0, nt, sweep_idx=si * len(imax) + ii)
            e1, e2 = MC._hip_alg12(inp, im)
            direct[ii, si, 0] = min(float(torch.as_tensor(e1).double().sum()) / nt, 1.0)
            direct[ii, si, 1] = min(float(torch.as_tensor(e2).double().sum()) / nt, 1.0)
    assert torch.equal(f32, direct) and torch.equal(f32, MC.run_approx_sweep(base, snrs, imax, nt))
