"""proposed_algorithm 'std' (Alg. 1: v = U\\(L\\k), proposed_algorithm.m:29,53), jstsp_ls_c32 and jstsp_pinv_c32 against float64:
the oracle's 'std' solve and numpy's pinv.

1. The Alg. 1 driver's operating point (plot_errorVSsnr_approx.m: SNR -15:5:15 dB, Imax 10 / 30 / 50, the library's training
   builder), both types scored as the driver scores them: |dNMSE| <= 1e-6 per trial, as for 'approximate'.
2. Every route through the 'std' branch (tests/std_problems.py: route) - the float64 pinv kernel, the Gram inverse by
   eigen-decomposition (order <= 128) and by Newton-Schulz (order > 128) - with the call's variants.
3. Conditioning sweeps with constructed factors: a call meets the documented accuracy (pinv kernel: K * 6e-8 * cond; Gram
   route: K * 6e-8 * cond^2) or fails with JSTSP_E_ILLCOND; it never returns truncated digits silently.

Every bound goes through check_below under its own name (the measured maxima land in measured_tolerances.json)."""
import os

import numpy as np
import pytest

import std_problems as P
from conftest import rel_err, check_below, ce_rel, TOL_NMSE

pytestmark = pytest.mark.gpu

EPS = 6e-8          # unit roundoff of fp32 ("relative error ~ 6e-8 * cond(factor)[^2]")
K = 64              # the one constant of every conditioning bound below (5x the largest k measured, 12.2).  On the Gram
                    # route K * 6e-8 * cond^2 reaches 1 at cond ~ 510: there the bound only rules out noise, and what holds
                    # the top of the sweep is the refusal rule (a truncated or unconverged inverse is refused)
TOL_STD = 5e-6      # S, Y vs the oracle at the driver's operating point: max|d| / max|ref|          (measured 5.1e-7)
TOL_DRIVER_CE = 5e-5  # there, convergence_error(:, j), j = 1, 2: max|d| / max|ref| per column            (measured 1.2e-6)
TOL_STD_CE = 3e-4   # constructed problems, convergence_error(:, 1:2): relative per entry             (measured 6.1e-5)
PRM = (0.01, 0.02, 0.3)       # tau_Y, tau_S, rho of the constructed problems


def _dev(a):
    import torch
    import jstsp19_amd as J
    return J.colmajor(torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0")))


def _np(t):
    return t.cpu().numpy()


def _oracle(subY, Om, A, B, Imax, tY, tS, rho, kind="std", indx=None, want_ce=True):
    from oracle import solvers as O
    return O.proposed_algorithm(np.asarray(subY, complex), np.asarray(Om, float), np.asarray(A, complex), np.asarray(B, complex),
                                Imax, tY, tS, rho, kind, indx_S=indx, want_ce=want_ce)


# ---------------------------------------------------------------------------------------------------- 1. the driver
def test_alg1_driver_operating_point_per_trial_against_float64():
    """plot_errorVSsnr_approx.m:34-72 trial by trial: 7 SNRs x 3 Imax x 4 trials = 84 per type, both types through the HIP path
    and the float64 oracle on identical complex64 inputs, scored S = pinv(A)*Y*pinv(B) (jstsp_ls_c32 / numpy)."""
    import torch
    import jstsp19_amd as J
    from jstsp19_amd.system_model import TrainingParams, build_trials_training
    from oracle import solvers as O
    dev = torch.device("cuda:0")
    dn = {"std": [], "approximate": []}
    for si, snr in enumerate(range(-15, 16, 5)):
        for ii, Imax in enumerate((10, 30, 50)):
            p = TrainingParams(snr_db=float(snr))
            inp = build_trials_training(p, 0, 4, seed=20190913, sweep_idx=si * 3 + ii, device=dev)
            assert P.route(*p.solver_shape) == ("pinv", "pinv")
            A = _np(inp["A"]).astype(complex)
            PA = np.linalg.pinv(A)
            for kind in ("std", "approximate"):
                S, Y, ce = J.proposed_algorithm(inp["subY"], inp["Omega"], inp["A"], inp["B"], Imax, inp["tau_X"].numpy(),
                                                inp["tau_S"].numpy(), inp["rho"].numpy(), kind)
                Sls = _np(J.ls_estimate(Y, inp["A"], inp["B"]))
                S, Y, ce = _np(S), _np(Y), _np(ce)
                for t in range(4):
                    B = _np(inp["B"][t]).astype(complex)
                    So, Yo, ceo = _oracle(_np(inp["subY"][t]), _np(inp["Omega"][t]), A, B, Imax, float(inp["tau_X"][t]),
                                          float(inp["tau_S"][t]), float(inp["rho"][t]), kind)
                    zb = _np(inp["Zbar"][t])
                    Slo = PA @ Yo @ np.linalg.pinv(B)
                    d = abs(O.nmse_capped(Sls[t].astype(complex), zb) - O.nmse_capped(Slo, zb))
                    dn[kind].append(d)
                    check_below("driver.%s.dnmse" % kind, d, TOL_NMSE)
                    check_below("driver.%s.Y" % kind, rel_err(Y[t], Yo), TOL_STD)
                    check_below("driver.%s.S" % kind, rel_err(S[t], So), TOL_STD)
                    check_below("driver.%s.Sls" % kind, rel_err(Sls[t], Slo), TOL_STD)
                    # (relative to each column's largest entry: the late entries of a converged solve sit at the rounding
                    #  floor of the relative change, where a per-entry ratio measures only noise)
                    for j in range(2):
                        check_below("driver.%s.ce12" % kind, rel_err(ce[t][:, j], ceo[:, j]), TOL_DRIVER_CE)
                    if kind == "std":
                        assert np.all(ce[t][:, 2] == 0)                 # column 3 is only written by 'approximate' (:51)
    for kind, v in dn.items():
        v = np.asarray(v)
        assert len(v) == 84
        check_below("driver.%s.dnmse_rms" % kind, np.sqrt(np.mean(v ** 2)), TOL_NMSE)
        print("driver %-11s |dNMSE| rms %.3g max %.3g over %d trials" % (kind, np.sqrt(np.mean(v ** 2)), v.max(), len(v)))


# ---------------------------------------------------------------------------------------------------- 2. the routes
ROUTES = [  # id, N, M, Gr, G2
    ("ragged", 29, 61, 27, 13),
    ("square", 16, 13, 16, 13),                       # the full-rank boundary N == Gr, M == G2
    ("largest_pinv", 32, P.largest_fitting(16), 32, 16),
    ("smallest_gram", 32, P.largest_fitting(16) + 1, 32, 16),
    ("eig64", 32, P.largest_fitting(64) + 1, 31, 64),
    ("eig63_odd", 24, P.largest_fitting(63) + 2, 17, 63),
    ("eig_square", 20, 100, 20, 100),
    ("ns140", 24, 200, 17, 140),
    ("ns129", 16, 160, 15, 129),
    ("ns_square", 16, 144, 16, 144),
    ("eig_eig", 100, 100, 64, 65),
    ("eig_eig_square", 95, 96, 95, 96),
]


def _problem(rng, b, N, M, Gr, G2, cA=10.0, cB=10.0):
    """A shared (N x Gr), B per trial (b x G2 x M): conditioned factors, a sparse S0, 60 % observed entries, 2 % noise."""
    A = P.factor(rng, N, Gr, cA)
    B0 = P.factor(rng, G2, M, cB)
    # per-trial dictionaries of the same conditioning: B0 with its columns rotated by random phases
    B = np.stack([B0 * np.exp(2j * np.pi * rng.random(M)) for _ in range(b)])
    subY, Om = [], []
    for t in range(b):
        S0 = np.zeros((Gr, G2), complex)
        S0[rng.integers(0, Gr, 6), rng.integers(0, G2, 6)] = rng.standard_normal(6) + 1j * rng.standard_normal(6)
        X = A @ S0 @ B[t]
        om = (rng.random((N, M)) < 0.6).astype(np.float32)
        noise = 0.02 * np.abs(X).max() * (rng.standard_normal((N, M)) + 1j * rng.standard_normal((N, M)))
        subY.append(om * (X + noise)); Om.append(om)
    c64 = lambda x: np.asarray(x).astype(np.complex64)
    return c64(A), c64(B), np.stack(Om), c64(np.stack(subY))


@pytest.mark.parametrize("rid,N,M,Gr,G2", ROUTES, ids=[r[0] for r in ROUTES])
def test_std_route_against_float64_with_every_variant(rid, N, M, Gr, G2):
    import torch
    import jstsp19_amd as J
    from capi_calls import _proposed
    ra, rb = P.route(N, M, Gr, G2)
    name = "route.%s+%s" % (ra, rb)
    rng = np.random.default_rng(N * 7919 + M * 31 + Gr * 7 + G2)
    b, Imax = 3, 6
    A, B, Om, subY = _problem(rng, b, N, M, Gr, G2)

    # the accuracy statement of the route: 6e-8 * cond per factor through the pinv kernel, 6e-8 * cond^2 through a Gram inverse
    scale = EPS * sum(P.cond(F) ** (1 if r == "pinv" else 2) for r, F in ((ra, A), (rb, B[0])))

    def vs_oracle(tag, S, Y, ce, Bt, imax=Imax, indx=None, want_ce=True):
        for t in range(b):
            So, Yo, ceo = _oracle(subY[t], Om[t], A, Bt(t), imax, *PRM, indx=None if indx is None else indx[t], want_ce=want_ce)
            check_below("%s.%s.k" % (name, tag), max(rel_err(S[t], So), rel_err(Y[t], Yo)) / scale, K)
            if want_ce:
                check_below("%s.%s.ce12" % (name, tag), ce_rel(ce[t][:, :2], ceo[:, :2]), TOL_STD_CE)
                assert np.all(ce[t][:, 2] == 0)

    # host, per-trial B, convergence_error
    S, Y, ce = J.proposed_algorithm(subY, Om, A, B, Imax, *PRM, "std")
    vs_oracle("host", S, Y, ce, lambda t: B[t])
    ctx = J.default_context(0)
    rc, res = ctx.last_conditioning()
    worst = max([P.cond(A)] + [P.cond(B[t]) for t in range(b)])
    check_below("%s.rcond_vs_numpy" % name, abs(np.log(rc * worst)), 2e-3)
    # the split-f16 dictionary path off (JSTSP_H2=0: the switches are read at every call)
    os.environ["JSTSP_H2"] = "0"
    try:
        S0, Y0, ce0 = J.proposed_algorithm(subY, Om, A, B, Imax, *PRM, "std")
    finally:
        del os.environ["JSTSP_H2"]
    vs_oracle("h2off", S0, Y0, ce0, lambda t: B[t])
    # device memory, one B for the batch (strideB = 0), indx_S given (proposed_algorithm_angles), no convergence_error
    indx = np.stack([rng.permutation(Gr * G2) + 1 for _ in range(b)]).astype(np.int32)
    Sd, Yd, ced = J.proposed_algorithm_angles(_dev(subY), _dev(Om), torch.from_numpy(indx).cuda(), _dev(A), _dev(B[0]), Imax,
                                              *PRM, "std", want_ce=False)
    assert ced is None
    vs_oracle("device_shared_angles", _np(Sd), _np(Yd), None, lambda t: B[0], indx=indx, want_ce=False)
    # Imax = 1
    S1, Y1, ce1 = J.proposed_algorithm(subY, Om, A, B, 1, *PRM, "std")
    vs_oracle("imax1", S1, Y1, ce1, lambda t: B[t], imax=1)
    # device per-trial; the two-phase form is bit-identical to the one-call form
    Sd2, Yd2, ced2 = J.proposed_algorithm(_dev(subY), _dev(Om), _dev(A), _dev(B), Imax, *PRM, "std")
    vs_oracle("device", _np(Sd2), _np(Yd2), _np(ced2), lambda t: B[t])
    h = J.proposed_algorithm_begin(_dev(subY), _dev(Om), _dev(A), _dev(B), Imax, *PRM, "std")
    Sb, Yb, ceb = h.end()
    assert np.array_equal(_np(Sb), _np(Sd2)) and np.array_equal(_np(Yb), _np(Yd2)) and np.array_equal(_np(ceb), _np(ced2))
    # _c64 on float-representable inputs: bit-identical to _c32
    lib = J.load()
    S64, Y64, ce64 = _proposed(lib, ctx, "c64", A.astype(complex), B.astype(complex), Om.astype(float), subY.astype(complex),
                               Imax, *PRM, 1)
    S32, Y32, ce32 = _proposed(lib, ctx, "c32", A, B, Om, subY, Imax, *PRM, 1)
    assert np.array_equal(S64, S32.astype(complex)) and np.array_equal(Y64, Y32.astype(complex))
    assert np.array_equal(ce64, ce32, equal_nan=True)


BATCH_ROUTES = [r for r in ROUTES if r[0] in ("ragged", "smallest_gram", "ns140", "eig_eig")]


@pytest.mark.parametrize("rid,N,M,Gr,G2", BATCH_ROUTES, ids=[r[0] for r in BATCH_ROUTES])
def test_std_batch_1_and_64_are_bit_identical(rid, N, M, Gr, G2):
    """A trial solved alone and inside a batch of 64 (per-trial dictionaries) gives the same bits: 'std' and jstsp_ls_c32."""
    import jstsp19_amd as J
    rng = np.random.default_rng(G2 * 101 + M)
    A, B, Om, subY = _problem(rng, 64, N, M, Gr, G2)
    S, Y, ce = J.proposed_algorithm(subY, Om, A, B, 4, *PRM, "std")
    for t in (0, 1, 37, 63):
        s1, y1, c1 = J.proposed_algorithm(subY[t:t + 1], Om[t:t + 1], A, B[t:t + 1], 4, *PRM, "std")
        assert np.array_equal(s1[0], S[t]) and np.array_equal(y1[0], Y[t]) and np.array_equal(c1[0], ce[t]), t
    Sl = J.ls_estimate(subY, A, B)
    for t in (0, 63):
        assert np.array_equal(J.ls_estimate(subY[t:t + 1], A, B[t:t + 1])[0], Sl[t]), t


# ---------------------------------------------------------------------------------------------------- 3. conditioning
@pytest.mark.parametrize("rows,cols", [(64, 64), (140, 16), (16, P.largest_fitting(16)), (33, 17), (17, 33)])
def test_pinv_kernel_accuracy_scales_with_cond(rows, cols):
    """The float64 pinv kernel: the result is limited by rounding it to fp32, K * 6e-8 * cond; jstsp_last_conditioning reports
    sigma_min/sigma_max of the complex64 input as numpy computes it."""
    import jstsp19_amd as J
    rng = np.random.default_rng(rows * 1000 + cols)
    for c in (1e1, 1e2, 1e3, 1e4):
        F = P.factor(rng, rows, cols, c).astype(np.complex64)
        Pk = J.pinv(F)
        check_below("cond.pinv.k", rel_err(Pk, np.linalg.pinv(F.astype(complex))) / (EPS * c), K)
        rc, res = J.default_context(0).last_conditioning()
        check_below("cond.pinv.rcond_rel", abs(rc * P.cond(F) - 1.0), 5e-7)
        assert res == 0.0


def _ls_case(rng, N, M, Gr, G2, cA, cB):
    A = P.factor(rng, N, Gr, cA).astype(np.complex64)
    B = P.factor(rng, G2, M, cB).astype(np.complex64)
    Y = (rng.standard_normal((N, M)) + 1j * rng.standard_normal((N, M))).astype(np.complex64)
    ref = np.linalg.pinv(A.astype(complex)) @ Y.astype(complex) @ np.linalg.pinv(B.astype(complex))
    return A, B, Y, ref


def test_ls_and_std_on_the_pinv_route_scale_with_cond():
    import jstsp19_amd as J
    rng = np.random.default_rng(404)
    N, M, Gr, G2 = 32, 70, 32, 16
    assert P.route(N, M, Gr, G2) == ("pinv", "pinv")
    for cA, cB in ((10, 1e3), (1e3, 10), (1e4, 1e4), (1e2, 1e2)):
        A, B, Y, ref = _ls_case(rng, N, M, Gr, G2, cA, cB)
        check_below("cond.ls.pinv+pinv.k", rel_err(J.ls_estimate(Y, A, B), ref) / (EPS * (cA + cB)), K)
        # 'std' on the same factors: the iteration applies both pinvs once per iteration
        Om = (rng.random((N, M)) < 0.6).astype(np.float32)
        S, _, _ = J.proposed_algorithm(Om * Y, Om, A, B, 3, *PRM, "std")
        So, _, _ = _oracle(Om * Y, Om, A, B, 3, *PRM, want_ce=False)
        check_below("cond.std.pinv+pinv.k", rel_err(S, So) / (EPS * (cA + cB)), K)


def _rcond_bound(c):
    """|log(rcond_min * cond)| allowed on a Gram route: the reported ratio is as accurate as the inverse it comes from
    (relative K * 6e-8 * cond^2), over a floor of 2e-3 for the fp32 Gram itself (measured at most 1e-3 at cond 3 ... 30)."""
    return 2e-3 + K * EPS * c * c


def _gram_cases():
    out = []
    for n in (32, 64, 128):                                   # eigen route: B (n x M) too large for the pinv kernel
        out.append((n, max(P.largest_fitting(n) + 1, n + 20)))
    for n in (129, 256, 512):                                 # Newton-Schulz
        out.append((n, n + 24))
    return out


@pytest.mark.parametrize("G2,M", _gram_cases(), ids=["order%d" % n for n, _ in _gram_cases()])
def test_gram_route_meets_its_accuracy_or_refuses(G2, M):
    """jstsp_ls_c32 with B through the fp32 Gram inverse, cond(B) 3 ... 2000 (lambda_min/lambda_max of B B^H 1e-1 ... 2.5e-7),
    across the cut of the eigen route (n * eps32 * lambda_max: 3.8e-6 / 7.6e-6 / 1.5e-5 for n = 32 / 64 / 128) and the refusal
    threshold 1e-6.  A JSTSP_HOST call either returns S within K * 6e-8 * cond^2 of float64 or fails with JSTSP_E_ILLCOND; it
    must fail where the route cannot deliver, and must not where it can.  A JSTSP_DEVICE call reports the same through
    jstsp_last_conditioning."""
    import jstsp19_amd as J
    from jstsp19_amd._lib import E_ILLCOND
    route = P.gram_route(G2)
    N, Gr = 16, 16
    assert P.route(N, M, Gr, G2) == ("pinv", route)
    thr = P.refuse_threshold(G2) if route == "eig" else P.GRAM_REFUSE
    rng = np.random.default_rng(G2)
    ctx = J.default_context(0)
    for c in (3, 30, 100, 300, 500, 700, 1000, 2000):
        ratio = 1.0 / c ** 2
        A, B, Y, ref = _ls_case(rng, N, M, Gr, G2, 1.0, c)
        try:
            S = J.ls_estimate(Y, A, B)
            refused = False
        except J.JstspError as e:
            assert e.code == E_ILLCOND, e
            refused = True
        if not refused:
            check_below("cond.ls.%s.k" % route, rel_err(S, ref) / (EPS * c * c), K)
        if ratio < thr / 1.5:
            assert refused, (G2, c, "returned a Gram inverse below the refusal threshold")
        if ratio > thr * 1.5:
            assert not refused, (G2, c, "refused a Gram inverse above the refusal threshold")
        # device memory: asynchronous, the record says it
        Sd = J.ls_estimate(_dev(Y), _dev(A), _dev(B))
        rc, res = ctx.last_conditioning()
        ok = rc * rc >= 1e-6                                  # the rule of diag_check_host (jstsp.h: jstsp_last_conditioning)
        assert ok == (not refused), (G2, c, rc, res)
        if ok:
            check_below("cond.ls.%s.k" % route, rel_err(_np(Sd), ref) / (EPS * c * c), K)
        if ratio > thr * 1.5:
            check_below("cond.%s.rcond_vs_numpy" % route, abs(np.log(rc * P.cond(B))) / _rcond_bound(c), 1.0)
        if route == "ns" and ok:
            check_below("cond.ns.residual_over_floor", res * rc * rc / EPS, K)


@pytest.mark.parametrize("G2", [256, 512])
@pytest.mark.parametrize("flat", [False, True], ids=["haar", "spread"])
def test_newton_schulz_two_level_spectra_up_to_the_threshold(G2, flat):
    """Newton-Schulz on spectra that are not geometric: half the singular values of B at 1, half at 1 / cond, with Haar or DFT
    left singular vectors - both make ||B B^H||_1 ~ sqrt(n) lambda_max / 2, the slowest start of the iteration.  Every case lies above the refusal threshold (lambda_min/lambda_max >= 1.6e-6): it must be solved, within
    K * 6e-8 * cond^2, and jstsp_last_conditioning must report its conditioning."""
    import jstsp19_amd as J
    N, Gr, M = 16, 16, G2 + 24
    rng = np.random.default_rng(G2 + flat)
    ctx = J.default_context(0)
    for c in (10, 100, 300, 600, 800):
        B = P.factor_two_level(rng, G2, M, c, flat=flat).astype(np.complex64)
        A = P.factor(rng, N, Gr, 1.0).astype(np.complex64)
        Y = (rng.standard_normal((N, M)) + 1j * rng.standard_normal((N, M))).astype(np.complex64)
        ref = np.linalg.pinv(A.astype(complex)) @ Y.astype(complex) @ np.linalg.pinv(B.astype(complex))
        S = J.ls_estimate(Y, A, B)                            # JSTSP_HOST: raises JSTSP_E_ILLCOND if refused
        check_below("cond.ns2.k", rel_err(S, ref) / (EPS * c * c), K)
        rc, res = ctx.last_conditioning()
        check_below("cond.ns2.rcond_vs_numpy", abs(np.log(rc * P.cond(B))) / _rcond_bound(c), 1.0)
        check_below("cond.ns.residual_over_floor", res * rc * rc / EPS, K)


STD_GRAM = [(64, 92, 10), (64, 92, 100), (128, 150, 500), (140, 170, 10), (140, 170, 100), (256, 280, 2000)]


@pytest.mark.parametrize("G2,M,c", STD_GRAM, ids=["%s%d-c%d" % (P.gram_route(n), n, c) for n, _, c in STD_GRAM])
def test_std_gram_route_meets_its_accuracy_or_refuses(G2, M, c):
    """proposed_algorithm 'std' with B through the Gram inverse: the same rule as jstsp_ls_c32.  (cond 500 at order 128:
    lambda_min/lambda_max = 4e-6, inside the band between the refusal threshold 1e-6 and the eigen route's cut 1.5e-5, where
    a JSTSP_HOST call used to return a truncated inverse without an error.)"""
    import jstsp19_amd as J
    from jstsp19_amd._lib import E_ILLCOND
    route = P.gram_route(G2)
    N, Gr = 24, 17
    assert P.route(N, M, Gr, G2) == ("pinv", route)
    rng = np.random.default_rng(G2 * 13 + c)
    A, B, Om, subY = _problem(rng, 2, N, M, Gr, G2, cA=3.0, cB=c)
    thr = P.refuse_threshold(G2) if route == "eig" else P.GRAM_REFUSE
    try:
        S, Y, _ = J.proposed_algorithm(subY, Om, A, B, 4, *PRM, "std")
        refused = False
    except J.JstspError as e:
        assert e.code == E_ILLCOND, e
        refused = True
    if 1.0 / c ** 2 < thr / 1.5:
        assert refused
    else:
        assert not refused
        for t in range(2):
            So, Yo, _ = _oracle(subY[t], Om[t], A, B[t], 4, *PRM, want_ce=False)
            check_below("cond.std.%s.k" % route, max(rel_err(S[t], So), rel_err(Y[t], Yo)) / (EPS * c * c), K)
