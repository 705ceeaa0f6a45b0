"""The problems of tests/std64_problems.py judged on the CPU: the oracle's 'std' branch is finite on each of them, its structured
form (pinv(A) K pinv(B)) agrees with the line-by-line dense-Kronecker restatement (LU of K2, U\\(L\\k)) on P2 - where K2 is
square and the solve exact - and on P1 (K2 is 91 x 45), and the loop that takes the pseudo-inverses as arguments is the oracle's
own.  d_ref, the largest of those differences, is what two float64 statements of Alg. 1 differ by on these problems: the device
bound 1e-10 / 1e-8 has to lie well above it (measured: d_ref = 3.2e-14 on S and Y, 1.1e-12 on convergence_error)."""
import numpy as np

import std64_problems as P


def test_the_oracle_is_finite_on_every_problem_and_the_shapes_are_the_stated_ones():
    shapes = {"P1": (7, 13, 5, 9, 25), "P2": (6, 9, 6, 9, 20), "P3": (16, 40, 12, 24, 20), "P4": (8, 520, 6, 6, 8), "P5": (72, 80, 8, 10, 4),
              "P6": (7, 13, 5, 9, 25)}
    for name in P.NAMES:
        p = P.problem(name)
        N, M = p["subY"].shape[-2:]
        Gr, G2 = p["A"].shape[-1], p["B"].shape[-2]
        assert (N, M, Gr, G2, p["Imax"]) == shapes[name] and N >= Gr and M >= G2
        assert all(p[k].dtype == np.complex128 for k in ("subY", "A", "B"))
        for S, Y, ce in (P.reference(name),) + ((P.reference("P3", True), P.reference("P3", True, *P.P3_SATURATE)) if name == "P3" else ()):
            assert np.all(np.isfinite(S)) and np.all(np.isfinite(Y)) and np.all(np.isfinite(ce[..., :2])) and np.all(ce[..., 2] == 0)
            assert np.max(np.abs(S)) > 0                        # the thresholds leave something to compare
    p = P.problem("P3")
    assert p["subY"].shape[0] == 5 and p["B"].ndim == 3 and p["A"].ndim == 2 and len(set(p["rho"])) == 5
    t, im = P.P3_SATURATE
    assert 10 + 5 * p["Imax"] < 12 * 24 <= 10 + 5 * im           # the mask count saturates only in the long run
    # with the mask saturated, the last iterations of _angles keep every entry the threshold leaves
    assert np.count_nonzero(P.reference("P3", True, t, im)[0]) > np.count_nonzero(P.reference("P3", True)[0][t])
    B, PB, d = P.p6_factor()
    s = np.linalg.svd(B, compute_uv=False)
    assert abs(s[0] / s[-1] / 1e6 - 1) < 1e-6 and np.linalg.norm(B @ PB @ B - B, 2) < 1e-9 * s[0]


def test_structured_and_literal_agree_and_d_ref_is_far_below_the_device_bounds():
    from oracle import solvers as O
    d_ref = d_ce = 0.0
    for name in ("P2", "P1"):
        a = P.args(name)
        Sl, Yl, cel = O.proposed_algorithm_literal(*a, "std")
        S, Y, ce = P.reference(name)
        d_ref = max(d_ref, P.rel_err(S, Sl), P.rel_err(Y, Yl))
        d_ce = max(d_ce, P.ce_spread(ce[:, :2], cel[:, :2]))
    print("std64: d_ref = %.3e (S, Y), %.3e (convergence_error)" % (d_ref, d_ce))
    assert d_ref < P.TOL64_S / 20 and d_ce < P.TOL64_CE / 20


def test_the_loop_with_given_factors_is_the_oracles_and_p6_has_a_bound():
    for name in ("P1", "P6"):
        a = P.args(name)
        out = P.std_loop(*a, np.linalg.pinv(a[2]), np.linalg.pinv(a[3]))
        for x, r in zip(out, P.reference(name)):
            assert np.array_equal(x, r)
    d, dce = P.p6_spread()
    bS, bce = P.p6_bounds()
    print("std64: P6 spread d = %.3e (S, Y), %.3e (convergence_error); bounds %.3e, %.3e" % (d, dce, bS, bce))
    assert np.isfinite(d) and bS == max(1e-10, 100 * d) and bce == max(1e-8, 100 * dce)
    assert bS < 1e-3                                             # (a bound that says nothing would not be worth a test)
