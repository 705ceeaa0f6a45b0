"""The cases of tests/score32_problems.py checked without a GPU: every route label is covered, the labelled split-k counts are the
stated ones, and for every generated case the float64 reference alone satisfies what tests/test_gpu_score32.py relies on."""
import numpy as np

import score32_problems as P


def test_every_route_label_occurs_and_the_split_counts_are_the_stated_ones():
    assert set(P.NMSE_SHAPES) | set(P.RATE_SHAPES) == set(P.SHAPES) and len(set(P.SHAPES)) == len(P.SHAPES)
    nm = [P.route(R, C, b) for (R, C, b, _) in P.cases()]
    rt = [P.route(R, C, b) for (R, C, b, _) in P.cases() if P.has_rate(R, C)]
    assert {r[0] for r in nm} == {"ZZh", "ZhZ"} == {r[0] for r in rt}
    assert {r[2] for r in nm} == {"h32", "h64", "h128", "block"} and {r[2] for r in rt} == {"h32", "h64", "h128"}
    assert {r[3] for r in rt} == {"lds", "hbm"} and {r[3] for r in nm} == {"lds", "hbm", "n/a"}
    assert {r[1] for r in nm} == {1, 2, 16} == {r[1] for r in rt}
    assert {(r[1], r[3]) for r in rt} >= {(1, "lds"), (2, "lds"), (1, "hbm"), (2, "hbm")}       # the eigen-kernels sum partials too
    for shape, b, ns in (((64, 512), 3, 2), ((512, 64), 3, 2), ((64, 512), 40, 2), ((33, 4097), 3, 16), ((64, 64), 3, 1), ((128, 600), 3, 2),
                         ((129, 140), 3, 1), ((260, 257), 3, 1)):
        assert P.route(*shape, b)[1] == ns, (shape, b)
    assert 4097 % 16 != 0                                                             # the splits are not equal: a k-tail
    # one shape per lambda_max route runs at batches 1, 3 and 300; the labels of the table are the routes taken
    for shape, lab in P.MANY.items():
        assert shape in P.SHAPES and all(P.route(*shape, b)[2] == lab for b in (1, 3, 300))
    for table in (P.NMSE_SHAPES, P.RATE_SHAPES):
        assert {lab for s, lab in P.MANY.items() if s in table} == {P.route(*s, 3)[2] for s in table}
    assert [P.route(*s, 3)[2] for s in P.ONE_PER_ROUTE] == ["h32", "h64", "h128", "block"]
    assert [P.route(*s, 3)[2:] for s in P.RATE_ROUTES] == [("h32", "lds"), ("h64", "lds"), ("h128", "lds"), ("h128", "hbm")]
    assert P.STRIDING[0][0] * P.STRIDING[0][1] * P.STRIDING[1] > 4096 * 256           # more entries than one pass of the grid


def test_the_eigenvector_boundary_and_the_orders_beside_each_kernel_threshold():
    assert [n for n in range(1, 129) if P.eig_needs_global_v(n) != P.eig_needs_global_v(n + 1)] == [100]
    assert not P.eig_needs_global_v(100) and P.eig_needs_global_v(101)
    assert (100, 100) in P.RATE_SHAPES and (101, 101) in P.RATE_SHAPES
    orders = {min(s) for s in P.NMSE_SHAPES}
    assert {1, 32, 33, 64, 65, 128, 129} <= orders and any(o % 2 for o in orders if o > 129)
    assert {P.route(*s, 3)[2] for s in ((32, 16), (33, 40))} == {"h32", "h64"}
    assert {P.route(*s, 3)[2] for s in ((64, 64), (65, 65))} == {"h64", "h128"}
    assert {P.route(*s, 3)[2] for s in ((128, 130), (129, 140))} == {"h128", "block"}
    assert P.route(130, 64, 3)[2:] == ("h64", "lds") and P.route(12, 40, 3)[0] == "ZZh" and P.route(40, 12, 3)[0] == "ZhZ"


def test_the_reference_alone_meets_the_conditions_of_the_nmse_cases():
    for (R, C, b, g) in P.cases():
        S, Z, e, _ = P.case(R, C, b, g)
        assert S.shape == Z.shape == (b, R, C) and e.shape == (b,) and np.all(np.isfinite(e)), (R, C, b, g)
        assert np.array_equal(S.astype(np.complex64).astype(np.complex128), S)        # the values the device sees
        if g == 0:
            assert np.any(e == 1.0) and (b == 1 or np.any(e < 1.0)), (R, C, b, g)     # capped trials, and uncapped ones beside them
            assert np.all(e > 1e-10)
        else:
            assert np.all(e > 1e-10) and np.all(e < 1.0), (R, C, b, g, e.min(), e.max())


def test_the_reference_alone_meets_the_conditions_of_the_rate_cases():
    for (R, C, b, g) in P.cases():
        if not P.has_rate(R, C):
            continue
        S, Z, e, r = P.case(R, C, b, g, True)
        assert r.shape == (b,) and np.all(np.isfinite(r)) and np.all(r > 1e-3), (R, C, b, g)
        if b <= 3:                                                                    # the closed form, with the uncapped e
            want = P.ref_rate_sigma(S, Z, P.NOISE_VAR)
            assert np.all(np.abs(r - want) <= 1e-12 * np.abs(want)), (R, C, b, g)


def test_the_low_rank_zbar_has_four_singular_values_and_a_floor_of_1e_minus_3():
    for (R, C) in ((64, 64), (101, 101), (128, 600)):
        _, Z = P.operands(R, C, 3, "lowrank")
        sig = np.linalg.svd(Z[0], compute_uv=False)
        assert sig[3] > 0.05 * sig[0] and sig[4] < 5e-3 * sig[0] and sig[-1] > 0


def test_scaled_operands_are_exact_and_their_reference_is_the_unscaled_one():
    for (R, C) in P.ONE_PER_ROUTE:
        S, Z, e, _ = P.case(R, C, 3, 4)
        for s in P.SCALES:
            assert np.array_equal(P.ref_nmse(P.scaled(S, s), P.scaled(Z, s)), e), (R, C, s)     # a power of two: the same bits
    for (R, C) in P.RATE_ROUTES + [(128, 600)]:
        S, Z, _, _ = P.case(R, C, 3, 2, True)
        for s in P.RATE_SCALES:
            Ss, Zs = P.scaled(S, s), P.scaled(Z, s)
            r = P.ref_rate_sigma(Ss, Zs, P.NOISE_VAR)
            # above 1e-6 the sum of log2(1 + x) keeps its digits (log1p-accurate terms are not needed: x > 1e-9 per term)
            assert np.all(np.isfinite(r)) and np.all(r > 1e-6), (R, C, s, r)
            with np.errstate(all="ignore"):
                d = P.ref_rate(Ss, Zs, P.NOISE_VAR)                                    # the determinant, where it is finite
            # (R > C: I + c Zbar Zbar' has R - C unit eigenvalues beside C of the order 2^(2 s) - at 2^20 the LU behind det loses them
            #  to 1e-6 relative, measured on 32 x 16; the sum over singular values does not)
            fin = np.isfinite(d) & (R <= C or s < 0)
            assert np.all(np.abs(d[fin] - r[fin]) <= 1e-12 * np.maximum(np.abs(r[fin]), 1.0)), (R, C, s)
    assert not np.all(np.isfinite(d))                                                 # (128 x 600 at 2^40: why the closed form is used)
