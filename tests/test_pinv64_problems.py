"""CPU checks of tests/pinv64_problems.py - that the accuracy test of jstsp_pinv_f64 (tests/test_gpu_pinv64.py) can fail:

1. numpy's SVD-based pinv stays inside 4 * cond * 2^-53 of the exact pseudo-inverse on every case, so the device bound
   8 * max(d_numpy, cond * 2^-53) is never looser than a small multiple of what a backward-stable SVD route achieves;
2. the float64 Gram route (solve(A'A, A') / its wide counterpart) lies OUTSIDE that bound on every case with cond >= 1e5:
   an implementation that forms a Gram matrix fails the GPU test;
3. the drop rule is not decided by rounding: every singular value numpy finds is at least 1e3 times the threshold
   max(rows, cols) * eps(sigma_max) or at most 1e-1 times it.
Plus the public surface without a GPU: the two names exist, fail loudly, and refuse bad shapes before any device work."""
import numpy as np
import pytest

import pinv64_problems as Q
from conftest import check_below

import jstsp19_amd as J


@pytest.mark.parametrize("case", Q.CASES, ids=Q.case_id)
def test_numpy_is_inside_and_the_gram_route_outside_the_device_bound(case):
    rows, cols, cond, rank = case
    A, P, s = Q.build(case)
    d_ref = Q.numpy_error(case)
    print("%s: numpy %.3g = %.3g x cond 2^-53" % (Q.case_id(case), d_ref, d_ref / (cond * Q.EPS53)))
    check_below("pinv64_problems/numpy_over_cond_eps", d_ref / (cond * Q.EPS53), 4.0)
    if cond >= 1e5:
        try:
            d_gram = Q.rel2(Q.gram_pinv(A), P)
        except np.linalg.LinAlgError:
            d_gram = np.inf                     # (a rank-deficient Gram matrix may be refused outright)
        if not np.isfinite(d_gram):
            d_gram = 1e300
        print("   Gram route %.3g = %.3g x cond 2^-53, device bound %.3g" % (d_gram, d_gram / (cond * Q.EPS53), Q.device_bound(case)))
        check_below("pinv64_problems/bound_over_gram_error", Q.device_bound(case) / d_gram, 1.0)


def _separation(A):
    sv = np.linalg.svd(A, compute_uv=False)
    thr = Q.drop_threshold(A.shape[0], A.shape[1], sv[0])
    kept, dropped = sv[sv > thr], sv[sv <= thr]
    return (float(kept.min() / thr) if kept.size else np.inf), (float(dropped.max() / thr) if dropped.size else 0.0), int(kept.size)


@pytest.mark.parametrize("case", Q.CASES, ids=Q.case_id)
def test_the_drop_rule_is_not_decided_by_rounding(case):
    A, _, s = Q.build(case)
    lo, hi, kept = _separation(A)
    print("%s: kept >= %.3g x threshold, dropped <= %.3g x threshold" % (Q.case_id(case), lo, hi))
    check_below("pinv64_problems/threshold_over_smallest_kept", 1.0 / lo, 1e-3)
    check_below("pinv64_problems/largest_dropped_over_threshold", hi, 1e-1)
    check_below("pinv64_problems/rank_mismatch", abs(kept - len(s)), 0.5)


def test_the_repeated_column_and_the_batch_are_separated_too():
    A = Q.repeated_column()
    lo, hi, kept = _separation(A)
    check_below("pinv64_problems/threshold_over_smallest_kept", 1.0 / lo, 1e-3)
    check_below("pinv64_problems/largest_dropped_over_threshold", hi, 1e-1)
    check_below("pinv64_problems/rank_mismatch", abs(kept - (A.shape[1] - 1)), 0.5)
    Ab, Pb, conds, ranks = Q.batch_of_five()
    for t in range(5):
        lo, hi, kept = _separation(Ab[t])
        check_below("pinv64_problems/threshold_over_smallest_kept", 1.0 / lo, 1e-3)
        check_below("pinv64_problems/largest_dropped_over_threshold", hi, 1e-1)
        check_below("pinv64_problems/rank_mismatch", abs(kept - ranks[t]), 0.5)
        check_below("pinv64_problems/numpy_over_cond_eps", Q.rel2(Q.numpy_pinv(Ab[t]), Pb[t]) / (conds[t] * Q.EPS53), 4.0)


def test_the_exact_pseudo_inverse_satisfies_penrose():
    A, P, _ = Q.build((140, 16, 1e5, None))
    for i, r in enumerate(Q.penrose(A, P)):
        check_below("pinv64_problems/exact_penrose_%d" % (i + 1), r, 1e5 * 64 * Q.EPS53)


def test_the_two_names_are_exported_and_fail_loudly_without_a_gpu():
    from jstsp19_amd import _lib, solvers
    for n in ("pinv_f64", "ls_estimate_f64"):
        assert callable(getattr(J, n)) and n in solvers.__all__
    lib = J.load()
    for n in ("jstsp_pinv_f64", "jstsp_ls_f64"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    with pytest.raises(ValueError):
        J.ls_estimate_f64(np.zeros((4, 6), complex), np.zeros((5, 3), complex), np.zeros((5, 6), complex))
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(J.JstspError):
            J.pinv_f64(np.eye(3, dtype=complex))
        with pytest.raises(J.JstspError):
            J.ls_estimate_f64(np.zeros((4, 6), complex), np.zeros((4, 3), complex), np.zeros((5, 6), complex))


def test_ls_precision_is_validated_before_any_device_work():
    from jstsp19_amd import montecarlo as mc
    with pytest.raises(ValueError):
        mc.run_points([], 1, ls_precision="f16", device="cpu", builder=lambda *a: None)
    import inspect
    assert inspect.signature(mc.run_points).parameters["ls_precision"].default == "f32"
    assert inspect.signature(mc._hip_baselines).parameters["ls_precision"].default == "f32"
