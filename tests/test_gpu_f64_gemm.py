"""The batched complex float64 GEMM on the f64 matrix pipe (csrc/zgemm64.hip) through its two kernel-level entries,
jstsp_correlate_f64 (A' K B') and jstsp_synthesize_f64 (A S B), against numpy complex128.

The tolerance is derived, not measured: entrywise |C - C_ref| <= 8 (k1 + k2 + 8) 2^-53 (|A| |S| |B|) (resp. |A'| |K| |B'|), k1, k2
the two inner dimensions - twice the standard forward bound of a chained complex product in any summation order (the
constant 4 >= 2 sqrt(2) covers the complex multiplication; twice, because numpy's result carries the same bound).  The
right-hand side is computed from the absolute-value matrices.  Measured on MI355X: at most 0.7 % of the bound."""
import numpy as np
import pytest

from conftest import check_below  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(7, 13, 5, 9), (32, 140, 32, 16), (64, 4096, 64, 512)]
BATCH = 3


def _rand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _operands(shape, shared_a, shared_b, seed):
    N, M, Gr, G2 = shape
    rng = np.random.default_rng(seed)
    A = _rand(rng, N, Gr) if shared_a else _rand(rng, BATCH, N, Gr)
    B = _rand(rng, G2, M) if shared_b else _rand(rng, BATCH, G2, M)
    return A, B, _rand(rng, BATCH, N, M), _rand(rng, BATCH, Gr, G2)


def _ct(x):
    return np.conj(np.swapaxes(x, -1, -2))


def _bound_ratio(C, ref, bound):
    """largest |C - ref| / bound over the entries (the bound is positive for these operands)"""
    return float(np.max(np.abs(C - ref) / bound))


def _call(fn, X, A, B, device):
    if not device:
        return fn(X, A, B)
    import torch
    import jstsp19_amd as J
    dev = torch.device("cuda:0")
    cm = lambda a: J.colmajor(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    out = fn(cm(X), cm(A), cm(B))
    torch.cuda.synchronize()
    assert out.dtype == torch.complex128
    return out.cpu().numpy()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("shared_a,shared_b", [(False, False), (True, True), (True, False)], ids=["per_trial", "shared", "shared_A"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_correlate_and_synthesize_within_the_forward_bound(shape, shared_a, shared_b, device):
    import jstsp19_amd as J
    N, M, Gr, G2 = shape
    A, B, K, S = _operands(shape, shared_a, shared_b, 11)
    u = 2.0 ** -53
    # synthesize: (N x Gr)(Gr x G2)(G2 x M), inner dimensions Gr and G2
    ref = A @ S @ B
    bound = 8 * (Gr + G2 + 8) * u * (np.abs(A) @ np.abs(S) @ np.abs(B))
    C = _call(J.synthesize_f64, S, A, B, device)
    assert C.shape == ref.shape and C.dtype == np.complex128
    check_below("f64_gemm.synthesize/bound", _bound_ratio(C, ref, bound), 1.0)
    # correlate: (Gr x N)(N x M)(M x G2), inner dimensions N and M
    ref = _ct(A) @ K @ _ct(B)
    bound = 8 * (N + M + 8) * u * (np.abs(_ct(A)) @ np.abs(K) @ np.abs(_ct(B)))
    C = _call(J.correlate_f64, K, A, B, device)
    assert C.shape == ref.shape and C.dtype == np.complex128
    check_below("f64_gemm.correlate/bound", _bound_ratio(C, ref, bound), 1.0)


def test_asymmetric_integer_operands_are_exact():
    """Small integers: every product and sum is exact in float64, so a wrong lane map (a row of the result tile in another
    row, real and imaginary planes exchanged, a missed conjugation) shows as a non-zero difference."""
    import jstsp19_amd as J
    rng = np.random.default_rng(5)
    N, M, Gr, G2 = 37, 150, 21, 70
    ri = lambda *s: rng.integers(-3, 4, s).astype(float) + 1j * rng.integers(-3, 4, s).astype(float)
    A, B, K, S = ri(N, Gr), ri(2, G2, M), ri(2, N, M), ri(2, Gr, G2)
    assert np.array_equal(J.synthesize_f64(S, A, B), A @ S @ B)
    assert np.array_equal(J.correlate_f64(K, A, B), _ct(A) @ K @ _ct(B))


def test_an_inf_poisons_only_the_entries_it_reaches():
    import jstsp19_amd as J
    shape = (32, 140, 32, 16)
    A, B, K, S = _operands(shape, True, True, 3)
    clean_s, clean_c = J.synthesize_f64(S, A, B), J.correlate_f64(K, A, B)
    # one entry of S: column 7 of A S, then - B is dense - every entry of A S B of that trial, and nothing of the other trials
    S2 = S.copy()
    S2[1, 4, 7] = np.inf
    C = J.synthesize_f64(S2, A, B)
    np.testing.assert_array_equal(C[[0, 2]], clean_s[[0, 2]])
    assert not np.any(np.isfinite(C[1]))
    # one entry of K: likewise for A' K B'
    K2 = K.copy()
    K2[2, 3, 9] = np.inf
    C = J.correlate_f64(K2, A, B)
    np.testing.assert_array_equal(C[:2], clean_c[:2])
    assert not np.any(np.isfinite(C[2]))
    # one entry of a per-trial dictionary: row 5 of A reaches row 5 of A S B only
    A3 = np.stack([A, A, A])
    A3[0, 5, 2] = np.inf
    C = J.synthesize_f64(S, A3, B)
    assert not np.any(np.isfinite(C[0, 5]))
    np.testing.assert_array_equal(np.delete(C[0], 5, axis=0), np.delete(clean_s[0], 5, axis=0))
    np.testing.assert_array_equal(C[1:], clean_s[1:])


@pytest.mark.parametrize("shape", [(7, 13, 5, 9), (64, 4096, 64, 512)], ids=lambda s: "x".join(map(str, s)))
def test_results_do_not_depend_on_the_batch_size_and_repeat_bitwise(shape):
    import jstsp19_amd as J
    A, B, K, S = _operands(shape, True, False, 23)
    full = J.correlate_f64(K, A, B)
    np.testing.assert_array_equal(full, J.correlate_f64(K, A, B))
    np.testing.assert_array_equal(full[1], J.correlate_f64(K[1], A, B[1]))
    np.testing.assert_array_equal(full[:2], J.correlate_f64(K[:2], A, B[:2]))
    fs = J.synthesize_f64(S, A, B)
    np.testing.assert_array_equal(fs[2], J.synthesize_f64(S[2], A, B[2]))


def test_complex64_inputs_are_widened_exactly_and_bad_shapes_raise():
    import jstsp19_amd as J
    A, B, K, S = _operands((7, 13, 5, 9), True, True, 2)
    A32, B32, S32 = A.astype(np.complex64), B.astype(np.complex64), S.astype(np.complex64)
    np.testing.assert_array_equal(J.synthesize_f64(S32, A32, B32),
                                  J.synthesize_f64(S32.astype(np.complex128), A32.astype(np.complex128), B32.astype(np.complex128)))
    with pytest.raises(ValueError):
        J.synthesize_f64(S, A[:, :-1], B)
    with pytest.raises(ValueError):
        J.correlate_f64(K, A[:-1], B)
