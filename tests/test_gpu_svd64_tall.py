"""jstsp_svd_tall_f64 / jstsp_lowrank_tall_f64 (csrc/svd64.hip, the QR route) on the GPU: singular triplets and the best rank-R
approximation for n = min(rows, cols) <= 64 and a long side up to 65536.

Shapes (svd64_tall_problems.SHAPES): the smallest at which each branch can go wrong - one ragged chunk (5x3, 3x5, 1x7, 7x1), exactly
one chunk of 128 (128x48), one plus 2 rows (130x48), chunk 64 with two full chunks plus 1 row (129x49), n = 64 (64x64, 200x64,
64x200), the shapes jstsp_svd_f64 refuses (8193x2, 2x8193), many chunks with a ragged last one (9000x33) - with batch 3 per problem
class (random, rank 6, sigma graded over 12 decades, repeated sigma), and one matrix of 64 x 65536.

Measures per matrix against numpy.linalg.svd on the same values, s1 = its sigma_1 (tests/svd64_problems.measures):
e_sv = max_k |sv_k - ref_k| / s1 <= 1.1e-13 (QR_TOL of tests/test_gpu_spectrum.py for this reduction); sv within 2 x 1.1e-13 s1 of
jstsp_spectrum_c64 on the same operand; e_rec = ||A - U diag(sv) V^H||_2 / s1, e_long / e_short = max |Q^H Q - I| over the kept
columns of the long-side factor / all columns of the short-side one, each <= 4 x the worst value of the numpy restatement of the
route (tests/golden/svd64_tall_restatement_worst.json); e_rec also within 4 x the restatement's worst over the problems in which the
drop rule drops no value (all but the graded class at 9000x33, whose sigma_33 = 1e-12 sigma_1 lies under the threshold and is
the recorded worst e_rec).  Every measured value goes through check_below
(profiles/svd64_tall_measured_tolerances.json keeps the device's)."""
import numpy as np
import pytest
import torch

import jstsp19_amd as J
import spectrum_problems as P
import svd64_problems as S
import svd64_tall_problems as T
from conftest import check_below
from jstsp19_amd import _lib

pytestmark = pytest.mark.gpu


def _dev(x):
    return J.colmajor(torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0"))


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _same(a, b):
    """the same bits (NaN patterns included)"""
    a, b = _np(a), _np(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _svd(A, keep=None):
    return tuple(_np(x) for x in J.svd_tall_f64(A, keep, info=True))


def _measure(tag, A, U, sv, V, ref):
    bd = T.bounds()
    w = S.worst([S.measures(A[t], U[t], sv[t], V[t], ref[t]) for t in range(A.shape[0])])
    print("svd_tall_f64 %s: " % tag + " ".join("%s %.3g" % kv for kv in sorted(w.items())))
    for k, v in w.items():
        check_below("svd64_tall_%s" % k, v, bd[k])
    if not T.drops_a_value(A.shape[1], A.shape[2], ref):
        check_below("svd64_tall_e_rec_nothing_dropped", w["e_rec"], bd["e_rec_nothing_dropped"])
    spec = _np(J.spectrum(A))
    d = float(np.max(np.abs(sv - spec) / ref[:, :1]))
    print("svd_tall_f64 %s: sv against spectrum %.3g%s" % (tag, d, " (the same bits)" if _same(sv, spec) else ""))
    check_below("svd64_tall_sv_vs_spectrum", d, 2 * T.QR_TOL)


def _rank_by_the_rule(rows, cols, ref):
    """the drop rule on numpy's values, which first have to be clear of the threshold themselves (svd64_tall_problems.CLEAR)"""
    thr = S.drop_threshold(rows, cols, ref[:, 0])[:, None]
    assert not np.any((ref > thr / T.CLEAR) & (ref < thr * T.CLEAR)), "a reference value lies within a factor %g of the drop threshold" % T.CLEAR
    return np.sum(ref > thr, axis=1)


@pytest.mark.parametrize("rows,cols", T.SHAPES)
def test_triplets_rank_and_convergence(rows, cols):
    n = min(rows, cols)
    for name, A in T.classes(rows, cols):
        ref = P.ref(A)
        U, sv, V, rk, cv = _svd(A)
        assert U.shape == (T.BATCH, rows, n) and sv.shape == (T.BATCH, n) and V.shape == (T.BATCH, cols, n)
        assert U.dtype == np.complex128 and sv.dtype == np.float64 and rk.dtype == np.int32 and cv.dtype == np.int32
        assert P.ordered(sv)
        _measure("%dx%d %s" % (rows, cols, name), A, U, sv, V, ref)
        assert np.array_equal(rk, _rank_by_the_rule(rows, cols, ref)), (name, rk)
        if (rows, cols, name) == (9000, 33, "rank6"):
            assert np.all(rk == 6)
        for t in range(T.BATCH):                                            # the long-side factor: zero columns from the rank on
            long = U[t] if rows >= cols else V[t]
            assert np.all(long[:, rk[t]:] == 0) and np.all(np.abs(long[:, :rk[t]]).max(axis=0) > 0)
        assert np.array_equal(cv, np.ones(T.BATCH, np.int32)), (name, cv)
        # a smaller n_keep: the leading values and short-side columns on the bits; the long-side columns to rounding level only,
        # because the correction L (I + E^H E / 2) couples the columns that are kept
        keep = max(1, n // 3)
        Uk, svk, Vk, rkk, cvk = _svd(A, keep)
        longk, shortk, long, short = (Uk, Vk, U, V) if rows >= cols else (Vk, Uk, V, U)
        assert _same(svk, sv[:, :keep]) and _same(shortk, short[:, :, :keep]) and _same(rkk, rk) and _same(cvk, cv)
        assert longk.shape == long[:, :, :keep].shape
        check_below("svd64_tall_long_side_n_keep_against_full", np.max(np.abs(longk - long[:, :, :keep])), T.bounds()["e_long"])


def test_one_matrix_of_64_by_65536():
    A = T.big_problem()
    ref = P.ref(A)
    U, sv, V, rk, cv = _svd(_dev(A))
    assert U.shape == (1, 64, 64) and V.shape == (1, 65536, 64) and P.ordered(sv)
    _measure("64x65536 random", A, U, sv, V, ref)
    assert rk[0] == 64 == _rank_by_the_rule(64, 65536, ref)[0] and cv[0] == 1


@pytest.mark.parametrize("rows,cols", [(9000, 33), (64, 200)])
def test_lowrank_residual_and_tail(rows, cols):
    n, bd = min(rows, cols), T.bounds()
    for name, A in T.classes(rows, cols):
        if name not in ("random", "rank6"):
            continue
        ref = P.ref(A)
        assert not T.drops_a_value(rows, cols, ref)
        for R in (1, 6, n):
            X, tail = J.lowrank_tall_f64(A, R, info=True)
            assert X.shape == A.shape and X.dtype == np.complex128 and tail.shape == (T.BATCH,)
            Xd, taild = J.lowrank_tall_f64(_dev(A), R, info=True)
            assert _same(Xd, X) and _same(taild, tail) and _same(J.lowrank_tall_f64(A[1], R), X[1])
            for t in range(T.BATCH):
                s1 = ref[t, 0]
                res = np.linalg.norm(A[t] - X[t], 2)
                want = ref[t, R] if R < n else 0.0
                print("lowrank_tall_f64 %dx%d %s R %d: residual %.3g tail %.3g numpy %.3g" % (rows, cols, name, R, res, tail[t], want))
                # (random and rank 6 drop no value that is not zero: the bound that watches the arithmetic)
                check_below("svd64_tall_lowrank_residual_vs_tail_over_bound", abs(res - tail[t]) / (bd["e_rec_nothing_dropped"] * s1), 1.0)
                check_below("svd64_tall_lowrank_residual_vs_numpy_over_bound", abs(res - want) / (bd["e_rec_nothing_dropped"] * s1), 1.0)
            if R == n:
                assert np.array_equal(tail, np.zeros(T.BATCH))


@pytest.mark.parametrize("rows,cols", [(64, 64), (200, 64)])
def test_product_agrees_with_svd_f64(rows, cols):
    """U diag(sv) V^H of the two entries within the sum of both residual bounds (no class drops a value at these shapes: the
    bound that watches the arithmetic); the vectors are not compared."""
    bound = T.bounds()["e_rec_nothing_dropped"] + S.bounds(S.route_of(rows, cols))["e_rec"]
    for name, A in T.classes(rows, cols):
        ref = P.ref(A)
        assert not T.drops_a_value(rows, cols, ref)
        U, sv, V = (_np(x) for x in J.svd_tall_f64(A))
        U0, sv0, V0 = (_np(x) for x in J.svd_f64(A))
        for t in range(T.BATCH):
            d = np.linalg.norm((U[t] * sv[t]) @ np.conj(V[t].T) - (U0[t] * sv0[t]) @ np.conj(V0[t].T), 2) / ref[t, 0]
            check_below("svd64_tall_product_vs_svd_f64_over_bound", d / bound, 1.0)


@pytest.mark.parametrize("rows,cols", [(130, 48), (64, 200), (9000, 33)])
def test_isolation_memspace_repeat_powers_of_two_and_the_zero_matrix(rows, cols):
    rng = np.random.default_rng(11 * rows + cols)
    n, tall = min(rows, cols), rows >= cols
    A = P.rand(rng, 3, rows, cols) * 0.3
    B = A.copy()
    B[1, rows // 2, cols // 3] = complex(np.nan, 0.0)
    clean = [_svd(A[[0, 2]]), _svd(B)]
    for k in range(5):                                                      # the neighbours of the NaN matrix: the bits of a call without it
        assert _same(clean[1][k][[0, 2]], clean[0][k]), k
    U, sv, V, rk, cv = clean[1]
    assert np.all(np.isnan(U[1])) and np.all(np.isnan(sv[1])) and np.all(np.isnan(V[1])) and rk[1] == 0 and cv[1] == 0
    assert all(_same(x, y) for x, y in zip(_svd(B), clean[1]))              # a repeated call
    assert all(_same(x, y) for x, y in zip(_svd(_dev(B)), clean[1]))        # the device memspace
    X, tail = J.lowrank_tall_f64(B, 1, info=True)
    assert np.all(np.isnan(X[1])) and np.isnan(tail[1]) and _same(X[0], J.lowrank_tall_f64(A[0], 1)) and _same(X[2], J.lowrank_tall_f64(A[2], 1))
    base = _svd(A)
    for k in (70, -70):
        Uk, svk, Vk, rkk, cvk = _svd(A * 2.0 ** k)
        assert _same(Uk, base[0]) and _same(Vk, base[2]) and _same(svk, base[1] * 2.0 ** k) and _same(rkk, base[3]) and _same(cvk, base[4]), k
    Z = A.copy()
    Z[1] = 0.0
    U, sv, V, rk, cv = _svd(Z)
    long, short = (U[1], V[1]) if tall else (V[1], U[1])
    assert np.all(sv[1] == 0) and not np.any(np.signbit(sv[1])) and rk[1] == 0 and cv[1] == 1
    assert np.all(long == 0) and np.array_equal(short, np.eye(n, dtype=complex))
    assert _same(U[0], base[0][0]) and _same(V[2], base[2][2])
    Xz = J.lowrank_tall_f64(Z, 1)
    assert np.all(Xz[1] == 0)


def test_null_outputs_leave_the_others_on_their_bits():
    rows, cols = 130, 48
    A = np.ascontiguousarray(np.swapaxes(P.rand(np.random.default_rng(5), 3, rows, cols), 1, 2))      # [t][c][r]: the C ABI's layout
    n = min(rows, cols)
    c = _lib.default_context(0)
    f = c._lib.jstsp_svd_tall_f64

    def run(wantU, wantV, wantI):
        U, sv, V = np.full((3, n, rows), -7.0 + 0j), np.full((3, n), -7.0), np.full((3, n, cols), -7.0 + 0j)
        rk, cv = np.full(3, -7, np.int32), np.full(3, -7, np.int32)
        _lib.check(f(c.handle, rows, cols, 3, A.ctypes.data, n, U.ctypes.data if wantU else None, sv.ctypes.data,
                     V.ctypes.data if wantV else None, rk.ctypes.data if wantI else None, cv.ctypes.data if wantI else None, _lib.HOST),
                   "jstsp_svd_tall_f64")
        return U, sv, V, rk, cv

    full = run(True, True, True)
    assert np.all(full[3] == n) and np.all(full[4] == 1)
    for wantU, wantV, wantI in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        got = run(wantU, wantV, wantI)
        for k, want in enumerate((wantU, True, wantV, wantI, wantI)):
            assert _same(got[k], full[k]) if want else np.all(got[k] == -7), (wantU, wantV, wantI, k)


def test_narrow_and_real_inputs_are_widened():
    rng = np.random.default_rng(2)
    A = P.rand(rng, 2, 13, 7).astype(np.complex64)
    assert all(_same(x, y) for x, y in zip(_svd(A), _svd(A.astype(np.complex128))))
    Ar = rng.standard_normal((7, 13))
    U, sv, V = J.svd_tall_f64(Ar)
    assert U.shape == (7, 7) and sv.shape == (7,) and V.shape == (13, 7)
    check_below("svd64_tall_e_rec", np.linalg.norm(Ar - (U * sv) @ np.conj(V.T), 2) / sv[0], T.bounds()["e_rec"])


def test_error_codes():
    c = _lib.default_context(0)
    buf = np.zeros(16)
    f, g = c._lib.jstsp_svd_tall_f64, c._lib.jstsp_lowrank_tall_f64
    p = buf.ctypes.data
    svd = lambda rows, cols, batch, keep, A=p, sv=p, mem=_lib.HOST: f(c.handle, rows, cols, batch, A, keep, None, sv, None, None, None, mem)
    low = lambda rows, cols, batch, R, A=p, X=p, mem=_lib.HOST: g(c.handle, rows, cols, batch, A, R, X, None, mem)
    for call in (svd, low):
        assert call(65, 9000, 1, 1) == -3 and call(9000, 65, 1, 1) == -3   # n = 65
        assert b"65536" in c._lib.jstsp_last_error() and b"64" in c._lib.jstsp_last_error()
        assert call(64, 65537, 1, 1) == -3 and call(65537, 64, 1, 1) == -3  # a long side of 65537
        assert call(2, 3, 1, 0) == -4 and call(2, 3, 1, 3) == -4            # n_keep / R outside 1..n
        assert call(2, 3, 1, 1, A=None) == -1
        assert call(0, 3, 1, 1) == -2 and call(2, -1, 1, 1) == -2 and call(2, 3, 0, 1) == -2
        assert call(2, 3, 1, 1, mem=5) == -4
        assert call(64, 65536, 400, 1, mem=_lib.DEVICE) == -3               # a workspace above 24 GiB: pointers it never reads
        assert b"largest batch that fits" in c._lib.jstsp_last_error()
    assert svd(2, 3, 1, 1, sv=None) == -1 and low(2, 3, 1, 1, X=None) == -1
    assert f(None, 2, 3, 1, p, 1, None, p, None, None, None, _lib.HOST) == -1
    assert low(2, 3, 65536, 1, mem=_lib.DEVICE) == -3
    assert np.all(buf == 0)
    for bad in (lambda: J.svd_tall_f64(np.zeros((65, 65))), lambda: J.lowrank_tall_f64(np.zeros((2, 65537)), 1)):
        with pytest.raises(J.JstspError) as e:
            bad()
        assert e.value.code == -3
    with pytest.raises(ValueError):
        J.svd_tall_f64(torch.zeros(3, 3, dtype=torch.complex128))
