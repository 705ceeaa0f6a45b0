"""jstsp_svd_f64 / jstsp_lowrank_f64 (csrc/svd64.hip) on the GPU: singular triplets and the best rank-R approximation on both
routes - the single-launch LDS kernel (n <= 64 within 160 KiB) and the global-memory Jacobi with the vectors kernel behind it.

Error measures per matrix, s1 = sigma_1 of numpy.linalg.svd (tests/svd64_problems.py): e_sv = max_k |sv_k - ref_k| / s1,
e_rec = ||A - U diag(sv) V^H||_2 / s1, e_long / e_short = max |Q^H Q - I| over the kept columns of the long-side factor / over all
columns of the short-side factor.  Bounds: e_sv <= 9e-14 (LDS route) / 3.6e-13 (global route), the bounds the project asserts for
the same rotations; the other three <= 4 x the worst value the numpy restatement of the algorithm reaches over the same problem
set (svd64_problems.bounds; tests/test_svd64_problems.py holds those against the a-priori ceiling and against numpy's own SVD).
Every measured value is recorded through check_below (profiles/svd64_measured_tolerances.json keeps the device's)."""
import numpy as np
import pytest
import torch

import jstsp19_amd as J
import pinv64_problems as Q
import spectrum_problems as P
import svd64_problems as S
from conftest import check_below
from jstsp19_amd import _lib

pytestmark = pytest.mark.gpu

ALL_SHAPES = S.LDS_SHAPES + S.GLOBAL_SHAPES
LOWRANK_SHAPES = [(32, 140), (128, 50), (7, 13), (96, 300), (200, 97)]
INVARIANCE_SHAPES = [(32, 140), (128, 50), (33, 3), (96, 300), (520, 66), (40, 600)]


def _dev(x):
    return J.colmajor(torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0"))


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _same(a, b):
    """the same bits (NaN patterns included)"""
    a, b = _np(a), _np(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _svd(A, keep=None):
    return tuple(_np(x) for x in J.svd_f64(A, keep, info=True))


@pytest.mark.parametrize("rows,cols", ALL_SHAPES)
def test_triplets_rank_convergence_and_the_bits_shared_with_the_value_entries(rows, cols):
    route, n = S.route_of(rows, cols), min(rows, cols)
    bd = S.bounds(route)
    for name, A in S.classes(rows, cols):
        ref = P.ref(A)
        U, sv, V, rk, cv = _svd(A)
        assert U.shape == (S.BATCH, rows, n) and sv.shape == (S.BATCH, n) and V.shape == (S.BATCH, cols, n)
        assert U.dtype == np.complex128 and sv.dtype == np.float64 and rk.dtype == np.int32 and cv.dtype == np.int32
        assert P.ordered(sv)                                                # descending, non-negative
        w = S.worst([S.measures(A[t], U[t], sv[t], V[t], ref[t]) for t in range(S.BATCH)])
        print("svd_f64 %dx%d %s (%s): " % (rows, cols, name, route) + " ".join("%s %.3g" % kv for kv in sorted(w.items())))
        for k, v in w.items():
            check_below("svd64_%s_%s" % (route, k), v, bd[k])
        # the rank: the drop rule on numpy's values, which first have to be clear of the threshold themselves
        thr = S.drop_threshold(rows, cols, ref[:, 0])[:, None]
        assert not np.any((ref > thr / 4) & (ref < thr * 4)), "a reference value lies within a factor 4 of the drop threshold"
        assert np.array_equal(rk, np.sum(ref > thr, axis=1)), (name, rk)
        for t in range(S.BATCH):                                            # the long-side factor: zero columns from the rank on
            long = U[t] if rows >= cols else V[t]
            assert np.all(long[:, rk[t]:] == 0) and np.all(np.abs(long[:, :rk[t]]).max(axis=0) > 0)
        assert np.array_equal(cv, np.ones(S.BATCH, np.int32)), (name, cv)
        # the bits of the value-only entries that run the same rotations
        if route == "lds" and rows * cols <= 8192:
            assert _same(sv, J.singular_values(A)), name
        if route == "global" and n > 64:
            assert _same(sv, J.spectrum(A)), name
        # the device memspace; a smaller n_keep; outputs not asked for
        Ud, svd, Vd, rkd, cvd = _svd(_dev(A))
        assert _same(Ud, U) and _same(svd, sv) and _same(Vd, V) and _same(rkd, rk) and _same(cvd, cv), name
        keep = max(1, n // 3)
        Uk, svk, Vk, rkk, cvk = _svd(A, keep)
        assert _same(Uk, U[:, :, :keep]) and _same(svk, sv[:, :keep]) and _same(Vk, V[:, :, :keep]) and _same(rkk, rk) and _same(cvk, cv)
        if name == "rank6":                                                 # Wedin: the gap is sigma_6, sigma_7 = 0
            Un = np.linalg.svd(A, full_matrices=False)[0]
            for t in range(S.BATCH):
                d = np.linalg.norm(U[t, :, :6] @ np.conj(U[t, :, :6].T) - Un[t, :, :6] @ np.conj(Un[t, :, :6].T), 2)
                check_below("svd64_%s_rank6_projector_over_bound" % route, d / (8 * bd["e_rec"] * ref[t, 0] / ref[t, 5]), 1.0)


@pytest.mark.parametrize("rows,cols,route", [(5081, 2, "lds"), (2, 5081, "lds"), (5082, 2, "global"), (2, 5082, "global")])
def test_the_last_shape_in_lds_and_the_first_one_beyond(rows, cols, route):
    """n = 2: 5081 rows are the longest columns that fit the LDS kernel (162 808 bytes of its 159 KiB), 5082 go to global memory."""
    assert S.route_of(rows, cols) == route
    bd = S.bounds(route)
    A = P.rand(np.random.default_rng(rows + cols), S.BATCH, rows, cols) * 0.3
    ref = P.ref(A)
    U, sv, V, rk, cv = _svd(A)
    w = S.worst([S.measures(A[t], U[t], sv[t], V[t], ref[t]) for t in range(S.BATCH)])
    print("svd_f64 %dx%d (%s): " % (rows, cols, route) + " ".join("%s %.3g" % kv for kv in sorted(w.items())))
    for k, v in w.items():
        check_below("svd64_%s_%s" % (route, k), v, bd[k])
    assert np.all(rk == 2) and np.all(cv == 1) and P.ordered(sv)
    assert all(_same(x, y) for x, y in zip(_svd(_dev(A)), (U, sv, V, rk, cv)))


@pytest.mark.parametrize("rows,cols", [(32, 140), (200, 97)])
def test_null_outputs_leave_the_others_on_their_bits(rows, cols):
    rng = np.random.default_rng(rows)
    A = np.ascontiguousarray(np.swapaxes(P.rand(rng, 3, rows, cols), 1, 2))          # [t][c][r]: the C ABI's layout
    n = min(rows, cols)
    c = _lib.default_context(0)
    f = c._lib.jstsp_svd_f64

    def run(wantU, wantV, wantI):
        U, sv, V = np.full((3, n, rows), -7.0 + 0j), np.full((3, n), -7.0), np.full((3, n, cols), -7.0 + 0j)
        rk, cv = np.full(3, -7, np.int32), np.full(3, -7, np.int32)
        _lib.check(f(c.handle, rows, cols, 3, A.ctypes.data, n, U.ctypes.data if wantU else None, sv.ctypes.data,
                     V.ctypes.data if wantV else None, rk.ctypes.data if wantI else None, cv.ctypes.data if wantI else None, _lib.HOST),
                   "jstsp_svd_f64")
        return U, sv, V, rk, cv

    full = run(True, True, True)
    assert np.all(full[3] == n) and np.all(full[4] == 1)
    for wantU, wantV, wantI in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        got = run(wantU, wantV, wantI)
        for k, want in enumerate((wantU, True, wantV, wantI, wantI)):
            assert _same(got[k], full[k]) if want else np.all(got[k] == -7), (wantU, wantV, wantI, k)


@pytest.mark.parametrize("rows,cols", LOWRANK_SHAPES)
def test_lowrank_residual_tail_and_rank(rows, cols):
    route, n = S.route_of(rows, cols), min(rows, cols)
    bd = S.bounds(route)
    for name, A in S.classes(rows, cols):
        if name not in ("random", "rank6"):
            continue
        ref = P.ref(A)
        for R in (1, 6, n) if name == "rank6" else (1, n):
            X, tail = J.lowrank_f64(A, R, info=True)
            assert X.shape == A.shape and X.dtype == np.complex128 and tail.shape == (S.BATCH,)
            Xd, taild = J.lowrank_f64(_dev(A), R, info=True)
            assert _same(Xd, X) and _same(taild, tail) and _same(J.lowrank_f64(A[1], R), X[1])
            svx = J.spectrum(X) if R < n else None
            for t in range(S.BATCH):
                s1 = ref[t, 0]
                res = np.linalg.norm(A[t] - X[t], 2)
                want = ref[t, R] if R < n else 0.0
                print("lowrank_f64 %dx%d %s R %d: residual %.3g tail %.3g numpy %.3g" % (rows, cols, name, R, res, tail[t], want))
                check_below("svd64_%s_lowrank_residual_vs_tail_over_bound" % route, abs(res - tail[t]) / (bd["e_rec"] * s1), 1.0)
                check_below("svd64_%s_lowrank_residual_vs_numpy_over_bound" % route, abs(res - want) / (bd["e_rec"] * s1), 1.0)
                if R < n:                                                   # X has rank at most R
                    check_below("svd64_%s_lowrank_value_R_plus_1_over_bound" % route, svx[t, R] / (bd["e_sv"] * s1), 1.0)
            if R == n:
                assert np.array_equal(tail, np.zeros(S.BATCH))


def test_cross_check_with_pinv_f64():
    case = (64, 48, 1e6, None)
    A, _, s = Q.build(case)
    U, sv, V, rk, cv = _svd(A)
    assert rk == 48 and cv == 1
    Psvd = (V / sv) @ np.conj(U.T)
    d = Q.rel2(Psvd, np.asarray(J.pinv_f64(A)))
    print("V diag(1/sv) U^H against pinv_f64, 64x48 cond 1e6: %.3g (bound %.3g)" % (d, Q.device_bound(case)))
    check_below("svd64_pinv_cross_check_over_bound", d / Q.device_bound(case), 1.0)


@pytest.mark.parametrize("rows,cols", INVARIANCE_SHAPES)
def test_isolation_memspace_repeat_and_powers_of_two(rows, cols):
    rng = np.random.default_rng(7 * rows + cols)
    n, tall = min(rows, cols), rows >= cols
    A = P.rand(rng, 5, rows, cols) * 0.3
    alone = [_svd(A[t]) for t in range(5)]
    B = A.copy()
    B[1, rows // 2, cols // 3] = complex(np.nan, 0.0)
    B[3] = 0.0
    U, sv, V, rk, cv = got = _svd(B)
    for t in (0, 2, 4):                                                     # the neighbours keep the bits they have alone
        assert all(_same(got[k][t], alone[t][k]) for k in range(5)), t
    assert np.all(np.isnan(U[1])) and np.all(np.isnan(sv[1])) and np.all(np.isnan(V[1])) and rk[1] == 0 and cv[1] == 0
    long, short = (U[3], V[3]) if tall else (V[3], U[3])
    assert np.all(sv[3] == 0) and not np.any(np.signbit(sv[3])) and rk[3] == 0 and cv[3] == 1
    assert np.all(long == 0) and np.array_equal(short, np.eye(n, dtype=complex))
    assert all(_same(x, y) for x, y in zip(_svd(B), got))                   # a repeated call
    assert all(_same(x, y) for x, y in zip(_svd(_dev(B)), got))             # the device memspace
    X, tail = J.lowrank_f64(B, 1, info=True)
    assert np.all(np.isnan(X[1])) and np.isnan(tail[1]) and np.all(X[3] == 0) and tail[3] == 0
    assert _same(X[0], J.lowrank_f64(A[0], 1)) and _same(X[4], J.lowrank_f64(A[4], 1))
    base = _svd(A)
    for k in (40, -40):
        Uk, svk, Vk, rkk, cvk = _svd(A * 2.0 ** k)
        assert _same(Uk, base[0]) and _same(Vk, base[2]) and _same(svk, base[1] * 2.0 ** k) and _same(rkk, base[3]) and _same(cvk, base[4]), k


def test_narrow_and_real_inputs_are_widened():
    rng = np.random.default_rng(2)
    A = P.rand(rng, 2, 13, 7).astype(np.complex64)
    assert all(_same(x, y) for x, y in zip(_svd(A), _svd(A.astype(np.complex128))))
    Ar = rng.standard_normal((7, 13))
    U, sv, V = J.svd_f64(Ar)
    assert U.shape == (7, 7) and sv.shape == (7,) and V.shape == (13, 7)
    check_below("svd64_lds_e_rec", np.linalg.norm(Ar - (U * sv) @ np.conj(V.T), 2) / sv[0], S.bounds("lds")["e_rec"])


def test_error_codes():
    c = _lib.default_context(0)
    buf = np.zeros(16)
    f, g = c._lib.jstsp_svd_f64, c._lib.jstsp_lowrank_f64
    p = buf.ctypes.data
    svd = lambda rows, cols, batch, keep, A=p, sv=p, mem=_lib.HOST: f(c.handle, rows, cols, batch, A, keep, None, sv, None, None, None, mem)
    low = lambda rows, cols, batch, R, A=p, X=p, mem=_lib.HOST: g(c.handle, rows, cols, batch, A, R, X, None, mem)
    for call in (svd, low):
        assert call(513, 513, 1, 1) == -3                                   # n = 513
        assert call(2, 8193, 1, 1) == -3 and call(8193, 2, 1, 1) == -3      # a long side of 8193
        assert call(96, 300, 65536, 1) == -3                                # the global route takes batch <= 65535
        assert call(2, 3, 1, 0) == -4 and call(2, 3, 1, 3) == -4            # n_keep / R outside 1..n
        assert call(2, 3, 1, 1, A=None) == -1
        assert call(0, 3, 1, 1) == -2 and call(2, -1, 1, 1) == -2 and call(2, 3, 0, 1) == -2
        assert call(2, 3, 1, 1, mem=5) == -4
    assert svd(2, 3, 1, 1, sv=None) == -1 and low(2, 3, 1, 1, X=None) == -1
    assert f(None, 2, 3, 1, p, 1, None, p, None, None, None, _lib.HOST) == -1
    assert f(c.handle, 512, 8192, 65535, p, 1, None, p, None, None, None, _lib.DEVICE) == -3        # a workspace above 24 GiB
    assert b"largest batch that fits" in c._lib.jstsp_last_error()
    assert np.all(buf == 0)
    for bad in (lambda: J.svd_f64(np.zeros((513, 513))), lambda: J.lowrank_f64(np.zeros((2, 8193)), 1)):
        with pytest.raises(J.JstspError) as e:
            bad()
        assert e.value.code == -3
    with pytest.raises(ValueError):
        J.svd_f64(torch.zeros(3, 3, dtype=torch.complex128))
