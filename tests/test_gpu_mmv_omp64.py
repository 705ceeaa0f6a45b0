"""Joint (MMV) OMP in float64, jstsp_mmv_omp_f64 (csrc/mmv_omp64.hip), on the problems of tests/mmv64_problems.py: the 32
engineered rows of the fp32 kernel's test (every split of the row scores, the three stop rules, exact ties, Y = 0, scaled
inputs) plus the rows that only float64 decides (M8: a selection with a relative gap of 1e-9 .. 1e-8) and Y * 2^+-100, 2^+-400.

Each problem is solved alone through the C ABI in host memory, for both row scores: count and support must equal the float64
oracle's wherever every gap is >= 1e-9 or exactly 0, and Z must meet it to 1e-12 of max|Z_ref| - cond(A[:, support]) <= 100
times 2^-53 times about 90 for dot products of up to 300 terms; the numpy restatement of the algorithm stays below 1e-14
(tests/test_mmv64_problems.py).  The same assertions on every row from device memory, and through the Python wrapper with
complex64 and complex128 numpy arrays and torch CUDA tensors (complex64 where the row's values are complex64).  Then the same bits
inside batches at several positions (shared and own dictionaries, strideA = N Gr and N Gr + 7), without
index_out / count_out, on a repeated call, and beside a problem whose Y holds a NaN or an Inf."""
import ctypes as C

import numpy as np
import pytest

import mmv64_problems as Q
import mmv_problems as P
from conftest import check_below, rel_err

pytestmark = pytest.mark.gpu

HOST, DEVICE = 0, 1
PNORM = {"l2": 2, "l1": 1}
_ALONE = {}
_FURTHER = []                       # rows that needed the "one atom further" clause


def _lib_ctx():
    import jstsp19_amd as J
    return J.load(), J.default_context(0)


def _pack(rows, strideA, shared):
    """column-major complex128 staging of a batch of same-shape rows; the padding between dictionaries is NaN."""
    N, Gr = rows[0]["A"].shape
    S = rows[0]["Y"].shape[1]
    assert all(r["A"].shape == (N, Gr) and r["Y"].shape == (N, S) for r in rows)
    if shared:
        assert all(np.array_equal(r["A"], rows[0]["A"]) for r in rows)
        a, strideA = np.ascontiguousarray(rows[0]["A"].T, np.complex128).reshape(-1), 0
    else:
        strideA = N * Gr if strideA is None else strideA
        a = np.full((len(rows) - 1) * strideA + N * Gr, np.nan + 1j * np.nan, np.complex128)
        for t, r in enumerate(rows):
            a[t * strideA:t * strideA + N * Gr] = r["A"].T.reshape(-1)
    y = np.ascontiguousarray(np.stack([r["Y"].T for r in rows]), np.complex128).reshape(-1)
    return a, y, strideA


def solve(rows, norm, memspace=HOST, strideA=None, shared=False, K=None, want_idx=True, want_cnt=True, expect=0):
    """one jstsp_mmv_omp_f64 call on a batch of rows: (Z (b, Gr, S), idx (b, K) or None, cnt (b,) or None)."""
    lib, ctx = _lib_ctx()
    b = len(rows)
    N, Gr = rows[0]["A"].shape
    S = rows[0]["Y"].shape[1]
    K = rows[0]["K"] if K is None else K
    a, y, strideA = _pack(rows, strideA, shared)
    if memspace == DEVICE:
        import torch
        ctx.use_torch_stream()
        dev = torch.device("cuda:0")
        ta, ty = torch.from_numpy(a).to(dev), torch.from_numpy(y).to(dev)
        tz = torch.full((b * Gr * S,), float("nan"), dtype=torch.complex128, device=dev)
        ti = torch.full((b * K,), -7, dtype=torch.int32, device=dev) if want_idx else None
        tc = torch.full((b,), -7, dtype=torch.int32, device=dev) if want_cnt else None
        rc = lib.jstsp_mmv_omp_f64(ctx.handle, N, Gr, S, b, ta.data_ptr(), strideA, ty.data_ptr(), K, PNORM[norm], tz.data_ptr(),
                                   ti.data_ptr() if want_idx else None, tc.data_ptr() if want_cnt else None, DEVICE)
        torch.cuda.synchronize()
        z, idx, cnt = tz.cpu().numpy(), ti.cpu().numpy() if want_idx else None, tc.cpu().numpy() if want_cnt else None
    else:
        z = np.full(b * Gr * S, np.nan + 1j * np.nan, np.complex128)
        idx = np.full(b * K, -7, np.int32) if want_idx else None
        cnt = np.full(b, -7, np.int32) if want_cnt else None
        p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
        rc = lib.jstsp_mmv_omp_f64(ctx.handle, N, Gr, S, b, p(a), strideA, p(y), K, PNORM[norm], p(z), p(idx), p(cnt), HOST)
    assert rc == expect, (rc, lib.jstsp_last_error())
    Z = np.transpose(z.reshape(b, S, Gr), (0, 2, 1))
    return Z, (idx.reshape(b, K) if want_idx else None), cnt


def alone(row, norm):
    key = (row["name"], norm)
    if key not in _ALONE:
        Z, idx, cnt = solve([row], norm)
        _ALONE[key] = (Z[0].copy(), idx[0].copy(), int(cnt[0]))
    return _ALONE[key]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_row(row, norm, Z, idx, cnt):
    ref, tag = row["ref"][norm], (row["name"], norm)
    assert 0 <= cnt <= min(row["K"], *row["A"].shape), tag
    assert np.all(idx[cnt:] == 0) and np.all(np.isfinite(Z)), tag
    assert Q.decisive(row, norm), tag                             # every row of the set is decisive at 1e-9 or an exact tie
    s = ref["count"]
    if cnt != s and row["kind"] == "M4":
        # the c32 contract's clause: a residual within rounding of rule (3) may take the device one atom further
        _, _, ratio = Q.restate(row["A"], row["Y"], row["K"], norm)
        assert cnt == s + 1 and np.array_equal(idx[:s], ref["sup"]) and abs(ratio - 1e-12) < 1e-13, (tag, cnt, s, ratio)
        _FURTHER.append(tag)
    else:
        assert cnt == s and np.array_equal(idx[:cnt], ref["sup"]), (tag, cnt, idx.tolist(), ref["sup"].tolist())
    err = rel_err(Z, ref["Z"])
    print("%-18s %s count %d rel_err(Z) %.3g" % (row["name"], norm, cnt, err))
    if row["kind"] == "M6":
        assert cnt == 1 and idx[0] == 1 and not Z.any(), tag
    elif row["kind"] == "M3":
        assert np.array_equal(Z, row["Z_exact"]), tag
    elif row["kind"] in ("M2", "M5") and "j" in row:
        assert idx[0] == row["j"] + 1 and all(idx[0] < c + 1 for c in row["copies"]), tag
    elif row["kind"] == "M5" and "p" in row:
        assert idx[0] == row["p"] + 1 < row["q"] + 1, tag
    check_below("mmv64.%s.Z" % row["kind"], err, Q.TOL_Z)


@pytest.mark.parametrize("norm", Q.NORMS)
def test_every_problem_alone(norm):
    red = []
    for row in Q.problems()["rows"]:                              # every row is checked: the report names all that fail
        try:
            check_row(row, norm, *alone(row, norm))
        except AssertionError as e:
            red.append((row["name"], str(e)[:300]))
    assert not red, red
    m4 = sum(r["kind"] == "M4" for r in Q.problems()["rows"])
    print("rows that needed the one-atom-further clause: %s" % _FURTHER)
    assert len([t for t in _FURTHER if t[1] == norm]) <= m4


def test_scaled_problems_return_the_unscaled_bits_times_the_factor():
    """M7 (Y * 2^k rows) and M9: supports and counts of the unscaled problem, Z = Z_unscaled * 2^k on the bits."""
    for norm in Q.NORMS:
        for r in (r for r in Q.problems()["rows"] if "scale_y" in r):
            Z0, i0, c0 = alone(Q.by_name(r["base"]), norm)
            Z, idx, cnt = alone(r, norm)
            k = r["scale_y"]
            assert cnt == c0 and np.array_equal(idx, i0), (r["name"], norm, idx.tolist(), i0.tolist())
            back = np.ldexp(Z.real, -k) + 1j * np.ldexp(Z.imag, -k)
            assert same_bits(back, Z0), (r["name"], norm, rel_err(back, Z0))


def _batches():
    pr = Q.problems()
    first = pr["rows"][0]["name"]
    ys = ["M7y%+d" % k for k in P.Y_SCALES] + ["M9y%+d" % k for k in Q.Y64_SCALES]
    return [dict(names=pr["mixed"], shared=False, strideA=None),
            dict(names=pr["own"] + [first], shared=False, strideA=None),
            dict(names=pr["own"] + [first], shared=False, strideA=32 * 32 + 7),
            dict(names=[first] + ys + pr["shared"], shared=True, strideA=None)]


def test_a_problem_returns_the_same_bits_alone_at_any_batch_position_and_on_a_repeated_call():
    for norm in Q.NORMS:
        for B in _batches():
            for names in (B["names"], B["names"][::-1]):
                rows = [Q.by_name(n) for n in names]
                Z, idx, cnt = solve(rows, norm, strideA=B["strideA"], shared=B["shared"])
                for t, r in enumerate(rows):
                    Za, ia, ca = alone(r, norm)
                    assert cnt[t] == ca and np.array_equal(idx[t], ia) and same_bits(Z[t], Za), (norm, names, t)
            rows = [Q.by_name(n) for n in B["names"]]
            first = solve(rows, norm, strideA=B["strideA"], shared=B["shared"])
            solve([Q.by_name("M1_64x257x300_K8")], norm)         # another shape through the same workspace in between
            again = solve(rows, norm, strideA=B["strideA"], shared=B["shared"])
            assert all(same_bits(x, y) for x, y in zip(first, again)), (norm, B["names"])


def test_device_memory_null_outputs_and_k_beyond_the_atoms_return_the_host_bits():
    cases = [([Q.by_name(n) for n in B["names"]], B["strideA"], B["shared"], None) for B in _batches()]
    for name, K in (("M1_300x513x3_K9", None), ("M1_16x4096x5_K6", None), ("M1_8x1x4_K3", None), ("M1_1x5x3_K2", None), ("M3", 40),
                    ("M1_32x32x16_K6", 100), ("M8", None)):
        cases.append(([Q.by_name(name)], None, False, K))
    for norm in Q.NORMS:
        for rows, strideA, shared, K in cases:
            kw = dict(strideA=strideA, shared=shared, K=K)
            Zh, ih, ch = solve(rows, norm, HOST, **kw)
            Zd, idd, cd = solve(rows, norm, DEVICE, **kw)
            tag = (norm, [r["name"] for r in rows], K)
            assert same_bits(Zh, Zd) and np.array_equal(ih, idd) and np.array_equal(ch, cd), tag
            for t in range(len(rows)):
                assert 0 <= ch[t] <= min(ih.shape[1], *rows[t]["A"].shape), tag
                assert np.all(ih[t, :ch[t]] > 0) and np.all(ih[t, ch[t]:] == 0), (tag, ih[t].tolist())
            if K is None:
                for t, r in enumerate(rows):
                    assert same_bits(Zh[t], alone(r, norm)[0]), tag
            for mem, wi, wc in ((HOST, False, False), (DEVICE, False, False), (HOST, True, False), (DEVICE, False, True)):
                Z, idx, cnt = solve(rows, norm, mem, want_idx=wi, want_cnt=wc, **kw)
                assert same_bits(Z, Zh) and (idx is None or np.array_equal(idx, ih)) and (cnt is None or np.array_equal(cnt, ch)), (tag, mem)
    r = Q.by_name("M1_32x32x16_K6")
    Z, idx, cnt = solve([r], "l2", K=100)
    assert cnt[0] == 32 and sorted(idx[0, :32].tolist()) == list(range(1, 33))
    A64 = r["A"].astype(complex)                                  # all 32 atoms of a square A: Z = A \\ Y, to 100 cond(A) 2^-53
    check_below("mmv64.all_atoms.Z_over_cond_eps", rel_err(Z[0], np.linalg.solve(A64, r["Y"].astype(complex))) / (np.linalg.cond(A64) * 2.0 ** -53),
                100.0)


@pytest.mark.parametrize("norm", Q.NORMS)
def test_every_problem_from_device_memory(norm):
    """every row through the C ABI with JSTSP_DEVICE: the oracle assertions of ``check_row``, and the bits of the host solve."""
    red = []
    for row in Q.problems()["rows"]:
        try:
            Z, idx, cnt = solve([row], norm, DEVICE)
            check_row(row, norm, Z[0], idx[0], int(cnt[0]))
            Za, ia, ca = alone(row, norm)
            assert same_bits(Z[0], Za) and np.array_equal(idx[0], ia) and cnt[0] == ca, (row["name"], norm, "device bits")
        except AssertionError as e:
            red.append((row["name"], str(e)[:300]))
    assert not red, red


def _input_types(row):
    """complex128 for every row; complex64 as well where the row's values ARE complex64 (M1-M7: the reused rows).  The M8 and M9
    rows exist only in complex128 - rounded to complex64 an M8 row is another problem (its close pair ties) and Y 2^+-400 has no
    complex64 value."""
    return (np.complex64, np.complex128) if row["A"].dtype == np.complex64 else (np.complex128,)


@pytest.mark.parametrize("norm", Q.NORMS)
def test_every_problem_through_the_wrapper_complex64_and_complex128_numpy_and_torch(norm):
    """every row through ``mmv_omp_f64`` with numpy arrays (host memspace) and torch CUDA tensors (device memspace), as complex64
    and as complex128: the oracle assertions of ``check_row`` on each of the four, and the bits of the C-ABI solve."""
    import torch
    import jstsp19_amd as J
    dev = torch.device("cuda:0")
    red = []
    for row in Q.problems()["rows"]:
        Za, ia, ca = alone(row, norm)
        for dt in _input_types(row):
            A, Y = row["A"].astype(dt), row["Y"].astype(dt)
            assert np.array_equal(A.astype(np.complex128), row["A"]) and np.array_equal(Y.astype(np.complex128), row["Y"])
            try:
                Z, idx, cnt = J.mmv_omp_f64(A, Y, row["K"], norm=norm)
                assert Z.dtype == np.complex128 and idx.dtype == np.int32
                check_row(row, norm, Z, idx, int(cnt))
                assert same_bits(Z, Za) and np.array_equal(idx, ia) and cnt == ca, (row["name"], norm, dt, "numpy bits")
                tA, tY = (J.colmajor(torch.from_numpy(x).to(dev)) for x in (A, Y))
                Zt, it, ct = J.mmv_omp_f64(tA, tY, row["K"], norm=norm)
                torch.cuda.synchronize()
                assert Zt.dtype == torch.complex128 and Zt.is_cuda
                check_row(row, norm, Zt.cpu().numpy(), it.cpu().numpy(), int(ct))
                assert same_bits(Zt.cpu().numpy(), Za) and np.array_equal(it.cpu().numpy(), ia) and int(ct) == ca, (row["name"], norm, dt, "torch bits")
            except AssertionError as e:
                red.append((row["name"], str(dt), str(e)[:300]))
    assert not red, red


def test_a_nan_or_inf_in_one_problem_leaves_its_batch_mates_alone():
    names = Q.problems()["mixed"]
    for norm in Q.NORMS:
        for victim, bad in ((0, np.nan), (2, np.nan), (len(names) - 1, np.inf), (2, complex(0.0, -np.inf))):
            rows = [dict(Q.by_name(n)) for n in names]
            Y = rows[victim]["Y"].copy()
            Y[3, 1] = bad
            rows[victim]["Y"] = Y
            Z, idx, cnt = solve(rows, norm)                      # status 0 is asserted in solve
            for t, n in enumerate(names):
                if t == victim:
                    assert 0 <= cnt[t] <= rows[t]["K"], (norm, victim, cnt[t])
                    assert np.all(idx[t, cnt[t]:] == 0) and np.all((idx[t, :cnt[t]] >= 1) & (idx[t, :cnt[t]] <= 48))
                else:
                    Za, ia, ca = alone(Q.by_name(n), norm)
                    assert cnt[t] == ca and np.array_equal(idx[t], ia) and same_bits(Z[t], Za), (norm, victim, n)


def test_bad_arguments_come_back_as_error_codes():
    lib, ctx = _lib_ctx()
    N, S, K = 4, 2, 2
    p = lambda x: x.ctypes.data_as(C.c_void_p)

    def call(Gr, pnorm, strideA, batch=2, null_y=False):
        a = np.zeros((batch * max(strideA, N * Gr),), np.complex128)
        y, z = np.zeros(batch * N * S, np.complex128), np.zeros(batch * Gr * S, np.complex128)
        return lib.jstsp_mmv_omp_f64(ctx.handle, N, Gr, S, batch, p(a), strideA, None if null_y else p(y), K, pnorm, p(z), None, None, HOST)

    assert call(8, 2, 0) == 0 and call(8, 1, 32) == 0 and call(4096, 2, 0, batch=1) == 0
    assert call(4097, 2, 0) == -3                                  # JSTSP_E_UNSUPPORTED
    assert call(8, 3, 0) == -4                                     # JSTSP_E_ARG
    assert call(8, 2, 31) == -2                                    # JSTSP_E_SHAPE: strideA < N Gr
    assert call(8, 2, 0, null_y=True) == -1                        # JSTSP_E_NULL
