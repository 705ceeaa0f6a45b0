"""Joint (MMV) OMP, jstsp_mmv_omp_c32 (csrc/mmv_omp.hip), on every path of its kernel with the engineered problems of
tests/mmv_problems.py: every split of the row scores (1 to 256 column groups, one or several atom passes with idle lanes in
the last), block-strided loops (N > 256, S > 256), the three stop rules (residual, dependent atom, all atoms in), exact ties,
Y = 0, and inputs scaled by powers of two far outside the range where a squared correlation fits an fp32.

Each problem is solved alone through the C ABI in host memory, for both row scores; support and count must equal the float64
reference on the same complex64 values, and Z must meet it to 1e-4 (exactly for the axis-aligned and zero problems).  Then:
the same bits inside a mixed batch at two positions, on a shared and on per-problem dictionaries (strideA = N Gr and
N Gr + 7), from device memory, without index_out / count_out, with K > min(N, Gr), on a repeated call, and beside a problem
whose Y holds a NaN or an Inf.

Measured on MI355X (profiles/mmv_measured_tolerances.json, mmv_paths.*): the largest Z error is 1.7e-7 (the noisy random rows,
M1; 6.4e-8 on the random noiseless rows, M4), the scaled problems' Z carries the bits of the unscaled one, and the device count
of the random noiseless rows equalled the reference's in 4 of 4 solves (2 rows, both row scores)."""
import ctypes as C

import numpy as np
import pytest

import mmv_problems as P
from conftest import check_below, load_golden, rel_err

pytestmark = pytest.mark.gpu

HOST, DEVICE = 0, 1
PNORM = {"l2": 2, "l1": 1}
TOL_Z = 1e-4                  # the bound of the well-conditioned joint-OMP problems of tests/test_gpu_baselines.py
_ALONE = {}
_M4_COUNTS = []


def _lib_ctx():
    import jstsp19_amd as J
    return J.load(), J.default_context(0)


def _pack(rows, strideA, shared):
    """column-major staging of a batch of same-shape rows: (A buffer, Y buffer, strideA); padding between dictionaries
    is NaN, so a kernel that read it would not pass."""
    N, Gr = rows[0]["A"].shape
    S = rows[0]["Y"].shape[1]
    assert all(r["A"].shape == (N, Gr) and r["Y"].shape == (N, S) and r["K"] == rows[0]["K"] for r in rows)
    if shared:
        assert all(np.array_equal(r["A"], rows[0]["A"]) for r in rows)
        a, strideA = np.ascontiguousarray(rows[0]["A"].T).reshape(-1), 0
    else:
        strideA = N * Gr if strideA is None else strideA
        a = np.full((len(rows) - 1) * strideA + N * Gr, np.nan + 1j * np.nan, np.complex64)
        for t, r in enumerate(rows):
            a[t * strideA:t * strideA + N * Gr] = r["A"].T.reshape(-1)
    y = np.ascontiguousarray(np.stack([r["Y"].T for r in rows])).reshape(-1)
    return a, y, strideA


def solve(rows, norm, memspace=HOST, strideA=None, shared=False, K=None, want_idx=True, want_cnt=True, expect=0):
    """one jstsp_mmv_omp_c32 call on a batch of rows: (Z (b, Gr, S), idx (b, K) or None, cnt (b,) or None)."""
    from jstsp19_amd import _lib
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
        tz = torch.full((b * Gr * S,), float("nan"), dtype=torch.complex64, device=dev)
        ti = torch.full((b * K,), -7, dtype=torch.int32, device=dev) if want_idx else None
        tc = torch.full((b,), -7, dtype=torch.int32, device=dev) if want_cnt else None
        rc = lib.jstsp_mmv_omp_c32(ctx.handle, N, Gr, S, b, ta.data_ptr(), strideA, ty.data_ptr(), K, PNORM[norm], tz.data_ptr(),
                                   ti.data_ptr() if want_idx else None, tc.data_ptr() if want_cnt else None, DEVICE)
        torch.cuda.synchronize()
        z, idx, cnt = tz.cpu().numpy(), ti.cpu().numpy() if want_idx else None, tc.cpu().numpy() if want_cnt else None
    else:
        z = np.full(b * Gr * S, np.nan + 1j * np.nan, np.complex64)
        idx = np.full(b * K, -7, np.int32) if want_idx else None
        cnt = np.full(b, -7, np.int32) if want_cnt else None
        p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
        rc = lib.jstsp_mmv_omp_c32(ctx.handle, N, Gr, S, b, p(a), strideA, p(y), K, PNORM[norm], p(z), p(idx), p(cnt), HOST)
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
    K = row["K"]
    assert 0 <= cnt <= min(K, *row["A"].shape), tag
    assert np.all(idx[cnt:] == 0) and np.all(np.isfinite(Z)), tag
    print("%-18s %s count %d (reference %d) support %s" % (row["name"], norm, cnt, ref["count"], idx[:cnt].tolist()))
    if row["kind"] == "M4":
        # fp32 residual 10-100x under the stop threshold: the count may exceed the reference's, the selections may not differ
        s = ref["count"]
        _M4_COUNTS.append(cnt == s)
        assert cnt >= s and np.array_equal(idx[:s], ref["sup"]), (tag, idx.tolist(), ref["sup"].tolist())
    else:
        assert cnt == ref["count"] and np.array_equal(idx[:cnt], ref["sup"]), (tag, cnt, idx.tolist(), ref["sup"].tolist())
    err = rel_err(Z, ref["Z"])
    print("%-18s %s rel_err(Z) %.3g" % (row["name"], norm, err))
    if row["kind"] == "M6":
        assert not Z.any(), tag
    elif row["kind"] == "M3":
        assert np.array_equal(Z, row["Z_exact"]), tag
    check_below("mmv_paths.%s.Z" % row["kind"], err, TOL_Z)


@pytest.mark.parametrize("norm", P.NORMS)
def test_every_engineered_problem_alone(norm):
    red = []
    for row in P.problems()["rows"]:                             # every row is checked: the report names all that fail
        try:
            check_row(row, norm, *alone(row, norm))
        except AssertionError as e:
            red.append((row["name"], str(e)[:300]))
    assert not red, red
    m4 = [r for r in P.problems()["rows"] if r["kind"] == "M4"]
    print("M4 count equal to the reference: %d of %d solves (%s)" % (sum(_M4_COUNTS[-len(m4):]), len(m4), norm))


def test_scaled_problems_return_the_unscaled_bits_times_the_factor():
    """M7: a power of two is exact.  Y * 2^k: the kernel's normalisation hands the iteration the bits of the unscaled
    problem, so support and count are equal and Z is the unscaled Z times 2^k bit for bit (asserted on the bits).  A * 2^k
    is not normalised: the same support and count, Z within 1e-6 of the unscaled Z times 2^-k."""
    rows = P.problems()["rows"]
    for norm in P.NORMS:
        for r in (r for r in rows if r["kind"] == "M7"):
            Z0, i0, c0 = alone(P.by_name(r["base"]), norm)
            Z, idx, cnt = alone(r, norm)
            k = r.get("scale_y", 0) - r.get("scale_a", 0)
            assert cnt == c0 and np.array_equal(idx, i0), (r["name"], norm, idx.tolist(), i0.tolist())
            err = rel_err(Z.astype(complex) * 2.0 ** -k, Z0.astype(complex))
            print("%-18s %s rel_err(Z 2^%d, Z unscaled) %.3g" % (r["name"], norm, -k, err))
            if "scale_y" in r:
                back = np.ldexp(Z.real, -k) + 1j * np.ldexp(Z.imag, -k)        # float32 in, float32 out: exact here
                assert back.dtype == Z0.dtype and same_bits(back, Z0), (r["name"], norm, err)
            check_below("mmv_paths.scale.Z", err, 1e-6)


def _batches():
    pr = P.problems()
    row = P.by_name
    first = pr["rows"][0]["name"]
    ys = ["M7y%+d" % k for k in P.Y_SCALES]
    return [dict(names=pr["mixed"], shared=False, strideA=None),
            dict(names=pr["own"] + [first] + ["M7a%+d" % k for k in P.A_SCALES], shared=False, strideA=None),
            dict(names=pr["own"] + [first], shared=False, strideA=32 * 32 + 7),
            dict(names=[first] + ys + pr["shared"], shared=True, strideA=None)], row


def test_a_problem_returns_the_same_bits_alone_and_at_any_batch_position():
    batches, row = _batches()
    for norm in P.NORMS:
        for B in batches:
            for names in (B["names"], B["names"][::-1], B["names"][1:] + B["names"][:1]):
                rows = [row(n) for n in names]
                Z, idx, cnt = solve(rows, norm, strideA=B["strideA"], shared=B["shared"])
                for t, r in enumerate(rows):
                    Za, ia, ca = alone(r, norm)
                    assert cnt[t] == ca and np.array_equal(idx[t], ia) and same_bits(Z[t], Za), (norm, names, t)
                    check_row(r, norm, Z[t], idx[t], int(cnt[t]))


def test_device_memory_null_outputs_and_k_beyond_the_atoms_return_the_host_bits():
    batches, row = _batches()
    cases = [([row(n) for n in B["names"]], B["strideA"], B["shared"], None) for B in batches]
    for name, K in (("M1_64x300x40_K10", None), ("M1_300x513x3_K9", None), ("M1_64x257x300_K8", None),
                    ("M1_8x1x4_K3", None), ("M1_1x5x3_K2", None), ("M3", 40), ("M1_32x32x16_K6", 100)):
        cases.append(([row(name)], None, False, K))               # K = 3 > min(8, 1), 2 > min(1, 5), 40 > 24, 100 > 32
    for norm in P.NORMS:
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
            for mem in (HOST, DEVICE):
                for wi, wc in ((False, False), (True, False), (False, True)):
                    Z, idx, cnt = solve(rows, norm, mem, want_idx=wi, want_cnt=wc, **kw)
                    assert same_bits(Z, Zh) and (idx is None or np.array_equal(idx, ih)) and \
                        (cnt is None or np.array_equal(cnt, ch)), (tag, mem, wi, wc)
    # K beyond the atoms of a square full-rank dictionary: every atom enters, and the engineered stops still hold
    r = row("M1_32x32x16_K6")
    Z, idx, cnt = solve([r], "l2", K=100)
    assert cnt[0] == 32 and sorted(idx[0, :32].tolist()) == list(range(1, 33))
    Z, idx, cnt = solve([row("M3")], "l2", K=40)
    assert cnt[0] == row("M3")["s"] and np.array_equal(Z[0], row("M3")["Z_exact"])


def test_a_repeated_call_returns_the_same_bits():
    batches, row = _batches()
    for norm in P.NORMS:
        for names in (batches[0]["names"], ["M1_128x128x140_K12"], ["M1_16x4096x5_K6"]):
            rows = [row(n) for n in names]
            first = solve(rows, norm)
            solve([row("M1_64x257x300_K8")], norm)               # another shape through the same workspace in between
            again = solve(rows, norm)
            assert all(same_bits(x, y) for x, y in zip(first, again)), (norm, names)


def test_a_nan_in_one_problem_leaves_its_batch_mates_alone():
    """a NaN, +Inf or -Inf component in one problem's Y."""
    _, row = _batches()
    names = P.problems()["mixed"]
    for norm in P.NORMS:
        for victim, bad in ((0, np.nan), (2, np.nan), (len(names) - 1, np.nan), (0, np.inf), (2, complex(0.0, -np.inf)),
                            (len(names) - 1, np.inf)):
            rows = [dict(row(n)) for n in names]
            Y = rows[victim]["Y"].copy()
            Y[3, 1] = bad
            assert not np.isfinite(Y[3, 1]) and np.isfinite(np.delete(Y.reshape(-1), 3 * Y.shape[1] + 1)).all()
            rows[victim]["Y"] = Y
            Z, idx, cnt = solve(rows, norm)                      # status 0 is asserted in solve
            for t, n in enumerate(names):
                if t == victim:
                    assert 0 <= cnt[t] <= rows[t]["K"], (norm, victim, cnt[t])
                    assert np.all(idx[t, cnt[t]:] == 0) and np.all((idx[t, :cnt[t]] >= 1) & (idx[t, :cnt[t]] <= 48))
                else:
                    Za, ia, ca = alone(row(n), norm)
                    assert cnt[t] == ca and np.array_equal(idx[t], ia) and same_bits(Z[t], Za), (norm, victim, n)


def test_bad_arguments_come_back_as_error_codes():
    lib, ctx = _lib_ctx()
    N, S, K = 4, 2, 2
    p = lambda x: x.ctypes.data_as(C.c_void_p)

    def call(Gr, pnorm, strideA, batch=2):
        a = np.zeros((batch * max(strideA, N * Gr),), np.complex64)
        y, z = np.zeros(batch * N * S, np.complex64), np.zeros(batch * Gr * S, np.complex64)
        return lib.jstsp_mmv_omp_c32(ctx.handle, N, Gr, S, batch, p(a), strideA, p(y), K, pnorm, p(z), None, None, HOST)

    assert call(8, 2, 0) == 0 and call(8, 1, 32) == 0 and call(4096, 2, 0, batch=1) == 0
    assert call(4097, 2, 0) == -3                                  # JSTSP_E_UNSUPPORTED
    assert call(8, 3, 0) == -4 and call(8, 0, 0) == -4            # JSTSP_E_ARG
    assert call(8, 2, 31) == -2 and call(8, 2, -32) == -2         # JSTSP_E_SHAPE: strideA < N Gr
    assert b"strideA" in lib.jstsp_last_error()


def test_tssr_on_device_resident_inputs_equals_the_host_call():
    import torch
    import jstsp19_amd as J
    g = load_golden("proposed_refnative")
    args = (30, float(g["tau_Y"]), 0.1, 8)
    host = J.tssr(g["subY"], g["Omega"], g["A"], g["B"], *args)
    dev = torch.device("cuda:0")
    t = lambda a, dt: J.colmajor(torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).to(dev))
    out = J.tssr(t(g["subY"], np.complex64), t(g["Omega"], np.float32), t(g["A"], np.complex64), t(g["B"], np.complex64), *args)
    torch.cuda.synchronize()
    for h, d, what in zip(host, out, ("S_tssr", "Y_svt", "S_svt")):
        assert same_bits(np.asarray(h), d.cpu().numpy()), what
