"""OMP in float64, jstsp_omp_f64 / jstsp_omp_kron_f64 (csrc/omp64.hip), on the problems of tests/omp64_problems.py: every engineered
row of tests/omp_problems.py (E1-E6) at the smallest shapes of tests/test_gpu_omp_paths.py, one dense shape whose correlation is shared
by several workgroups (measures 100, size_d 300), and the rows that only float64 decides (D1: an iteration-1 gap of 1e-9 .. 1e-8;
D2: v * 2^+-400).

Each problem is solved alone through the C ABI in host memory and held against the float64 literal OMP.m on the same values
(``ref`` of the row): the index set is equal (every selection of the set has a float64 gap >= 1e-9 or exactly 0), x_hat lies within
1e-12 of max|x_ref| (the bound of jstsp_mmv_omp_f64: cond of the selected columns <= 100 times 2^-53 times the length of the dot
products), target_out holds A's columns on the bits.  Then the same bits for a batch of all rows of a group with a shared and with
copied dictionaries, on a repeated call, from device memory, through the Python wrappers, and beside a problem whose v holds a NaN."""
import ctypes as C

import numpy as np
import pytest

import omp64_problems as Q
from conftest import check_below, rel_err

pytestmark = pytest.mark.gpu

HOST, DEVICE = 0, 1
TOL_X = 1e-12
_ALONE = {}


def _lib_ctx():
    import jstsp19_amd as J
    return J.load(), J.default_context(0)


def _cm(a):
    """column-major complex128 staging of a matrix or of a stack of matrices"""
    a = np.asarray(a, np.complex128)
    return np.ascontiguousarray(np.swapaxes(a, -1, -2)).reshape(-1)


def solve(kind, dic, V, m, memspace=HOST, shared=True, want_target=True, expect=0):
    """one call on the rows V (b, meas): (x (b, size_d), idx (b, m), T (b, meas, m) or None).  dic: A, or (Af, Bf); shared = False
    gives every problem a copy of its own."""
    lib, ctx = _lib_ctx()
    V = np.ascontiguousarray(np.asarray(V, np.complex128))
    b, meas = V.shape
    mats = [np.asarray(d, np.complex128) for d in (dic if kind == "kron" else (dic,))]
    flat = [_cm(d if shared else np.broadcast_to(d, (b,) + d.shape)) for d in mats]
    strides = [0 if shared else d.size for d in mats]
    size_d = mats[0].shape[1] * (mats[1].shape[0] if kind == "kron" else 1)
    want_target = want_target and kind == "dense"
    x = np.full(b * size_d, np.nan + 1j * np.nan, np.complex128)
    idx = np.full(b * m, -7, np.int32)
    T = np.full(b * meas * m, np.nan + 1j * np.nan, np.complex128) if want_target else None
    if memspace == DEVICE:
        import torch
        ctx.use_torch_stream()
        dev = torch.device("cuda:0")
        up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
        tf, tv, tx, ti, tT = [up(f) for f in flat], up(V.reshape(-1)), up(x), up(idx), up(T)
        p = lambda t: None if t is None else t.data_ptr()
    else:
        tf, tv, tx, ti, tT = flat, V.reshape(-1), x, idx, T
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    if kind == "dense":
        rc = lib.jstsp_omp_f64(ctx.handle, meas, size_d, b, p(tf[0]), strides[0], p(tv), m, p(tx), p(ti), p(tT), memspace)
    else:
        (N, Gr), (G2, M) = mats[0].shape, mats[1].shape
        rc = lib.jstsp_omp_kron_f64(ctx.handle, N, M, Gr, G2, b, p(tf[0]), strides[0], p(tf[1]), strides[1], p(tv), m, p(tx), p(ti), memspace)
    assert rc == expect, (rc, lib.jstsp_last_error())
    if memspace == DEVICE:
        import torch
        torch.cuda.synchronize()
        x, idx, T = tx.cpu().numpy(), ti.cpu().numpy(), None if tT is None else tT.cpu().numpy()
    return x.reshape(b, size_d), idx.reshape(b, m), None if T is None else np.swapaxes(T.reshape(b, m, meas), 1, 2)


def _m(G):
    return len(next(iter(G["rows"].values()))["ref"]["idx"])


def alone(kind, shape, G, name):
    key = (kind, shape, G["name"], name)
    if key not in _ALONE:
        x, idx, T = solve(kind, G["dict"], G["rows"][name]["v"][None], _m(G))
        _ALONE[key] = (x[0].copy(), idx[0].copy(), None if T is None else T[0].copy())
    return _ALONE[key]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_row(kind, G, name, x, idx, T):
    row, ref, tag = G["rows"][name], G["rows"][name]["ref"], (kind, G["name"], name)
    assert Q.decisive(row), tag
    assert np.array_equal(np.asarray(idx, np.int64), ref["idx"]), (tag, idx.tolist(), ref["idx"].tolist())
    assert np.all(np.isfinite(x)), tag
    err = rel_err(x, ref["x"])
    print("%-6s %-6s %-8s rel_err(x) %.3g" % (kind, G["name"], name, err))
    if row["kind"] == "E5":
        assert np.all(idx == 1) and not np.any(x), tag
    else:
        check_below("omp64.%s.%s.x" % (kind, row["kind"]), err, TOL_X)
    if row["kind"] in ("E4a", "E4b"):
        # the zero residual re-selects atom 1: a duplicate, whose coefficient pinv splits equally; x_hat keeps the last copy
        assert idx[-1] == 1 and list(idx).count(1) == 2, (tag, idx.tolist())
        full = G["Phi64"][:, 0].conj() @ row["v"].astype(np.complex128)          # the atom's coefficient (orthonormal dictionary)
        assert abs(x[0] - 0.5 * full) <= 1e-15 * max(1.0, abs(full)), (tag, x[0], full)
        assert (row["kind"] == "E4a") == (abs(full) > 0), tag
    if row["kind"].startswith("D1"):
        assert idx[0] == row["winner"] + 1, tag
    if T is not None:
        assert same_bits(T, G["Phi64"][:, idx - 1]), tag                           # the selected columns, copied


def _groups(kind):
    return [(s, Q.dense_groups(s)) for s in Q.DENSE] if kind == "dense" else [(s, Q.kron_groups(s)) for s in Q.KRON]


@pytest.mark.parametrize("kind", ["dense", "kron"])
def test_every_problem_alone_against_the_float64_reference(kind):
    red = []
    for shape, groups in _groups(kind):
        for G in groups:
            for name in G["rows"]:                                # every row is checked: the report names all that fail
                try:
                    check_row(kind, G, name, *alone(kind, shape, G, name))
                except AssertionError as e:
                    red.append((shape, G["name"], name, str(e)[:300]))
    assert not red, red


@pytest.mark.parametrize("kind", ["dense", "kron"])
def test_scaled_problems_return_the_unscaled_bits_times_the_factor(kind):
    """E6v (v * 2^+-70, 2^+-100) and D2 (2^+-400): E1's index set and E1's x_hat times 2^k on the bits; E6A (dictionary * 2^+-40): E1's
    index set."""
    for shape, groups in _groups(kind):
        main = groups[0]
        x1, i1, _ = alone(kind, shape, main, "E1")
        for name, r in main["rows"].items():
            if "scale_v" in r:
                x, idx, _ = alone(kind, shape, main, name)
                k = r["scale_v"]
                assert np.array_equal(idx, i1), (shape, name)
                assert same_bits(np.ldexp(x.real, -k) + 1j * np.ldexp(x.imag, -k), x1), (shape, name)
        for G in groups[1:]:
            for name, r in G["rows"].items():
                if "scale_A" in r:
                    x, idx, _ = alone(kind, shape, G, name)
                    assert np.array_equal(idx, i1), (shape, name)
                    check_below("omp64.%s.scale_A.x" % kind, rel_err(x * 2.0 ** r["scale_A"], x1), TOL_X)


@pytest.mark.parametrize("kind", ["dense", "kron"])
def test_a_batch_a_repeated_call_and_device_memory_return_the_bits_of_the_single_calls(kind):
    for shape, groups in _groups(kind):
        for G in groups:
            names = list(G["rows"])
            V = np.stack([G["rows"][n]["v"].astype(np.complex128) for n in names])
            m = _m(G)
            first = None
            for mem, shared in ((HOST, True), (HOST, False), (DEVICE, True), (DEVICE, False), (HOST, True)):
                x, idx, T = solve(kind, G["dict"], V, m, mem, shared)
                for t, n in enumerate(names):
                    xa, ia, Ta = alone(kind, shape, G, n)
                    tag = (shape, G["name"], n, mem, shared)
                    assert np.array_equal(idx[t], ia) and same_bits(x[t], xa), tag
                    assert T is None or same_bits(T[t], Ta), tag
                if first is None:
                    first = (x, idx)
            assert same_bits(first[0], x) and same_bits(first[1], idx)            # the repeated call
            xr, ir, _ = solve(kind, G["dict"], V[::-1], m, HOST, True, want_target=False)     # other positions, no target_out
            assert same_bits(xr[::-1], first[0]) and same_bits(ir[::-1], first[1]), (shape, G["name"])


@pytest.mark.parametrize("kind", ["dense", "kron"])
def test_a_nan_in_one_problem_leaves_its_batch_mates_alone(kind):
    shape, groups = _groups(kind)[0]
    G = groups[0]
    names = list(G["rows"])
    m = _m(G)
    for victim, bad in ((0, np.nan), (len(names) - 1, np.inf), (2, complex(0.0, -np.inf))):
        V = np.stack([G["rows"][n]["v"].astype(np.complex128) for n in names])
        V[victim, 3] = bad
        x, idx, _ = solve(kind, G["dict"], V, m)                  # status 0 is asserted in solve
        for t, n in enumerate(names):
            if t == victim:
                assert np.all((idx[t] >= 1) & (idx[t] <= x.shape[1])), (kind, victim, idx[t].tolist())
            else:
                xa, ia, _ = alone(kind, shape, G, n)
                assert np.array_equal(idx[t], ia) and same_bits(x[t], xa), (kind, victim, n)


def test_the_wrappers_return_the_bits_of_the_c_abi_from_numpy_and_torch():
    import torch
    import jstsp19_amd as J
    dev = torch.device("cuda:0")
    shape, G = Q.DENSE[0], Q.dense_groups(Q.DENSE[0])[0]
    m = _m(G)
    for name in ("E1", "E2", "D1hi"):
        xa, ia, Ta = alone("dense", shape, G, name)
        A, v = G["dict"], G["rows"][name]["v"]                    # complex64 values go in as complex64: widened exactly
        x, idx, vv, T = J.OMP_f64(A, v, m)
        assert x.dtype == np.complex128 and idx.dtype == np.int32 and vv is v
        assert same_bits(x, xa) and np.array_equal(idx, ia) and same_bits(T, Ta), name
        tA, tv = J.colmajor(torch.from_numpy(np.asarray(A)).to(dev)), torch.from_numpy(np.asarray(v)).to(dev)
        xt, it, _, Tt = J.OMP_f64(tA, tv, m)
        torch.cuda.synchronize()
        assert xt.is_cuda and xt.dtype == torch.complex128
        assert same_bits(xt.cpu().numpy(), xa) and np.array_equal(it.cpu().numpy(), ia) and same_bits(Tt.cpu().numpy(), Ta), name
    V = np.stack([G["rows"][n]["v"].astype(np.complex128) for n in ("E1", "D1lo")])
    x, idx, _, T = J.OMP_f64(G["dict"], V, m, want_target=False)
    assert T is None and all(same_bits(x[t], alone("dense", shape, G, n)[0]) for t, n in enumerate(("E1", "D1lo")))
    shape, G = Q.KRON[0], Q.kron_groups(Q.KRON[0])[0]
    m = _m(G)
    Af, Bf = G["dict"]
    for name in ("E1", "D1lo"):
        xa, ia, _ = alone("kron", shape, G, name)
        v = G["rows"][name]["v"]
        x, idx = J.omp_kron_f64(Af, Bf, v, m)
        assert same_bits(x, xa) and np.array_equal(idx, ia), name
        tA, tB = (J.colmajor(torch.from_numpy(np.asarray(a)).to(dev)) for a in (Af, Bf))
        xt, it = J.omp_kron_f64(tA, tB, torch.from_numpy(np.asarray(v)).to(dev), m)
        torch.cuda.synchronize()
        assert same_bits(xt.cpu().numpy(), xa) and np.array_equal(it.cpu().numpy(), ia), name


def test_bad_arguments_come_back_as_error_codes():
    lib, ctx = _lib_ctx()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    a, v, x, idx = np.zeros(2 * 8 * 12, np.complex128), np.zeros(2 * 8, np.complex128), np.zeros(2 * 12, np.complex128), np.zeros(2 * 2000, np.int32)
    call = lambda meas, sd, b, sA, m, mem=HOST, vv=v: lib.jstsp_omp_f64(ctx.handle, meas, sd, b, p(a), sA, None if vv is None else p(vv), m, p(x), p(idx), None, mem)
    assert call(8, 12, 2, 0, 3) == 0 and call(8, 12, 2, 96, 3) == 0
    assert call(8, 12, 2, 0, 20) == 0                             # as in the fp32 entry, m is not limited by measures
    assert call(8, 12, 2, 0, 1025) == -3 and call(65537, 12, 1, 0, 2) == -3          # JSTSP_E_UNSUPPORTED
    assert call(8, 12, 2, 95, 3) == -2 and call(8, 12, 2, 0, 0) == -2                # JSTSP_E_SHAPE
    assert call(8, 12, 2, 0, 3, mem=7) == -4                                         # JSTSP_E_ARG
    assert call(8, 12, 2, 0, 3, vv=None) == -1                                       # JSTSP_E_NULL
    k = lambda N, M, Gr, G2, b, m: lib.jstsp_omp_kron_f64(ctx.handle, N, M, Gr, G2, b, p(a), 0, p(a), 0, p(v), m, p(x), p(idx), HOST)
    assert k(2, 4, 3, 4, 2, 3) == 0 and k(2, 4, 3, 4, 2, 1025) == -3 and k(2, 0, 3, 4, 2, 3) == -2
    assert k(1024, 1024, 3, 4, 1, 3) == -3                        # N M beyond the limit
    assert b"largest batch" in lib.jstsp_last_error() or b"limits" in lib.jstsp_last_error()
