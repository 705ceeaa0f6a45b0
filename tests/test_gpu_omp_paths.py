"""OMP.m:17 selection on every dispatch path of jstsp_omp_c32 / jstsp_omp_kron_c32 (csrc/omp.hip), with the engineered
problems of tests/omp_problems.py: exact and near ties, a residual that is exactly zero before m, v = 0, and inputs scaled
by powers of two far outside the range where |c|^2 fits an fp32.

Dense dictionary, by call shape:
  correlation  omp_corr_gemv_kernel (per-problem dictionary, or batch <= 16) | complex-fp32 MFMA GEMM (shared, batch > 16)
  step         omp_step_reg_kernel<1> (batch <= 64, meas <= 1024; at meas 1024 with m 24 fewer LDS columns than atoms)
               | <2> (meas 1025..2048) | omp_step_kernel<1024> (meas > 2048) | omp_step_mgs_kernel (batch > 64)
Kronecker dictionary: omp_gram_kernel (coefficient domain, m <= 96) | the measurement-space Gram-Schmidt loop (m >= 97),
each with the fp32 GEMM (JSTSP_H2=0) and the split-f16 GEMM (JSTSP_H2=2) correlation, shared and per-problem Bf.

Each engineered problem sits at the first and at the last position of calls with batch 1, 16, 17, 64, 65 and 1024 (random
problems fill the rest); its index set must equal the float64 literal OMP.m on the same values, on every path and at every
position, so it is also the same across all of them.  Random problems sampled from the fillers are held to the reference
on the prefix of decisive iterations (see include/jstsp.h, jstsp_omp_c32, for the selection contract)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import omp_problems as P
from conftest import check_below, rel_err
from oracle import solvers as O

pytestmark = pytest.mark.gpu

DENSE = [(96, 160, 10), (1024, 256, 24), (1536, 256, 20), (2100, 256, 8)]
KRON = [(8, 16, 8, 16, 24), (8, 16, 8, 16, 97)]
BATCHES = (1, 16, 17, 64, 65, 1024)
PER_PROBLEM_BATCHES = (1, 17, 65)
TOL_X = {"dense": 5e-7, "kron": 2e-6}           # (measured on MI355X: 1.0e-7, 4.0e-7)


@functools.lru_cache(maxsize=None)
def _dense(shape):
    return P.dense_groups(*shape, seed=sum(shape))


@functools.lru_cache(maxsize=None)
def _kron(shape):
    return P.kron_groups(*shape, seed=sum(shape))


def _fillers(Phi64, n, rng):
    """random sparse problems on the group's dictionary (not checked against the reference unless sampled)."""
    meas, size_d = Phi64.shape
    X = np.zeros((n, size_d), complex)
    for t in range(n):
        X[t, rng.choice(size_d, 5, replace=False)] = rng.standard_normal(5) + 1j * rng.standard_normal(5)
    noise = 0.05 * (rng.standard_normal((n, meas)) + 1j * rng.standard_normal((n, meas))) / np.sqrt(meas)
    return (X @ Phi64.T + noise).astype(np.complex64)


def _layouts(names, batch):
    """lists of (name or None) per row: every engineered row at position 0.. and at the last positions."""
    k = len(names)
    if batch >= 2 * k:
        lay = [None] * batch
        for i, n in enumerate(names):
            lay[i] = n
            lay[batch - 1 - i] = n
        return [lay]
    if batch >= k:
        front = list(names) + [None] * (batch - k)
        return [front, front[::-1]]
    return [[n] for n in names]


class _Env:
    def __init__(self, h2):
        self.h2 = h2

    def __enter__(self):
        self.old = os.environ.get("JSTSP_H2")
        if self.h2 is not None:
            os.environ["JSTSP_H2"] = self.h2

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("JSTSP_H2", None)
        else:
            os.environ["JSTSP_H2"] = self.old


def _check_row(tag, kind, row, idx, x, T=None):
    ref = row["ref"]
    assert np.array_equal(np.asarray(idx, np.int64), ref["idx"]), (tag, row["kind"], list(idx), list(ref["idx"]))
    x = np.asarray(x)
    assert np.all(np.isfinite(x)), tag
    if row["kind"] == "E5":
        assert not np.any(x), tag
    else:
        check_below("omp_paths.%s.x" % kind, rel_err(x, ref["x"]), TOL_X[kind])
    if T is not None:
        assert np.array_equal(T, ref["T"]), tag                  # the selected columns, copied


def _check_scaled(tag, res):
    """E6: x_hat of a scaled problem is E1's x_hat of the same call shape times the exact factor."""
    e1 = res.get("E1")
    for name, x in res.items():
        if name.startswith("E6v"):
            check_below("omp_paths.scale.x", rel_err(np.asarray(x) * 2.0 ** -int(name[3:]), e1), 1e-6)
        elif name.startswith("E6A"):
            check_below("omp_paths.scale.x", rel_err(np.asarray(x) * 2.0 ** int(name[3:]), e1), 1e-6)


def _sample_prefix(tag, Phi64, V, idx, m, rows):
    """random filler problems against the reference up to their first non-decisive iteration."""
    full = 0
    for t in rows:
        x, io, _, _, gaps = O.omp_literal_margins(Phi64, V[t].astype(complex), m)
        bad = np.flatnonzero(gaps < P.DECISIVE)
        n = bad[0] if len(bad) else m
        full += n == m
        assert np.array_equal(np.asarray(idx[t][:n], np.int64), io[:n]), (tag, t, n)
    assert full >= (3 * len(rows)) // 4, (tag, full, len(rows))      # the prefix check is not vacuous


@pytest.mark.parametrize("shape", DENSE, ids=lambda s: "meas%d_d%d_m%d" % s)
def test_dense_omp_selection_on_every_path_and_batch(shape):
    import jstsp19_amd as J
    meas, size_d, m = shape
    groups = _dense(shape)
    rng = np.random.default_rng(meas)
    scaled = {}
    for per_problem in (False, True):
        for batch in (PER_PROBLEM_BATCHES if per_problem else BATCHES):
            res = {}
            for G in groups:
                A, Phi64, rows = G["dict"], G["Phi64"], G["rows"]
                names = list(rows)
                for lay in _layouts(names, batch):
                    nb = len(lay)
                    V = _fillers(Phi64, nb, rng)
                    for i, n in enumerate(lay):
                        if n is not None:
                            V[i] = rows[n]["v"]
                    Ain = np.ascontiguousarray(np.broadcast_to(A, (nb,) + A.shape)) if per_problem else A
                    want_t = nb <= 65
                    x, idx, _, T = J.OMP(Ain, V if nb > 1 else V[0], m, want_target=want_t)
                    x, idx = np.asarray(x).reshape(nb, -1), np.asarray(idx).reshape(nb, -1)
                    T = np.asarray(T).reshape(nb, meas, m) if want_t else None
                    tag = (shape, "per-problem" if per_problem else "shared", batch, G["name"])
                    for i, n in enumerate(lay):
                        if n is not None:
                            _check_row(tag + (n, i), "dense", rows[n], idx[i], x[i], None if T is None else T[i])
                            res[n] = x[i]
                    if G["name"] == "main" and batch == 1024 and not per_problem:
                        free = [i for i, n in enumerate(lay) if n is None]
                        _sample_prefix(tag, Phi64, V, idx, m, free[1::len(free) // 8][:8])
            _check_scaled((shape, batch, per_problem), res)
            scaled[(batch, per_problem)] = res["E1"]
    # the same x_hat whatever the path, to fp32 rounding of the orthogonalisation
    e1 = scaled[(1, False)]
    for key, x in scaled.items():
        check_below("omp_paths.dense.x_across_paths", rel_err(x, e1), 2e-7)     # (measured 4e-8)


@pytest.mark.parametrize("h2", ["0", "2"])
@pytest.mark.parametrize("shape", KRON, ids=lambda s: "coef_m%d" % s[4] if s[4] <= 96 else "meas_m%d" % s[4])
def test_kron_omp_selection_on_every_path_and_batch(shape, h2):
    import jstsp19_amd as J
    N, M, Gr, G2, m = shape
    groups = _kron(shape)
    rng = np.random.default_rng(m)
    with _Env(h2):
        for per_problem in (False, True):
            for batch in (PER_PROBLEM_BATCHES if per_problem else BATCHES):
                res = {}
                for G in groups:
                    (Af, Bf), Phi64, rows = G["dict"], G["Phi64"], G["rows"]
                    names = list(rows)
                    for lay in _layouts(names, batch):
                        nb = len(lay)
                        V = _fillers(Phi64, nb, rng)
                        for i, n in enumerate(lay):
                            if n is not None:
                                V[i] = rows[n]["v"]
                        Bin = np.ascontiguousarray(np.broadcast_to(Bf, (nb,) + Bf.shape)) if per_problem else Bf
                        x, idx = J.omp_kron(Af, Bin, V if nb > 1 else V[0], m)
                        x, idx = np.asarray(x).reshape(nb, -1), np.asarray(idx).reshape(nb, -1)
                        tag = (shape, "H2=" + h2, "per-problem" if per_problem else "shared", batch, G["name"])
                        for i, n in enumerate(lay):
                            if n is not None:
                                _check_row(tag + (n, i), "kron", rows[n], idx[i], x[i])
                                res[n] = x[i]
                        if G["name"] == "main" and batch == 1024 and not per_problem:
                            free = [i for i, n in enumerate(lay) if n is None]
                            _sample_prefix(tag, Phi64, V, idx, m, free[1::len(free) // 8][:8])
                _check_scaled((shape, h2, batch, per_problem), res)


def test_omp_c64_entry_selects_the_same_atoms():
    """jstsp_omp_c64 (MATLAB's own element type, converted to the complex64 path) on the engineered set of one shape."""
    import jstsp19_amd
    from jstsp19_amd import _lib
    lib, ctx = jstsp19_amd.load(), jstsp19_amd.Context(0)
    meas, _, m = DENSE[0]
    for G in _dense(DENSE[0]):
        A = np.ascontiguousarray(G["dict"].astype(np.complex128).T)                  # column-major
        rows = list(G["rows"].values())
        V = np.ascontiguousarray(np.stack([r["v"] for r in rows]).astype(np.complex128))
        b, sd = len(rows), G["dict"].shape[1]
        xh, idx = np.empty(b * sd, complex), np.empty(b * m, np.int32)
        _lib.check(lib.jstsp_omp_c64(ctx.handle, meas, sd, b, A.ctypes.data_as(C.c_void_p), 0,
                                     V.ctypes.data_as(C.c_void_p), m, xh.ctypes.data_as(C.c_void_p),
                                     idx.ctypes.data_as(C.c_void_p), None, 0), "jstsp_omp_c64")
        for t, r in enumerate(rows):
            _check_row(("c64", G["name"], t), "dense", r, idx.reshape(b, m)[t], xh.reshape(b, -1)[t])
