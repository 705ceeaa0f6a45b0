"""The fp32 entry points outside the solver measure their workspace with the code that lays it out (csrc/solver_common.h: arena_open).
What can be seen of that from outside: on a context of its own a call succeeds; the same call again leaves ``workspace_bytes()``
where it was and returns the same bytes; a smaller call afterwards does not grow the workspace either.  One shape on each side of
every predicate that changes a layout (use_hgemm through JSTSP_H2=2, hgemm_pair_shape, pinv_fits, eig_needs_global_v at orders
100 | 101, orders 64 | 65 and 128 | 129 of the Gram workspace, want_ce, strided dictionaries, target_out, the two routes of omp_kron,
tall and wide VAMP), on both memspaces."""
import os

import numpy as np
import pytest
import torch

import jstsp19_amd as J
from jstsp19_amd import _lib

pytestmark = pytest.mark.gpu
HOST, DEVICE = _lib.HOST, _lib.DEVICE
H2 = {"JSTSP_H2": "2"}


def cplx(seed, *shape):
    r = np.random.default_rng(seed)
    return (r.standard_normal(shape) + 1j * r.standard_normal(shape)).astype(np.complex64)


def place(a, mem, vec=False):
    if a is None or mem == HOST:
        return a
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if vec else J.colmajor(t)


def lowrank(seed, b, R, C):
    return (cplx(seed, b, R, 2) @ cplx(seed + 1, b, 2, C)).astype(np.complex64)


# ---- one builder per entry: dims -> f(mem, ctx) -------------------------------------------------------------------------------------
def kron(entry):
    def build(N, M, Gr, G2, b, strided=False, m=4):
        lead = (b,) if strided else ()
        A, B = cplx(1, *lead, N, Gr), cplx(2, *lead, G2, M)
        X = cplx(3, b, Gr, G2) if entry == "synthesize" else cplx(3, b, N, M)
        if entry == "omp_kron":
            return lambda mem, c: J.omp_kron(place(A, mem), place(B, mem), place(X.reshape(b, -1), mem, True), m, ctx=c)
        fn = {"correlate": J.correlate, "synthesize": J.synthesize, "ls": J.ls_estimate}[entry]
        return lambda mem, c: fn(place(X, mem), place(A, mem), place(B, mem), ctx=c)
    return build


def matrix(entry):
    def build(R, C, b=2, ce=True):
        H = lowrank(4, b, R, C)
        Y = H + 0.1 * cplx(6, b, R, C)
        Om = (np.random.default_rng(7).random((b, R, C)) < 0.6).astype(np.float32)
        OH = (H * Om).astype(np.complex64)
        if entry == "sparse_admm":
            Dr, Dt = cplx(8, R, R) / 4, cplx(9, C, C) / 4
            return lambda mem, c: J.sparse_admm(place(H, mem) if ce else None, place(Y, mem), place(Dr, mem), place(Dt, mem), 3, want_ce=ce, ctx=c)
        return {"pinv": lambda mem, c: J.pinv(place(Y, mem), ctx=c),
                "svt": lambda mem, c: J.svt(place(Y, mem), 0.5, ctx=c),
                "nmse": lambda mem, c: J.nmse_spectral(place(Y, mem), place(H, mem), ctx=c),
                "rate": lambda mem, c: J.rate(place(Y, mem), place(H, mem), 0.1, ctx=c),
                "mc_svt": lambda mem, c: J.mc_svt(place(OH, mem), place(Om, mem), 2, 0.5, 0.8, ctx=c),
                "mc_admm": lambda mem, c: J.mc_admm(place(H, mem) if ce else None, place(OH, mem), place(Om, mem), 2, 0.5, 0.8, want_ce=ce, ctx=c)}[entry]
    return build


def _lambda_max_sequence(n, b, steps):
    G = cplx(10, steps, b, n, 2 * n)
    G = np.ascontiguousarray(np.swapaxes(G @ np.conj(np.swapaxes(G, -1, -2)), 2, 3))

    def call(mem, c):
        g = G if mem == HOST else torch.from_numpy(G).to("cuda:0")
        out = np.empty((steps, b), np.float32) if mem == HOST else torch.empty((steps, b), dtype=torch.float32, device="cuda:0")
        ptr = lambda x: x.data_ptr() if torch.is_tensor(x) else x.ctypes.data
        if mem == DEVICE:
            c.use_torch_stream()
        _lib.check(c._lib.jstsp_lambda_max_sequence_c32(c.handle, n, b, steps, ptr(g), ptr(out), mem), "jstsp_lambda_max_sequence_c32")
        return out
    return call


def _gradient_head(G2, b, strided=False, rv=True):
    lead = (b,) if strided else ()
    Tc, A, GA, RV = cplx(11, b, 64, G2), cplx(12, *lead, 64, 64), cplx(13, *lead, 64, 64), cplx(14, b, 64, G2)
    return lambda mem, c: J.gradient_head(place(Tc, mem), place(A, mem), place(GA, mem), place(RV, mem) if rv else None, ctx=c)


def _omp(meas, size_d, b, m, strided=False, target=True):
    A, v = cplx(15, *((b,) if strided else ()), meas, size_d), cplx(16, b, meas)

    def call(mem, c):
        x, idx, _, tm = J.OMP(place(A, mem), place(v, mem, True), m, want_target=target, ctx=c)
        return x, idx, tm
    return call


def _mmv_omp(N, Gr, S, b, K, strided=False):
    A, Y = cplx(17, *((b,) if strided else ()), N, Gr), cplx(18, b, N, S)
    return lambda mem, c: J.mmv_omp(place(A, mem), place(Y, mem), K, ctx=c)


def _vamp_kron(Na, Gr, G2, b, strided=False):
    lead = (b,) if strided else ()
    Af, Bh, Y = cplx(19, *lead, Na, Gr), cplx(20, *lead, G2, G2 + 2), cplx(21, b, Na, G2)
    Gb = np.ascontiguousarray(Bh @ np.conj(np.swapaxes(Bh, -1, -2)))
    return lambda mem, c: J.vamp_kron(place(Y, mem), place(Af, mem), place(Gb, mem), 1.0, 4, nit=3, ctx=c)


def _vamp(M, N, b):
    A, y = cplx(22, M, N), cplx(23, b, M)
    return lambda mem, c: J.vamp(place(y, mem, True), place(A, mem), 1.0, 4, nit=3, ctx=c)


def lazy(build):
    """build(*a, **k) as a call that makes its arrays when it first runs (collecting the tests makes none)"""
    def deferred(*a, **k):
        made = []

        def call(mem, c):
            if not made:
                made.append(build(*a, **k))
            return made[0](mem, c)
        return call
    return deferred


# entry -> (the smaller call, [(layout branch, call, environment)])
def _cases():
    K = lambda e, *a, **k: lazy(kron(e))(*a, **k)
    Mx = lambda e, *a, **k: lazy(matrix(e))(*a, **k)
    lambda_max_sequence, gradient_head, omp, mmv_omp, vamp_kron, vamp = (lazy(f) for f in (_lambda_max_sequence, _gradient_head, _omp, _mmv_omp, _vamp_kron, _vamp))
    out = {}
    for e in ("correlate", "synthesize"):
        out[e] = (K(e, 8, 12, 8, 8, 2), [("plain", K(e, 16, 24, 8, 12, 3), {}), ("strided", K(e, 16, 24, 8, 12, 3, True), {}),
                                         ("h2", K(e, 64, 64, 8, 64, 3), H2), ("h2_strided", K(e, 64, 64, 8, 64, 3, True), H2),
                                         ("h2_below_pair", K(e, 64, 64, 8, 64, 510), H2), ("h2_pair", K(e, 64, 64, 8, 64, 512), H2)])
    out["ls"] = (K("ls", 16, 24, 8, 12, 2), [("fit_fit", K("ls", 64, 64, 64, 64, 2), {}), ("fit_fit_strided", K("ls", 16, 24, 8, 12, 3, True), {}),
                                             ("inv_fit", K("ls", 80, 24, 72, 12, 2), {}), ("fit_inv", K("ls", 16, 80, 8, 72, 2), {}),
                                             ("inv_inv_strided", K("ls", 80, 80, 72, 72, 2, True), {}), ("inv100", K("ls", 104, 24, 100, 12, 1), {}),
                                             ("inv101", K("ls", 104, 24, 101, 12, 1), {}), ("inv129", K("ls", 136, 24, 129, 12, 1), {})])
    out["pinv"] = (Mx("pinv", 8, 8), [("8x12", Mx("pinv", 8, 12, 3), {})])
    out["svt"] = (Mx("svt", 8, 8), [("%dx%d" % s, Mx("svt", *s), {}) for s in ((8, 12), (12, 8), (64, 70), (65, 70), (100, 104), (101, 104), (129, 132))])
    out["nmse"] = (Mx("nmse", 8, 8), [("%dx%d" % s, Mx("nmse", *s), {}) for s in ((8, 12), (128, 130), (129, 130))])
    out["rate"] = (Mx("rate", 8, 8), [("%dx%d" % s, Mx("rate", *s), {}) for s in ((8, 12), (100, 104), (101, 104))])
    out["lambda_max_sequence"] = (lambda_max_sequence(8, 2, 2), [("n8", lambda_max_sequence(8, 3, 4), {}), ("n65", lambda_max_sequence(65, 3, 2), {})])
    out["mc_svt"] = (Mx("mc_svt", 8, 8), [("%dx%d" % s, Mx("mc_svt", *s), {}) for s in ((8, 12), (65, 70))])
    for e in ("mc_admm", "sparse_admm"):
        shapes = ((8, 12), (65, 70)) if e == "mc_admm" else ((16, 16), (65, 70))
        out[e] = (Mx(e, 8, 8, ce=False), [("%dx%d/ce%d" % (s + (ce,)), Mx(e, *s, ce=ce), {}) for s in shapes for ce in (False, True)])
    out["gradient_head"] = (gradient_head(64, 1, rv=False), [("shared", gradient_head(128, 2, rv=False), {}), ("shared_rv", gradient_head(128, 2), {}),
                                                   ("strided_rv", gradient_head(128, 2, True), {})])
    out["omp"] = (omp(16, 32, 2, 3, target=False), [("target", omp(32, 64, 3, 4), {}), ("no_target", omp(32, 64, 3, 4, target=False), {}), ("strided", omp(32, 64, 3, 4, True), {}),
                                      ("batch17_gemm", omp(32, 64, 17, 4), {}), ("batch65_mgs", omp(32, 64, 65, 4), {})])
    out["omp_kron"] = (K("omp_kron", 8, 8, 8, 8, 2, m=3), [("gram", K("omp_kron", 8, 8, 8, 12, 3), {}), ("gram_strided", K("omp_kron", 8, 8, 8, 12, 3, True), {}),
                                                           ("gram_h2", K("omp_kron", 64, 64, 8, 64, 3), H2), ("gram_m96", K("omp_kron", 16, 8, 16, 16, 2, m=96), {}),
                                                           ("meas_m97", K("omp_kron", 16, 8, 16, 16, 2, m=97), {}),
                                                           ("meas_m97_h2", K("omp_kron", 64, 64, 8, 64, 2, m=97), H2)])
    out["mmv_omp"] = (mmv_omp(8, 16, 2, 2, 2), [("shared", mmv_omp(16, 32, 4, 3, 4), {}), ("strided", mmv_omp(16, 32, 4, 3, 4, True), {}),
                                                ("K_above_N", mmv_omp(16, 32, 4, 2, 20), {})])
    out["vamp"] = (vamp_kron(8, 8, 2, 1), [("kron_wide", vamp_kron(8, 16, 4, 3), {}), ("kron_tall", vamp_kron(16, 8, 4, 3), {}),
                                           ("kron_strided", vamp_kron(8, 16, 4, 3, True), {}), ("dense_wide", vamp(8, 16, 2), {}), ("dense_tall", vamp(16, 8, 2), {})])
    return out


CASES = _cases()


def _bytes(out):
    out = out if isinstance(out, tuple) else (out,)
    return [None if o is None else (o.cpu().numpy() if torch.is_tensor(o) else np.asarray(o)).tobytes() for o in out]


@pytest.mark.parametrize("entry", sorted(CASES))
def test_measured_equals_used(entry):
    smaller, branches = CASES[entry]
    for name, call, env in branches:
        for mem in (HOST, DEVICE):
            ctx = _lib.Context(0)
            os.environ.update(env)
            try:
                first = _bytes(call(mem, ctx))                  # (a refusal raises JstspError)
                torch.cuda.synchronize()
                ws = ctx.workspace_bytes()
                again = _bytes(call(mem, ctx))
                torch.cuda.synchronize()
            finally:
                for k in env:
                    os.environ.pop(k, None)
            assert ctx.workspace_bytes() == ws, "%s/%s/mem%d: the same call again changed the workspace" % (entry, name, mem)
            assert again == first, "%s/%s/mem%d: the same call again returned other bytes" % (entry, name, mem)
            smaller(mem, ctx)
            torch.cuda.synchronize()
            assert ctx.workspace_bytes() == ws, "%s/%s/mem%d: a smaller call grew the workspace" % (entry, name, mem)
            ctx.close()
