#!/usr/bin/env python
"""Bits, refusals and workspace sizes of the fp32 entry points outside the solver whose workspace goes through ``arena_open``
(csrc/solver_common.h), to hold one build of the library against another as tools/f32_frame_bits.py does for proposed_algorithm.
Every call runs on a context of its own, on both memspaces, at the smallest shape on each side of every predicate that changes
the layout of the workspace.  ``--dump FILE`` writes, per call, each output array (above 4 KiB: its SHA-256), the status, the
message of a refused call and ``workspace_bytes()``, from the library that JSTSP_LIB names (default: the one built in the tree);
``--against FILE`` runs the same calls and compares: outputs, statuses and messages byte for byte, the workspace as "never larger".

    JSTSP_LIB=/path/to/other/libjstsp_mi355x.so python tools/f32_aux_bits.py --dump other.npz
    python tools/f32_aux_bits.py --against other.npz --report profiles/f32_aux_bits.json
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from jstsp19_amd import _lib  # noqa: E402

if os.environ.get("JSTSP_LIB"):
    _lib.LIB_PATH = os.environ["JSTSP_LIB"]

import jstsp19_amd as J  # noqa: E402
import torch  # noqa: E402

DEV = torch.device("cuda:0")
HOST, DEVICE = _lib.HOST, _lib.DEVICE
H2 = {"JSTSP_H2": "2"}          # the split-f16 products at any shape (use_hgemm)
WS = "/status_workspace"

# why a call's workspace may be smaller than the older sum gave it (by the first matching start of its tag)
REASONS = (
    ("vamp", "the sum carried 4096 bytes of slack"),
    ("ls/", "the sum counted the temporaries of each Gram inverse although they are given back before the next array is taken, and a third Gr x G2 array that is never taken"),
    ("pinv/", "the sum counted the output array, which only a host call takes"),
    ("omp/", "the sum counted targetMatrix although target_out is NULL"),
    ("rate/", "the sum counted the global eigenvector array of orders that keep it in LDS"),
    ("gradient_head/", "the sum counted a staged copy of RV although RV is NULL"),
    ("mc_admm/", "the sum counted a staged copy of Htrue although ce_out is NULL"),
    ("sparse_admm/", "the sum counted a staged copy of Htrue although ce_out is NULL"),
)


def cplx(seed, *shape):
    r = np.random.default_rng(seed)
    return (r.standard_normal(shape) + 1j * r.standard_normal(shape)).astype(np.complex64)


def place(a, mem, vec=False):
    """a host array as the wrappers take it for this memspace (device: matrices column-major per problem; vec: one vector per problem)"""
    if a is None or mem == HOST:
        return a
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if vec else J.colmajor(t)


def lowrank(seed, batch, R, C, rank=2):
    return (cplx(seed, batch, R, rank) @ cplx(seed + 1, batch, rank, C)).astype(np.complex64)


def dicts(seed, N, M, Gr, G2, batch, strided):
    lead = (batch,) if strided else ()
    return cplx(seed, *lead, N, Gr), cplx(seed + 1, *lead, G2, M)


# ---- the calls: name -> f(mem, ctx) returning the outputs -----------------------------------------------------------------------
def kron_cases():
    """correlate / synthesize / ls / omp_kron: N, M, Gr, G2, batch, strided dictionaries, environment"""
    shapes = [("small", 16, 24, 8, 12, 3, False, {}), ("strided", 16, 24, 8, 12, 3, True, {}), ("batch1", 16, 24, 8, 12, 1, False, {}),
              ("h2", 64, 64, 8, 64, 3, False, H2), ("h2_strided", 64, 64, 8, 64, 3, True, H2),
              ("h2_pair", 64, 64, 8, 64, 512, False, H2), ("h2_below_pair", 64, 64, 8, 64, 510, False, H2)]
    for nm, N, M, Gr, G2, b, st, env in shapes:
        A, B = dicts(1, N, M, Gr, G2, b, st)
        K, S = cplx(3, b, N, M), cplx(4, b, Gr, G2)
        yield "correlate/" + nm, env, lambda mem, c, K=K, A=A, B=B: J.correlate(place(K, mem), place(A, mem), place(B, mem), ctx=c)
        yield "synthesize/" + nm, env, lambda mem, c, S=S, A=A, B=B: J.synthesize(place(S, mem), place(A, mem), place(B, mem), ctx=c)
    # use_hgemm's own threshold: m n k = 2^22 with k, n >= 64, and one column of the dictionary less
    for nm, M in (("h2_at_threshold", 256), ("h2_below_threshold", 255)):
        A, B = dicts(5, 64, M, 8, 256, 1, False)
        K, S = cplx(6, 1, 64, M), cplx(7, 1, 8, 256)
        yield "correlate/" + nm, {}, lambda mem, c, K=K, A=A, B=B: J.correlate(place(K, mem), place(A, mem), place(B, mem), ctx=c)
        yield "synthesize/" + nm, {}, lambda mem, c, S=S, A=A, B=B: J.synthesize(place(S, mem), place(A, mem), place(B, mem), ctx=c)
    # ls: pinv_fits on either side (72 x 80 does not fit), eig_needs_global_v of the inverted Gram (orders 100 | 101), Newton-Schulz above 128
    for nm, N, M, Gr, G2, b, st in (("fit_fit", 16, 24, 8, 12, 3, False), ("fit_fit_strided", 16, 24, 8, 12, 3, True), ("inv_fit", 80, 24, 72, 12, 2, False),
                                    ("fit_inv", 16, 80, 8, 72, 2, False), ("inv_inv", 80, 80, 72, 72, 2, False), ("inv_inv_strided", 80, 80, 72, 72, 2, True),
                                    ("inv100", 104, 104, 100, 100, 1, False), ("inv101", 104, 104, 101, 101, 1, False), ("inv130", 140, 24, 130, 12, 1, False)):
        A, B = dicts(8, N, M, Gr, G2, b, st)
        Y = cplx(9, b, N, M)
        yield "ls/" + nm, {}, lambda mem, c, Y=Y, A=A, B=B: J.ls_estimate(place(Y, mem), place(A, mem), place(B, mem), ctx=c)
    yield "ls/refused", {}, lambda mem, c: J.ls_estimate(place(cplx(1, 1, 72, 80), mem), place(cplx(2, 72, 80), mem), place(cplx(3, 12, 80), mem), ctx=c)
    # omp_kron: the coefficient-domain route (m <= 96) and the measurement-space one, each with either correlation; batch > 64: omp_step_mgs_kernel
    for nm, N, M, Gr, G2, b, st, m, env in (("gram", 8, 8, 8, 8, 3, False, 4, {}), ("gram_strided", 8, 8, 8, 8, 3, True, 4, {}), ("gram_h2", 64, 64, 8, 64, 3, False, 4, H2),
                                            ("gram_m96", 16, 8, 16, 16, 2, False, 96, {}), ("meas_m97", 16, 8, 16, 16, 2, False, 97, {}),
                                            ("meas_m97_h2_strided", 64, 64, 8, 64, 2, True, 97, H2), ("meas_m97_batch80", 16, 8, 16, 16, 80, False, 97, {})):
        A, B = dicts(10, N, M, Gr, G2, b, st)
        y = cplx(11, b, N * M)
        yield "omp_kron/" + nm, env, lambda mem, c, A=A, B=B, y=y, m=m: J.omp_kron(place(A, mem), place(B, mem), place(y, mem, True), m, ctx=c)


def matrix_cases():
    """pinv, svt, nmse, rate, lambda_max_sequence, mc_svt, mc_admm, sparse_admm, gradient_head"""
    yield "pinv/small", {}, lambda mem, c: J.pinv(place(cplx(20, 3, 8, 12), mem), ctx=c)
    yield "pinv/refused", {}, lambda mem, c: J.pinv(place(cplx(20, 1, 80, 80), mem), ctx=c)
    # the Gram workspace with a projector: orders <= 64 | above, eig_needs_global_v (100 | 101), the block Jacobi above 128
    for R, C in ((8, 12), (12, 8), (64, 70), (65, 70), (100, 104), (101, 104), (129, 132)):
        Y = lowrank(21, 2, R, C) + 0.1 * cplx(23, 2, R, C)
        yield "svt/%dx%d" % (R, C), {}, lambda mem, c, Y=Y: J.svt(place(Y, mem), 0.5, ctx=c)
    yield "svt/refused", {}, lambda mem, c: J.svt(place(np.zeros((1, 2049, 2049), np.complex64), mem), 0.5, ctx=c)
    # the Gram workspace of a norm: Lanczos vectors up to order 128, the basis of the block Jacobi above
    for R, C in ((8, 12), (128, 130), (129, 130)):
        Zb = lowrank(24, 2, R, C)
        S = Zb + 0.05 * cplx(26, 2, R, C)
        yield "nmse/%dx%d" % (R, C), {}, lambda mem, c, S=S, Zb=Zb: J.nmse_spectral(place(S, mem), place(Zb, mem), ctx=c)
    for R, C in ((8, 12), (100, 104), (101, 104)):
        Zb = lowrank(27, 2, R, C)
        S = Zb + 0.05 * cplx(29, 2, R, C)
        yield "rate/%dx%d" % (R, C), {}, lambda mem, c, S=S, Zb=Zb: J.rate(place(S, mem), place(Zb, mem), 0.1, ctx=c)
    yield "rate/refused", {}, lambda mem, c: J.rate(place(cplx(1, 1, 129, 130), mem), place(cplx(2, 1, 129, 130), mem), 0.1, ctx=c)

    G = cplx(30, 4, 3, 8, 16)
    G = np.ascontiguousarray(G @ np.conj(np.swapaxes(G, -1, -2)))           # (steps, batch, n, n), Hermitian

    def lmax_seq(mem, c):
        steps, batch, n, _ = G.shape
        Gc = np.ascontiguousarray(np.swapaxes(G, 2, 3))
        g = Gc if mem == HOST else torch.from_numpy(Gc).to(DEV)
        out = np.empty((steps, batch), np.float32) if mem == HOST else torch.empty((steps, batch), dtype=torch.float32, device=DEV)
        ptr = lambda x: x.data_ptr() if torch.is_tensor(x) else x.ctypes.data
        if mem == DEVICE:
            c.use_torch_stream()
        _lib.check(c._lib.jstsp_lambda_max_sequence_c32(c.handle, n, batch, steps, ptr(g), ptr(out), mem), "jstsp_lambda_max_sequence_c32")
        return out
    yield "lambda_max_sequence/n8", {}, lmax_seq

    for R, C in ((8, 12), (65, 70)):
        H = lowrank(31, 2, R, C)
        Om = (np.random.default_rng(33).random((2, R, C)) < 0.6).astype(np.float32)
        OH = (H * Om).astype(np.complex64)
        yield "mc_svt/%dx%d" % (R, C), {}, lambda mem, c, OH=OH, Om=Om: J.mc_svt(place(OH, mem), place(Om, mem), 3, 0.5, 0.8, ctx=c)
        for ce in (False, True):
            yield "mc_admm/%dx%d/ce%d" % (R, C, ce), {}, lambda mem, c, H=H, OH=OH, Om=Om, ce=ce: J.mc_admm(
                place(H, mem) if ce else None, place(OH, mem), place(Om, mem), 3, 0.5, 0.8, want_ce=ce, ctx=c)
    H, Dr, Dt = lowrank(34, 2, 16, 16), cplx(36, 16, 16) / 4, cplx(37, 16, 16) / 4
    for ce in (False, True):
        yield "sparse_admm/16x16/ce%d" % ce, {}, lambda mem, c, ce=ce: J.sparse_admm(place(H, mem) if ce else None, place(H, mem), place(Dr, mem), place(Dt, mem),
                                                                                    3, want_ce=ce, ctx=c)
    for nm, st, rv in (("shared", False, False), ("shared_rv", False, True), ("strided_rv", True, True)):
        lead = (2,) if st else ()
        Tc, A, GA, RV = cplx(38, 2, 64, 64), cplx(39, *lead, 64, 64), cplx(40, *lead, 64, 64), cplx(41, 2, 64, 64)
        yield "gradient_head/" + nm, {}, lambda mem, c, Tc=Tc, A=A, GA=GA, RV=RV, rv=rv: J.gradient_head(place(Tc, mem), place(A, mem), place(GA, mem),
                                                                                                    place(RV, mem) if rv else None, ctx=c)
    yield "gradient_head/refused", {}, lambda mem, c: J.gradient_head(place(cplx(1, 1, 32, 64), mem), place(cplx(2, 32, 32), mem), place(cplx(3, 32, 32), mem), ctx=c)


def greedy_cases():
    """OMP (its four step kernels), mmv_omp, vamp"""
    for nm, meas, size_d, b, st, m, tgt in (("reg1", 32, 64, 3, False, 4, True), ("reg1_no_target", 32, 64, 3, False, 4, False), ("reg1_strided", 32, 64, 3, True, 4, True),
                                            ("batch1", 32, 64, 1, False, 4, True), ("batch20_gemm", 32, 64, 20, False, 4, True), ("batch64", 32, 64, 64, False, 4, True),
                                            ("batch65_mgs", 32, 64, 65, False, 4, False), ("batch80_mgs", 32, 64, 80, False, 4, True),
                                            ("reg2_meas1030", 1030, 16, 2, False, 3, True), ("step_meas2049", 2049, 16, 2, False, 3, True)):
        A = cplx(50, *((b,) if st else ()), meas, size_d)
        v = cplx(51, b, meas)
        yield "omp/" + nm, {}, lambda mem, c, A=A, v=v, m=m, tgt=tgt: _omp(A, v, m, tgt, mem, c)
    yield "omp/refused", {}, lambda mem, c: _omp(cplx(1, 8, 8), cplx(2, 1, 8), 1025, True, mem, c)
    for nm, N, Gr, S, b, st, K in (("shared", 16, 32, 4, 3, False, 4), ("strided", 16, 32, 4, 3, True, 4), ("K_above_N", 16, 32, 4, 2, False, 20)):
        A = cplx(52, *((b,) if st else ()), N, Gr)
        Y = cplx(53, b, N, S)
        yield "mmv_omp/" + nm, {}, lambda mem, c, A=A, Y=Y, K=K: J.mmv_omp(place(A, mem), place(Y, mem), K, ctx=c)
    for nm, Na, Gr, G2, b, st in (("wide", 8, 16, 4, 3, False), ("tall", 16, 8, 4, 3, False), ("wide_strided", 8, 16, 4, 3, True), ("square", 8, 8, 4, 1, False)):
        lead = (b,) if st else ()
        Af, Bh = cplx(54, *lead, Na, Gr), cplx(55, *lead, G2, 6)
        Gb = np.ascontiguousarray(Bh @ np.conj(np.swapaxes(Bh, -1, -2)))
        Y = cplx(56, b, Na, G2)
        yield "vamp_kron/" + nm, {}, lambda mem, c, Y=Y, Af=Af, Gb=Gb: J.vamp_kron(place(Y, mem), place(Af, mem), place(Gb, mem), 1.0, 4, nit=3, ctx=c)
    for nm, M, N in (("wide", 8, 16), ("tall", 16, 8), ("order130", 130, 140)):
        A, y = cplx(57, M, N), cplx(58, 2, M)
        yield "vamp/" + nm, {}, lambda mem, c, A=A, y=y: J.vamp(place(y, mem, True), place(A, mem), 1.0, 4, nit=2, ctx=c)
    yield "vamp_kron/refused", {}, lambda mem, c: J.vamp_kron(place(cplx(1, 1, 8, 4), mem), place(cplx(2, 8, 16), mem), place(cplx(3, 4, 4), mem), -1.0, 4, nit=3, ctx=c)


def _omp(A, v, m, tgt, mem, c):
    x, idx, _, target = J.OMP(place(A, mem), place(v, mem, True), m, want_target=tgt, ctx=c)
    return x, idx, target


def all_calls():
    for gen in (kron_cases, matrix_cases, greedy_cases):
        yield from gen()


def run(tag, env, fn, mem):
    """One call on a context of its own: (name, array) for every output, then [status, workspace_bytes], then the message of a refusal."""
    ctx = _lib.Context(0)
    os.environ.update(env)
    rc, msg, out = 0, b"", ()
    try:
        try:
            out = fn(mem, ctx)
        except _lib.JstspError as e:
            rc, msg = e.code, _lib.load().jstsp_last_error()
        torch.cuda.synchronize()
        ws = ctx.workspace_bytes()
    finally:
        for k in env:
            os.environ.pop(k, None)
    out = out if isinstance(out, tuple) else (out,)
    for i, o in enumerate(out):
        if o is not None:
            yield "%s/%d" % (tag, i), np.ascontiguousarray(o.cpu().numpy() if torch.is_tensor(o) else o)
    yield tag + WS, np.array([rc, ws], np.int64)
    if rc:
        yield tag + "/message", np.frombuffer(msg, np.uint8)
    ctx.close()


def cases():
    for name, env, fn in all_calls():
        for mem in (HOST, DEVICE):
            yield from run("%s/mem%d" % (name, mem), env, fn, mem)


def collect():
    got, nbytes = {}, 0
    for k, v in cases():
        assert k not in got, k
        nbytes += v.nbytes
        got[k] = v if v.nbytes <= 4096 else np.frombuffer(hashlib.sha256(repr((v.dtype.str, v.shape)).encode() + v.tobytes()).digest(), np.uint8)
    return got, nbytes


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--dump", metavar="FILE")
    g.add_argument("--against", metavar="FILE")
    ap.add_argument("--report", metavar="JSON", help="with --against: write the counts here")
    a = ap.parse_args()
    got, nbytes = collect()
    if a.dump:
        np.savez(a.dump, **got)
        print(json.dumps({"library": os.path.relpath(_lib.LIB_PATH, ROOT), "arrays": len(got), "calls": sum(k.endswith(WS) for k in got)}))
        return 0
    with np.load(a.against, allow_pickle=False) as z:
        ref = {k: z[k] for k in z.files}
    same = lambda k: k in ref and k in got and ref[k].dtype == got[k].dtype and ref[k].shape == got[k].shape and ref[k].tobytes() == got[k].tobytes()
    diff, larger, smaller = [], [], []
    for k in sorted(set(ref) | set(got)):
        if not k.endswith(WS):
            diff += [] if same(k) else [k]
        elif k not in ref or k not in got or ref[k][0] != got[k][0]:
            diff.append(k)
        elif got[k][1] != ref[k][1]:
            why = next((r for p, r in REASONS if k.startswith(p)), None)
            rec = {"call": k[:-len(WS)], "workspace_bytes_against": int(ref[k][1]), "workspace_bytes": int(got[k][1]), "reason": why}
            (smaller if got[k][1] < ref[k][1] and why else larger).append(rec)
    rep = {"library": os.path.relpath(_lib.LIB_PATH, ROOT), "against": os.path.basename(a.against), "calls": sum(k.endswith(WS) for k in got),
           "arrays_compared": len(set(ref) | set(got)), "bytes_compared": int(nbytes), "differences": len(diff), "differing": diff,
           "workspace_larger_or_unexplained": larger, "workspace_smaller": smaller}
    print(json.dumps({k: (v if not isinstance(v, list) else len(v)) for k, v in rep.items()}))
    if a.report:
        with open(a.report, "w") as f:
            json.dump(rep, f, indent=1)
            f.write("\n")
    return 1 if diff or larger else 0


if __name__ == "__main__":
    sys.exit(main())
