#!/usr/bin/env python
"""Bits of the fp32 proposed_algorithm through every entry of its call frame (plain, begin/end, resumed, the _c64 forms, the
pipelined host calls, the refusals, the refreshed and the until entries) and every branch of its driver (branch_cases), to hold one build of
the library against another as tools/f64_bits.py does for float64:
``--dump FILE`` writes, for every call, each output array (above 4 KiB: its SHA-256), the status with
jstsp_last_fused_fallbacks, jstsp_last_dictionary_block and the workspace size, and the message of a refused call, from the
library that JSTSP_LIB names (default: the one built in the tree); ``--against FILE`` runs the same calls and compares byte for
byte, except that the workspace may be smaller than the other library's (reported as ``workspace_smaller``), never larger;
``--trace-call NAME`` runs one call alone, for a kernel trace of it.

    JSTSP_LIB=/path/to/other/libjstsp_mi355x.so python tools/f32_frame_bits.py --dump other.npz
    python tools/f32_frame_bits.py --against other.npz --report profiles/f32_frame_bits.json
    rocprofv3 --kernel-trace --stats -- python tools/f32_frame_bits.py --trace-call small_ce
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from jstsp19_amd import _lib  # noqa: E402

if os.environ.get("JSTSP_LIB"):
    _lib.LIB_PATH = os.environ["JSTSP_LIB"]

import jstsp19_amd as J  # noqa: E402
import torch  # noqa: E402
from jstsp19_amd.system_model import SweepParams, build_trials  # noqa: E402

DEV = torch.device("cuda:0")
HOST, DEVICE = _lib.HOST, _lib.DEVICE
FORCED = {"JSTSP_FUSED_KBACK": "-20"}           # every trial overflows its predicted k scale: one run of the whole batch
UNFUSED = {"JSTSP_FUSED": "0"}
ARGS = ("N", "M", "Gr", "G2", "batch", "subY", "Omega", "A", "strideA", "B", "strideB", "Imax", "tau_Y", "tau_S", "rho", "type", "indx_S",
        "S", "Y", "ce")


class Problem:
    """The arrays of build_trials in the C ABI's layout on the host: complex64 / float32, and widened for the _c64 entries."""

    def __init__(self, inp, Omega=None):
        colm = lambda a: np.ascontiguousarray(np.swapaxes(a.cpu().numpy(), -1, -2))
        self.batch, self.N, self.M = (int(v) for v in inp["subY"].shape)
        self.Gr, self.G2 = int(inp["A"].shape[-1]), int(inp["B"].shape[-2])
        self.arr = {"subY": colm(inp["subY"]), "Omega": colm(inp["Omega"] if Omega is None else Omega).astype(np.float32), "A": colm(inp["A"]),
                    "B": colm(inp["B"]), "indx_S": np.ascontiguousarray(inp["indx_S"].cpu().numpy().astype(np.int32))}
        self.scal = {k: np.ascontiguousarray(inp[s].numpy(), dtype=np.float64) for k, s in (("tau_Y", "tau_Y"), ("tau_S", "tau_Z"), ("rho", "rho"))}
        self.strideA = 0 if inp["A"].ndim == 2 else self.N * self.Gr
        self.strideB = 0 if inp["B"].ndim == 2 else self.G2 * self.M
        self.state_elems = 4 * self.N * self.M + 2 * self.Gr * self.G2


def _place(a, mem):
    return a if mem == HOST else torch.from_numpy(a).to(DEV)


def _ptr(x):
    return None if x is None else (x.data_ptr() if torch.is_tensor(x) else x.ctypes.data)


def _host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else x


def call(tag, P, Imax, mem, *, c64=False, type=0, indx=False, ce=True, resume=None, refresh=None, until=None, env=None, **over):
    """One call of jstsp_proposed_{algorithm,resume,refresh,until}_{c32,c64} on P; yields (name, array) for every output, the status and
    the counters, and the message when the call was refused.  resume: dict(it0, state (host array or None), same (state_out is
    state_in), out (a state is returned)).  refresh: (start, period) of jstsp_proposed_refresh_c32, which takes resume too (default:
    from zero); indx: True the whole order of P, an int its first so many entries (refresh and until only).  until: dict(tol, min_iters, check)
    of jstsp_proposed_until_c32, which takes refresh (default: no policy) and resume too.  over: arguments replaced by name (None: a
    NULL pointer)."""
    lib, ctx = _lib.load(), _lib.default_context(0)
    cdt, rdt = (np.complex128, np.float64) if c64 else (np.complex64, np.float32)
    wide = lambda a: a.astype(rdt if a.dtype.kind == "f" else cdt)
    ins = {k: _place(wide(P.arr[k]), mem) for k in ("subY", "Omega", "A", "B")}
    n_indx = 0 if not indx else (P.Gr * P.G2 if indx is True else int(indx))
    ins["indx_S"] = _place(np.ascontiguousarray(P.arr["indx_S"][:, :n_indx]), mem) if indx else None
    zeros = lambda n, dt: _place(np.zeros(max(int(n), 1), dt), mem)
    outs = {"S": zeros(P.batch * P.Gr * P.G2, cdt), "Y": zeros(P.batch * P.N * P.M, cdt), "ce": zeros(P.batch * 3 * Imax, np.float64) if ce else None}
    v = dict(N=P.N, M=P.M, Gr=P.Gr, G2=P.G2, batch=P.batch, strideA=P.strideA, strideB=P.strideB, Imax=Imax, type=type, memspace=mem)
    v.update({k: _ptr(x) for k, x in list(ins.items()) + list(outs.items())})
    v.update({k: a.ctypes.data_as(_lib.c_dp) for k, a in P.scal.items()})
    v.update(over)
    args = [ctx.handle] + [v[k] for k in ARGS]
    if refresh or until:
        resume = resume or dict(it0=0)
        outs["order"] = zeros(P.batch * min(P.Gr * P.G2, _lib.SUPPORT_TOP_MAX), np.int32)
        start, period = refresh or (0, -1)                      # (a negative period: the until entry without a policy)
        args[-3:-3] = [n_indx, start, period]                   # (... type, indx_S, n_indx, start, period, [rule,] S, Y, ce)
    if until:
        tol = np.ascontiguousarray(np.broadcast_to(np.asarray(until["tol"], np.float64), (P.batch,)))
        outs["iters"], outs["ce3"] = zeros(P.batch, np.int32), zeros(P.batch, np.float64)
        args[-3:-3] = [tol.ctypes.data_as(_lib.c_dp), until.get("min_iters", 2), until.get("check", 1)]
    name = "jstsp_proposed_%s_%s" % ("until" if until else "refresh" if refresh else "resume" if resume else "algorithm", "c64" if c64 else "c32")
    if resume:
        st = resume.get("state")
        s_in = None if st is None else _place(np.ascontiguousarray(st, dtype=cdt), mem)
        s_out = s_in if resume.get("same") else (zeros(P.batch * P.state_elems, cdt) if resume.get("out", True) else None)
        outs["state"] = s_out
        args += [resume["it0"], _ptr(s_in), _ptr(s_out)] + ([_ptr(outs["order"])] if refresh or until else [])
        args += [_ptr(outs["iters"]), _ptr(outs["ce3"])] if until else []
    os.environ.update(env or {})
    try:
        rc = getattr(lib, name)(*args, v["memspace"])
        torch.cuda.synchronize()
        msg = lib.jstsp_last_error() if rc else b""
        info = [rc, ctx.last_fused_fallbacks(), ctx.last_dictionary_block(), ctx.workspace_bytes()]     # (the workspace only grows)
    finally:
        for k in env or {}:
            os.environ.pop(k, None)
    res = {k: (None if x is None else _host(x)) for k, x in outs.items()}
    for k, a in res.items():
        if a is not None:
            yield "%s/%s" % (tag, k), a
    yield tag + "/status_fallbacks_block_workspace", np.array(info, np.int64)
    if rc:
        yield tag + "/message", np.frombuffer(msg, np.uint8)
    call.last = res


def small():
    import test_gpu_overflow_recovery as T
    return Problem(T._small())


def toeplitz():
    p = SweepParams(Nt=64, Nr=64, L=4, T=8, Mr=8, snr_db=5.0)
    assert p.solver_shape == (64, 512, 64, 256)
    return Problem(build_trials(p, 0, 5, seed=43))


def plain_cases():
    for sname, P in (("small", small()), ("toeplitz", toeplitz())):
        for ename, env in (("default", {}), ("forced", FORCED), ("unfused", UNFUSED)):
            for mem in (HOST, DEVICE):
                for type in (_lib.TYPE_APPROXIMATE, _lib.TYPE_STD):
                    for indx in (False, True):
                        for ce in (False, True):
                            for Imax in (0, 1, 2, 12):
                                tag = "plain/%s/%s/mem%d/type%d/indx%d/ce%d/Imax%d" % (sname, ename, mem, type, indx, ce, Imax)
                                yield from call(tag, P, Imax, mem, type=type, indx=indx, ce=ce, env=env)


def two_run_cases():
    """three flagged trials in two runs (tests/test_gpu_overflow_recovery.py): the offsets of a second run"""
    import test_gpu_overflow_recovery as T
    inp, Om, IM = T._two_runs()
    P = Problem(inp, Om)
    for mem in (HOST, DEVICE):
        yield from call("two_runs/plain/mem%d" % mem, P, IM, mem)
        yield from call("two_runs/plain_two_outputs/mem%d" % mem, P, IM, mem, ce=False)
        healthy = Problem(inp)
        list(call("-", healthy, IM // 2, mem, resume=dict(it0=0)))
        st = call.last["state"]
        yield from call("two_runs/resumed/mem%d" % mem, P, IM - IM // 2, mem, resume=dict(it0=IM // 2, state=st))
        yield from call("two_runs/resumed_in_place/mem%d" % mem, P, IM - IM // 2, mem, resume=dict(it0=IM // 2, state=st.copy(), same=True))
    r = J.proposed_algorithm_begin(inp["subY"], Om, inp["A"], inp["B"], IM, inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())
    out = r.end()
    for i, o in enumerate(out):
        yield "two_runs/begin_end/%d" % i, o.cpu().numpy()
    yield "two_runs/begin_end/fallbacks", np.array([r.fallbacks, J.default_context(0).last_fused_fallbacks()])


def begin_end_cases():
    import test_gpu_overflow_recovery as T
    inp = T._small()
    hyp = [inp[k].numpy() for k in ("tau_Y", "tau_Z", "rho")]
    for ename, env in (("default", {}), ("forced", FORCED)):
        for want_ce, indx in ((True, None), (False, None), (True, inp["indx_S"])):
            os.environ.update(env)
            try:
                h = J.proposed_algorithm_begin(inp["subY"], inp["Omega"], inp["A"], inp["B"], 12, *hyp, want_ce=want_ce, indx_S=indx)
                out = h.end()
                torch.cuda.synchronize()
            finally:
                for k in env:
                    os.environ.pop(k, None)
            tag = "begin_end/%s/ce%d/indx%d" % (ename, want_ce, indx is not None)
            for i, o in enumerate(out):
                if o is not None:
                    yield "%s/%d" % (tag, i), o.cpu().numpy()
            ctx = J.default_context(0)
            yield tag + "/fallbacks_block", np.array([h.fallbacks, ctx.last_fused_fallbacks(), ctx.last_dictionary_block()])


def resume_cases():
    P = small()
    for c64 in (False, True):
        for mem in (HOST, DEVICE):
            for ename, env in (("default", {}), ("forced", FORCED)):
                for indx in (False, True):
                    tag = "resume/%s/mem%d/%s/indx%d" % ("c64" if c64 else "c32", mem, ename, indx)
                    kw = dict(c64=c64, indx=indx, env=env)
                    yield from call(tag + "/zero12", P, 12, mem, resume=dict(it0=0), **kw)
                    yield from call(tag + "/leg1", P, 6, mem, resume=dict(it0=0), **kw)
                    st = call.last["state"]
                    yield from call(tag + "/leg2", P, 6, mem, resume=dict(it0=6, state=st), **kw)
                    yield from call(tag + "/leg2_in_place", P, 6, mem, resume=dict(it0=6, state=st.copy(), same=True), **kw)
                    yield from call(tag + "/leg2_no_state_out", P, 6, mem, ce=False, resume=dict(it0=6, state=st, out=False), **kw)
            yield from call("resume/%s/mem%d/refused/negative_it0" % (c64, mem), P, 3, mem, c64=c64, resume=dict(it0=-1))
            yield from call("resume/%s/mem%d/refused/it0_without_state" % (c64, mem), P, 3, mem, c64=c64, resume=dict(it0=2))
            yield from call("resume/%s/mem%d/refused/Imax0" % (c64, mem), P, 0, mem, c64=c64, resume=dict(it0=0))
            yield from call("resume/%s/mem%d/refused/it0_overflow" % (c64, mem), P, 3, mem, c64=c64, resume=dict(it0=2 ** 31 - 2))


def c64_cases():
    for sname, P in (("small", small()), ("toeplitz", toeplitz())):
        for mem in (HOST, DEVICE):
            for ename, env in (("default", {}), ("forced", FORCED), ("unfused", UNFUSED)):
                for type, indx, ce in ((0, False, True), (0, True, True), (0, False, False), (1, False, True)):
                    tag = "c64/%s/mem%d/%s/type%d/indx%d/ce%d" % (sname, mem, ename, type, indx, ce)
                    yield from call(tag, P, 12, mem, c64=True, type=type, indx=indx, ce=ce, env=env)


def pipelined_cases():
    """the two-halves frame (tests/test_gpu_overflow_recovery.py): batch 128 is its threshold"""
    p = SweepParams(Nt=64, Nr=64, L=8, T=64, Mr=8, snr_db=5.0)
    P = Problem(build_trials(p, 0, 128, seed=11))
    for c64 in (False, True):
        for ename, env in (("default", {}), ("forced", FORCED), ("staged", {"JSTSP_HOST_PIPELINE": "0"})):
            yield from call("pipelined/%s/%s" % ("c64" if c64 else "c32", ename), P, 12, HOST, c64=c64, env=env)
        yield from call("pipelined/%s/forced_angles_two_outputs" % ("c64" if c64 else "c32"), P, 12, HOST, c64=c64, env=FORCED, indx=True, ce=False)


def refusal_cases():
    P = small()
    for mem in (HOST, DEVICE):
        for c64 in (False, True):
            tag = "refused/%s/mem%d/" % ("c64" if c64 else "c32", mem)
            for name in ("subY", "Omega", "A", "B", "tau_Y", "tau_S", "rho", "S"):
                yield from call(tag + "null_" + name, P, 3, mem, c64=c64, **{name: None})
            yield from call(tag + "bad_type", P, 3, mem, c64=c64, type=5)
            if not c64:         # (the _c64 form narrows (batch - 1) strideA + N Gr elements before the stride is judged)
                yield from call(tag + "strideA_too_small", P, 3, mem, strideA=1)
            yield from call(tag + "strideB_too_small", P, 3, mem, c64=c64, strideB=1)
            yield from call(tag + "bad_shape", P, 3, mem, c64=c64, N=0)
            yield from call(tag + "negative_Imax", P, -1, mem, c64=c64)
            yield from call(tag + "std_N_below_Gr", P, 3, mem, c64=c64, type=_lib.TYPE_STD, N=P.N // 2)
            yield from call(tag + "bad_memspace", P, 3, mem, c64=c64, memspace=7)
    lib, ctx = _lib.load(), _lib.default_context(0)
    one = np.zeros(16, np.complex64)
    vp = one.ctypes.data
    rc = lib.jstsp_proposed_algorithm_c32(None, 2, 2, 2, 2, 1, vp, vp, vp, 0, vp, 0, 1, None, None, None, 0, None, vp, vp, None, HOST)
    yield "refused/null_context", np.frombuffer(("%d: " % rc).encode() + lib.jstsp_last_error(), np.uint8)
    h = C.c_void_p()
    rc = lib.jstsp_proposed_algorithm_begin_c32(ctx.handle, 2, 2, 2, 2, 1, None, vp, vp, 0, vp, 0, 1, None, None, None, 0, None, vp, vp, None, C.byref(h))
    yield "refused/begin_null_array", np.frombuffer(("%d: " % rc).encode() + lib.jstsp_last_error(), np.uint8)
    rc = lib.jstsp_proposed_algorithm_end(ctx.handle, None, None)
    yield "refused/end_null_handle", np.frombuffer(("%d: " % rc).encode() + lib.jstsp_last_error(), np.uint8)


def random_problem(N, M, Gr, G2, batch=3, seed=7):
    """A random complex64 problem of a shape build_trials does not make: a sparse S0 seen through normalised Gaussian A (shared) and
    B (per trial) under a random mask, with a random order as indx_S."""
    r = np.random.default_rng([seed, N, M, Gr, G2])
    cn = lambda *s: torch.from_numpy(((r.standard_normal(s) + 1j * r.standard_normal(s)) / np.sqrt(2)).astype(np.complex64))
    A, B = cn(N, Gr) / np.sqrt(N), cn(batch, G2, M) / np.sqrt(M)
    S0 = cn(batch, Gr, G2) * torch.from_numpy(r.random((batch, Gr, G2)) < 4.0 / (Gr * G2) + 0.05)
    Om = torch.from_numpy((r.random((batch, N, M)) < 0.6).astype(np.float32))
    subY = (Om * (A @ S0 @ B + 0.05 * cn(batch, N, M))).to(torch.complex64)
    order = np.stack([r.permutation(Gr * G2) + 1 for _ in range(batch)]).astype(np.int32)
    hyp = lambda lo: torch.from_numpy(lo * (1.0 + 0.25 * r.random(batch)))
    return Problem(dict(subY=subY, Omega=Om, A=A, B=B, indx_S=torch.from_numpy(order), tau_Y=hyp(0.05), tau_Z=hyp(0.02), rho=hyp(0.5)))


def shared_b(P):
    """P with the dictionary of its first trial for the whole batch (strideB = 0)"""
    Q = Problem.__new__(Problem)
    Q.__dict__.update(P.__dict__)
    Q.arr = dict(P.arr, B=np.ascontiguousarray(P.arr["B"][0]))
    Q.strideB = 0
    return Q


def toeplitz256():
    p = SweepParams(Nt=64, Nr=64, L=4, T=8, Mr=8, snr_db=5.0)
    return shared_b(Problem(build_trials(p, 0, 256, seed=43)))


# The branches of the solver that the two shapes above (fused-pass shapes, N = 64 <= M, batch 5-6, A shared, B per trial) never reach:
# shape -> what it is for.  Which branch a shape takes depends on the library's tuning; --trace-call runs one call alone for a kernel trace.
BRANCH_SHAPES = {
    (8, 16, 8, 16): "no split-f16 path, cgemm epilogues",
    (16, 8, 8, 8): "N > M: svt_apply / update_x / update_c with an explicit C",
    (64, 1024, 64, 64): "split-f16 products and the epilogues' maxima, no fused pass",
    (128, 256, 128, 128): "N > 64; 'std' with both factors by the Gram inverse",
}
SWITCHES = (("JSTSP_OVERLAP", "0"), ("JSTSP_OVERLAP", "1"), ("JSTSP_TOEPLITZ", "0"), ("JSTSP_TOEPLITZ", "1"), ("JSTSP_FUSED", "2"), ("JSTSP_H2", "0"))


def branch_cases():
    for shape, what in BRANCH_SHAPES.items():
        P = random_problem(*shape)
        for Imax in (1, 2, 6):
            for mem in (HOST, DEVICE):
                for ce in (False, True):
                    for indx in (False, True):
                        for type in (_lib.TYPE_APPROXIMATE, _lib.TYPE_STD):         # ('std' is admissible at all four: N >= Gr, M >= G2)
                            tag = "branch/%dx%dx%dx%d/Imax%d/mem%d/ce%d/indx%d/type%d" % (shape + (Imax, mem, ce, indx, type))
                            yield from call(tag, P, Imax, mem, type=type, indx=indx, ce=ce)
    P = random_problem(16, 8, 8, 8)
    for mem in (HOST, DEVICE):
        for indx in (False, True):
            for type in (_lib.TYPE_APPROXIMATE, _lib.TYPE_STD):
                tag = "branch/16x8x8x8/resumed/mem%d/indx%d/type%d" % (mem, indx, type)
                yield from call(tag + "/leg1", P, 3, mem, type=type, indx=indx, resume=dict(it0=0))
                st = call.last["state"]
                yield from call(tag + "/leg2", P, 3, mem, type=type, indx=indx, resume=dict(it0=3, state=st))
    S, T = small(), toeplitz()
    for Imax in (1, 2, 6):
        for ce in (False, True):
            for indx in (False, True):
                tail = "Imax%d/ce%d/indx%d" % (Imax, ce, indx)
                # (build_trials makes B per trial: the shapes above run with strideB != 0 throughout; one dictionary for the batch here)
                for mem in (HOST, DEVICE):
                    yield from call("branch/small_shared_B/mem%d/%s" % (mem, tail), shared_b(S), Imax, mem, indx=indx, ce=ce)
                yield from call("branch/small_host_compact/" + tail, S, Imax, HOST, indx=indx, ce=ce, env={"JSTSP_HOST_COMPACT": "2"})
                for sname, P in (("small", S), ("toeplitz", T)):
                    for k, v in SWITCHES:
                        for mem in (HOST, DEVICE):
                            yield from call("branch/%s/%s=%s/mem%d/%s" % (sname, k, v, mem, tail), P, Imax, mem, indx=indx, ce=ce, env={k: v})
    P = toeplitz256()           # one dictionary for 256 trials: the pair kernel on K in fragment order
    for mem in (HOST, DEVICE):
        for ce in (False, True):
            for ename, env in (("default", {}), ("unfused", UNFUSED)):
                yield from call("branch/toeplitz256_shared_B/%s/mem%d/ce%d" % (ename, mem, ce), P, 2, mem, ce=ce, env=env)


def refresh_cases():
    """jstsp_proposed_refresh_c32 on the small shape: from zero, and a second leg from the returned state"""
    P = small()
    for mem in (HOST, DEVICE):
        for pol in ((0, 1), (3, 2), (2, 0)):
            for indx in (False, 40):
                for ename, env in (("default", {}), ("forced", FORCED)):
                    if env and pol != (3, 2):
                        continue
                    tag = "refresh/mem%d/start%d_period%d/indx%d/%s" % (mem, pol[0], pol[1], indx, ename)
                    yield from call(tag + "/leg1", P, 6, mem, indx=indx, refresh=pol, env=env)
                    st = call.last["state"]
                    yield from call(tag + "/leg2", P, 6, mem, indx=indx, refresh=pol, resume=dict(it0=6, state=st), env=env)
                    yield from call(tag + "/leg2_two_outputs", P, 6, mem, indx=indx, ce=False, refresh=pol, resume=dict(it0=6, state=st, out=False), env=env)


def until_cases():
    """jstsp_proposed_until_c32 / _c64 on the small shape, with and without a policy, with no positive tol and with one: from zero,
    and a second leg from the returned state"""
    P = small()
    for c64 in (False, True):
        for mem in (HOST, DEVICE):
            for pol in (None, (3, 2)):
                for tol in (0.0, (1e-1, 1e-2)):
                    for indx in (False, 40):
                        tag = "until/%s/mem%d/%s/tol%d/indx%d" % ("c64" if c64 else "c32", mem, "start%d_period%d" % pol if pol else "no_policy",
                                                                 tol != 0.0, indx)
                        rule = dict(tol=np.resize(np.asarray(tol, np.float64), P.batch), min_iters=2, check=3)
                        kw = dict(c64=c64, indx=indx, refresh=pol, until=rule)
                        yield from call(tag + "/leg1", P, 8, mem, **kw)
                        st = call.last["state"]
                        yield from call(tag + "/leg2", P, 8, mem, resume=dict(it0=8, state=st), **kw)
            yield from call("until/%s/mem%d/forced" % ("c64" if c64 else "c32", mem), P, 8, mem, c64=c64, env=FORCED,
                            until=dict(tol=1e-2, min_iters=2, check=3))


def entry_refusal_cases():
    """status, message and the outputs written (none) of every row of tests/test_gpu_admm_refusals.py for the fp32 entries"""
    import test_gpu_admm_refusals as R
    for name in sorted(n for n, e in R.ENTRIES.items() if e[1] != "f64"):
        for mem in (HOST, DEVICE):
            c = R.Call(name, mem)
            for label, over, _ in R.rows_for(name):
                rc, msg, written = c(over)
                yield "entry_refused/%s/mem%d/%s" % (name, mem, label), np.frombuffer(("%d: %s %s" % (rc, msg, sorted(written))).encode(), np.uint8)


# single calls for a kernel trace (one process per call): name -> (problem, arguments of call())
TRACE_CALLS = {
    "small_ce": (small, dict(Imax=6)),
    "small_unfused": (small, dict(Imax=6, env=UNFUSED)),
    "16x8x8x8": (lambda: random_problem(16, 8, 8, 8), dict(Imax=6)),
    "refresh_0_1": (small, dict(Imax=6, refresh=(0, 1))),
    "8x16x8x16": (lambda: random_problem(8, 16, 8, 16), dict(Imax=6)),
    "64x1024x64x64": (lambda: random_problem(64, 1024, 64, 64), dict(Imax=6)),
    "128x256x128x128_std": (lambda: random_problem(128, 256, 128, 128), dict(Imax=6, type=1)),
    "small_host_compact": (small, dict(Imax=6, mem=HOST, env={"JSTSP_HOST_COMPACT": "2"})),
    "toeplitz256_shared_B": (toeplitz256, dict(Imax=2)),
}


def cases():
    _lib.default_context(0).use_torch_stream()
    for gen in (plain_cases, two_run_cases, begin_end_cases, resume_cases, c64_cases, pipelined_cases, refusal_cases, branch_cases, refresh_cases, until_cases,
                entry_refusal_cases):
        yield from gen()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--dump", metavar="FILE")
    g.add_argument("--against", metavar="FILE")
    g.add_argument("--trace-call", choices=sorted(TRACE_CALLS), help="run this one call and nothing else (under a kernel trace)")
    ap.add_argument("--report", metavar="JSON", help="with --against: write the counts here")
    a = ap.parse_args()
    if a.trace_call:
        _lib.default_context(0).use_torch_stream()
        make, kw = TRACE_CALLS[a.trace_call]
        kw = dict(dict(mem=DEVICE), **kw)
        out = dict(call(a.trace_call, make(), kw.pop("Imax"), kw.pop("mem"), **kw))
        print(json.dumps({"call": a.trace_call, "status_fallbacks_block_workspace": out[a.trace_call + "/status_fallbacks_block_workspace"].tolist()}))
        return 0
    got, nbytes = {}, 0
    for k, v in cases():
        if k.startswith("-"):
            continue
        assert k not in got, k
        if len(got) % 500 == 0:
            print("%d arrays, at %s" % (len(got), k), file=sys.stderr, flush=True)
        v = np.ascontiguousarray(v)
        nbytes += v.nbytes
        # (the outputs of the pipelined calls alone are gigabytes: an array above 4 KiB is kept as the SHA-256 of its type, shape and bytes)
        got[k] = v if v.nbytes <= 4096 else np.frombuffer(hashlib.sha256(repr((v.dtype.str, v.shape)).encode() + v.tobytes()).digest(), np.uint8)
    if a.dump:
        np.savez(a.dump, **got)
        print(json.dumps({"library": os.path.relpath(_lib.LIB_PATH, ROOT), "arrays": len(got)}))
        return 0
    with np.load(a.against, allow_pickle=False) as z:
        ref = {k: z[k] for k in z.files}
    # the workspace (last word of a call's record: the context's, which only grows) may be smaller than the other library's, never larger
    WS = "/status_fallbacks_block_workspace"
    smaller = {k: [int(ref[k][-1]), int(got[k][-1])] for k in got if k.endswith(WS) and k in ref and got[k][-1] < ref[k][-1]}
    for k in smaller:
        got[k] = np.append(got[k][:-1], ref[k][-1])
    diff = sorted(k for k in set(ref) | set(got) if k not in ref or k not in got or ref[k].dtype != got[k].dtype or
                  ref[k].shape != got[k].shape or ref[k].tobytes() != got[k].tobytes())
    rep = {"library": os.path.relpath(_lib.LIB_PATH, ROOT), "against": os.path.basename(a.against), "arrays_compared": len(set(ref) | set(got)),
           "bytes_compared": int(nbytes), "differences": len(diff), "differing": diff, "workspace_smaller": smaller}
    print(json.dumps(rep))
    if a.report:
        with open(a.report, "w") as f:
            json.dump(rep, f, indent=1)
            f.write("\n")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
