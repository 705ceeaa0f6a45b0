"""What every ADMM entry of include/jstsp.h refuses, entry by entry and argument by argument: the four _c32 entries
(jstsp_proposed_algorithm / _resume / _refresh / _until), their four _c64 forms and the six float64 ones (Alg. 2 plain, resumed,
refreshed, until; Alg. 1 plain and resumed), through raw ctypes calls in both memspaces on the problem of tests/test_until32_api.py
(batch 2, 6 x 7, Gr*G2 = 12).  One bad argument per call.  Asserted: the status code, that the message names the entry, and that no
output array was written (every output starts as a sentinel pattern).

The expectations are read off include/jstsp.h and the entries' sources, not off a run.  A few messages do not carry the name of
the entry that was called, because a shared stage words them: "ctx is NULL" and "bad memspace %d" everywhere but in the fp32
refreshed and until entries, and what check_arguments of the fp32 solver refuses for the plain and resumed fp32 entries (a NULL
array of the resumed one, "bad type %d", "strideA too small", the rank rule of 'std').  Those rows assert the literal text instead;
_fragments() lists them.

A _c64 entry narrows its inputs before the fp32 entry behind it can refuse, so such a call does launch conversions; nothing else
here launches, and no call reaches a solver.  tools/f32_frame_bits.py and tools/f64_bits.py dump the same rows (status and whole
message) to hold one build against another."""
import ctypes as C

import numpy as np
import pytest

from jstsp19_amd import _lib

pytestmark = pytest.mark.gpu

HOST, DEVICE = 0, 1
E_NULL, E_SHAPE, E_UNSUPPORTED, E_ARG = -1, -2, -3, -4
N, M, GR, G2, BATCH, IMAX = 6, 7, 4, 3, 2, 3
G = GR * G2
SENTINEL = 0x5A
IX = object()                   # in a row: the call's index list (12 entries per trial)

_HEAD = ("ctx", "N", "M", "Gr", "G2", "batch", "subY", "Omega", "A", "strideA", "B", "strideB")
_PRM = ("Imax", "tau_Y", "tau_S", "rho")
_OUT = ("S", "Y", "ce")
_RES = ("it0", "state_in", "state_out")
_POL = ("indx_S", "n_indx", "start", "period")
_RULE = ("tol", "min_iters", "check")
LAYOUT = {
    "algorithm": _HEAD + _PRM + ("type", "indx_S") + _OUT + ("memspace",),
    "resume": _HEAD + _PRM + ("type", "indx_S") + _OUT + _RES + ("memspace",),
    "refresh": _HEAD + _PRM + ("type",) + _POL + _OUT + _RES + ("indx_out", "memspace"),
    "until": _HEAD + _PRM + ("type",) + _POL + _RULE + _OUT + _RES + ("indx_out", "iters_out", "ce3_out", "memspace"),
    "refresh_f64": _HEAD + _PRM + _POL + _OUT + _RES + ("indx_out", "memspace"),
    "until_f64": _HEAD + _PRM + _POL + _RULE + _OUT + _RES + ("indx_out", "iters_out", "ce3_out", "memspace"),
    "std": _HEAD + ("PA", "PB") + _PRM + ("indx_S",) + _OUT + ("rcond_out", "memspace"),
    "std_resume": _HEAD + ("PA", "PB") + _PRM + ("indx_S",) + _OUT + ("rcond_out",) + _RES + ("memspace",),
}
# entry -> (layout, element type, the name its messages carry)
ENTRIES = {
    "jstsp_proposed_algorithm_c32": ("algorithm", "c32", "proposed_algorithm"),
    "jstsp_proposed_resume_c32": ("resume", "c32", "proposed_algorithm resume"),
    "jstsp_proposed_refresh_c32": ("refresh", "c32", "proposed_algorithm refresh"),
    "jstsp_proposed_until_c32": ("until", "c32", "proposed_algorithm until"),
    "jstsp_proposed_algorithm_c64": ("algorithm", "c64", "proposed_algorithm"),
    "jstsp_proposed_resume_c64": ("resume", "c64", "proposed_algorithm resume"),
    "jstsp_proposed_refresh_c64": ("refresh", "c64", "proposed_algorithm refresh"),
    "jstsp_proposed_until_c64": ("until", "c64", "proposed_algorithm until"),
    "jstsp_proposed_algorithm_f64": ("algorithm", "f64", "proposed_algorithm (float64)"),
    "jstsp_proposed_resume_f64": ("resume", "f64", "proposed_algorithm resume (float64)"),
    "jstsp_proposed_refresh_f64": ("refresh_f64", "f64", "proposed_algorithm refresh (float64)"),
    "jstsp_proposed_until_f64": ("until_f64", "f64", "proposed_algorithm until (float64)"),
    "jstsp_proposed_std_f64": ("std", "f64", "proposed_algorithm 'std' (float64)"),
    "jstsp_proposed_std_resume_f64": ("std_resume", "f64", "proposed_algorithm 'std' resume (float64)"),
}
_FP32_PLAIN = tuple(n for n, (k, el, _) in ENTRIES.items() if el != "f64" and k in ("algorithm", "resume"))
_FP32 = tuple(n for n, (_, el, _) in ENTRIES.items() if el != "f64")
_C32 = tuple(n for n, (_, el, _) in ENTRIES.items() if el == "c32")
_F64 = tuple(n for n, (_, el, _) in ENTRIES.items() if el == "f64")
_STD64 = ("jstsp_proposed_std_f64", "jstsp_proposed_std_resume_f64")
_UNTIL = tuple(n for n in ENTRIES if "_until_" in n)
_REFRESH = tuple(n for n in ENTRIES if "_refresh_" in n)
_TYPED_APPROX_ONLY = tuple(n for n in ENTRIES if "type" in LAYOUT[ENTRIES[n][0]] and n not in _FP32_PLAIN)

# (label, the one bad argument - with what it needs to be reached -, status, entries: None = every entry that has the argument)
ROWS = [
    ("null_ctx", dict(ctx=None), E_NULL, None),
    ("bad_memspace", dict(memspace=7), E_ARG, None),
    ("zero_N", dict(N=0), E_SHAPE, None),
    ("negative_Imax", dict(Imax=-1), E_SHAPE, None),
    ("zero_Imax", dict(Imax=0), E_SHAPE, tuple(n for n in ENTRIES if n != "jstsp_proposed_algorithm_c32")),    # (that one returns zeros)
    ("negative_strideA", dict(strideA=-1), E_SHAPE, None),
    ("negative_strideB", dict(strideB=-1), E_SHAPE, None),
] + [("null_" + k, {k: None}, E_NULL, None) for k in ("subY", "Omega", "A", "B", "tau_Y", "tau_S", "rho", "S")] + [
    ("bad_type", dict(type=5), E_ARG, None),
    ("std_type", dict(type=1), E_UNSUPPORTED, _TYPED_APPROX_ONLY),
    ("std_N_below_Gr", dict(type=1, N=3), E_UNSUPPORTED, _FP32_PLAIN),
    ("std64_N_below_Gr", dict(N=3), E_UNSUPPORTED, _STD64),
    ("std64_M_below_G2", dict(M=2), E_UNSUPPORTED, _STD64),
    # (the float64 Alg. 2 does not judge a short stride: those entries are left out)
    ("strideA_too_small", dict(strideA=1), E_SHAPE, _FP32 + _STD64),
    ("strideB_too_small", dict(strideB=1), E_SHAPE, _FP32 + _STD64),
    # limits, judged before an array is read (a _c64 entry would narrow arrays of the stated size first: left out)
    ("g_at_2_31", dict(Gr=65536, G2=32768), E_SHAPE, ("jstsp_proposed_refresh_c32", "jstsp_proposed_until_c32")),
    ("order_above_2048", dict(N=2049, M=2049), E_UNSUPPORTED, _C32),
    ("f64_g_at_2_31", dict(N=65536, M=32768, Gr=65536, G2=32768), E_UNSUPPORTED, _F64),
    ("f64_order_above_512", dict(N=600, M=600), E_UNSUPPORTED, _F64),
    ("f64_batch_above_65535", dict(batch=65536), E_UNSUPPORTED, _F64),
    ("negative_it0", dict(it0=-1), E_ARG, None),
    ("it0_overflow", dict(it0=2 ** 31 - 2), E_ARG, None),
    ("it0_without_state", dict(it0=2), E_ARG, None),
    ("negative_start", dict(start=-1, period=1), E_ARG, None),
    ("negative_period", dict(period=-1), E_ARG, _REFRESH),                         # (the until entries: no policy)
    ("n_indx_zero_with_list", dict(indx_S=IX, n_indx=0, period=1), E_ARG, None),
    ("n_indx_above_g", dict(indx_S=IX, n_indx=G + 1, period=1), E_ARG, None),
    ("n_indx_without_list", dict(n_indx=1, period=1), E_ARG, None),
    ("rule_n_indx_negative", dict(indx_S=IX, n_indx=-1), E_ARG, _UNTIL),
    ("rule_n_indx_above_g", dict(indx_S=IX, n_indx=G + 1), E_ARG, _UNTIL),
    ("rule_n_indx_without_list", dict(n_indx=1), E_ARG, _UNTIL),
    ("null_tol", dict(tol=None), E_NULL, None),
    ("null_iters_out", dict(iters_out=None), E_NULL, None),
    ("zero_min_iters", dict(min_iters=0), E_ARG, None),
    ("zero_check", dict(check=0), E_ARG, None),
]


def rows_for(name):
    lay = LAYOUT[ENTRIES[name][0]]
    return [(label, over, code) for label, over, code, only in ROWS
            if all(k in lay for k in over) and (only is None or name in only)]


def _fragments(name, label):
    """what the message of a refused call must contain"""
    kind, el, nmf = ENTRIES[name]
    own = name in ("jstsp_proposed_refresh_c32", "jstsp_proposed_until_c32")
    if label == "null_ctx":
        return ["ctx is NULL"] + ([nmf] if own else [])
    if label == "bad_memspace":
        return ["bad memspace 7"] + ([nmf] if own else [])
    if name in _FP32_PLAIN:                             # refused by check_arguments of the fp32 solver
        if label in ("bad_type",):
            return ["bad type 5"]
        if label == "std_N_below_Gr":
            return ["proposed_algorithm 'std': K2 = kron(B.', A) must have full column rank"]
        if label.startswith("null_") and name == "jstsp_proposed_resume_c32":
            return ["proposed_algorithm: NULL array argument"]
        if label.startswith("negative_stride") and el == "c32":
            return [label[-7:] + " too small"]
    if label == "order_above_2048":
        return ["proposed_algorithm: min(N, M) = 2049"]
    if el != "f64" and label.endswith("_too_small"):
        return [label[:7] + " too small"]
    return [nmf]


class Call:
    """The arguments of one entry in one memspace: valid as they stand, every output a sentinel pattern."""

    def __init__(self, name, mem):
        import torch
        kind, el, _ = ENTRIES[name]
        self.name, self.mem, self.layout = name, mem, LAYOUT[kind]
        cdt, rdt = (np.complex64, np.float32) if el == "c32" else (np.complex128, np.float64)
        rng = np.random.default_rng(5)
        cplx = lambda n: (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(cdt)
        place = lambda a: a if mem == HOST else torch.from_numpy(a).to("cuda:0")
        sent = lambda n, dt: place(np.frombuffer(bytes([SENTINEL]) * (n * np.dtype(dt).itemsize), dt).copy())
        nm, ne = N * M, 4 * N * M + 2 * G
        # (a dictionary per trial is held although the call says "shared": the short-stride rows of a _c64 entry read past one)
        self.ins = {"subY": place(cplx(BATCH * nm)), "Omega": place(np.ones(BATCH * nm, rdt)), "A": place(cplx(BATCH * N * GR)),
                    "B": place(cplx(BATCH * G2 * M)),
                    IX: place(np.tile(np.arange(1, G + 1, dtype=np.int32), BATCH))}
        self.host = {k: np.full(BATCH, v, np.float64) for k, v in (("tau_Y", 0.1), ("tau_S", 0.1), ("rho", 0.5), ("tol", 1e-3))}
        self.outs = {"S": sent(BATCH * G, cdt), "Y": sent(BATCH * nm, cdt), "ce": sent(BATCH * 3 * IMAX, np.float64),
                     "state_out": sent(BATCH * ne, cdt), "indx_out": sent(BATCH * G, np.int32), "iters_out": sent(BATCH, np.int32),
                     "ce3_out": sent(BATCH, np.float64), "rcond_out": sent(2, np.float64)}
        self.base = dict(ctx=_lib.default_context(0).handle, N=N, M=M, Gr=GR, G2=G2, batch=BATCH, strideA=0, strideB=0, Imax=IMAX, type=0,
                         indx_S=None, n_indx=0, start=0, period=1 if "refresh" in kind else -1, min_iters=1, check=1, it0=0, state_in=None,
                         PA=None, PB=None, memspace=mem)
        self.base.update(self.ins)
        self.base.update(self.host)
        self.base.update(self.outs)

    def __call__(self, over):
        """(status, message, the outputs that were written) of the call with `over` replacing arguments by name"""
        import torch
        lib = _lib.load()
        v = dict(self.base, **over)
        types = _lib.SIGNATURES[self.name][1]
        assert len(types) == len(self.layout), self.name
        args = []
        for k, ty in zip(self.layout, types):
            x = self.ins[IX] if v[k] is IX else v[k]
            if torch.is_tensor(x):
                x = x.data_ptr()
            elif isinstance(x, np.ndarray):
                x = x.ctypes.data_as(ty) if ty is _lib.c_dp else x.ctypes.data
            args.append(x)
        rc = getattr(lib, self.name)(*args)
        msg = lib.jstsp_last_error().decode() if rc else ""
        torch.cuda.synchronize()
        raw = lambda x: (x.cpu().numpy() if torch.is_tensor(x) else x).view(np.uint8)
        return rc, msg, [k for k, x in self.outs.items() if not (raw(x) == SENTINEL).all()]


@pytest.mark.parametrize("mem", (HOST, DEVICE), ids=("host", "device"))
@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_one_bad_argument_is_refused_with_nothing_written(name, mem):
    call = Call(name, mem)
    rows = rows_for(name)
    assert len(rows) >= 17
    bad = []
    for label, over, code in rows:
        rc, msg, written = call(over)
        if rc != code or written or not all(f in msg for f in _fragments(name, label)):
            bad.append((label, rc, msg, written))
    assert not bad, bad
