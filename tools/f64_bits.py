#!/usr/bin/env python
"""Bits of the float64 OMP family and of the float64 ADMM (Alg. 1 and Alg. 2) on the cases the tests define, to hold one build
of the library against another: ``--dump FILE`` writes every output array (and every refusal message) of the library that
JSTSP_LIB names (default: the one built in the tree); ``--against FILE`` runs the same cases and compares byte for byte.

    JSTSP_LIB=/path/to/other/libjstsp_mi355x.so python tools/f64_bits.py --dump other.npz
    python tools/f64_bits.py --against other.npz --report profiles/f64_frame_bits.json
"""
import argparse
import ctypes as C
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

DEV = torch.device("cuda:0")


def _np(x):
    return None if x is None else (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x))


def _up(x):
    """matrices, vectors of complex values and index arrays go to the device; scalars and per-trial real scalars stay"""
    if isinstance(x, np.ndarray) and (x.ndim >= 2 or (x.ndim == 1 and x.dtype.kind in "ci")):
        t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
        return J.colmajor(t) if t.ndim >= 2 else t
    return x


def both(name, fn, *args, **kw):
    """fn on numpy arguments (host memspace) and on the same as torch tensors (device memspace)"""
    for mem, a, k in (("host", args, kw), ("device", tuple(_up(x) for x in args), {k: _up(v) for k, v in kw.items()})):
        out = fn(*a, **k)
        for i, o in enumerate(out if isinstance(out, tuple) else (out,)):
            if o is not None:
                yield "%s/%s/%d" % (name, mem, i), _np(o)


def omp_cases():
    import omp64_problems as Q
    for kind, shapes, groups in (("dense", Q.DENSE, Q.dense_groups), ("kron", Q.KRON, Q.kron_groups)):
        for shape in shapes:
            for G in groups(shape):
                names = list(G["rows"])
                m = len(G["rows"][names[0]]["ref"]["idx"])
                V = np.stack([G["rows"][n]["v"].astype(np.complex128) for n in names])
                if kind == "kron":
                    dic = tuple(np.asarray(d, np.complex128) for d in G["dict"])
                    run = lambda v, Af, Bf, m=m: J.omp_kron_f64(Af, Bf, v, m)
                else:
                    dic = (np.asarray(G["dict"], np.complex128),)
                    run = lambda v, A, m=m: J.OMP_f64(A, v, m)[0:4:3]                              # x_hat, targetMatrix
                    yield from both("omp64/dense%s/%s/index" % (shape, G["name"]), lambda v, A, m=m: J.OMP_f64(A, v, m)[1], V, *dic)
                tag = "omp64/%s%s/%s" % (kind, shape, G["name"])
                yield from both(tag + "/batch", run, V, *dic)
                for i, n in enumerate(names):                       # every row alone: E2/E4 ties, D2 scales, the NaN row, v = 0
                    yield from both(tag + "/" + n, run, V[i], *dic)


def mmv_cases():
    import mmv64_problems as Q
    for r in Q.problems()["rows"]:                                  # M1 shapes with Gr = 1 and Gr = 4096, rank-5 K = 6, Y = 0, 2^+-400
        for norm in Q.NORMS:
            yield from both("mmv64/%s/%s" % (r["name"], norm), lambda A, Y, r=r, norm=norm: J.mmv_omp_f64(A, Y, r["K"], norm=norm),
                            np.asarray(r["A"], np.complex128), np.asarray(r["Y"], np.complex128))


def admm_cases():
    import std64_problems as Q
    def load_golden(name):
        with np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"), allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    for name in Q.NAMES:                                            # P5: N = 72, the global-memory Jacobi
        p = Q.problem(name)
        a = tuple(np.asarray(p[k]) if k in ("subY", "Omega", "A", "B") else p[k]
                  for k in ("subY", "Omega", "A", "B", "Imax", "tau_Y", "tau_S", "rho"))
        kw = {} if p["indx_S"] is None else {"indx_S": p["indx_S"]}
        yield from both("std64/%s/inverts" % name, lambda *x, **k: J.proposed_algorithm_std_f64(*x, info=True, **k), *a, **kw)
        PA, PB = J.pinv_f64(a[2]), J.pinv_f64(a[3])
        yield from both("std64/%s/given" % name, lambda *x, **k: J.proposed_algorithm_std_f64(*x, info=True, **k), *a, PA=PA, PB=PB, **kw)
        yield from both("alg2/%s" % name, J.proposed_algorithm_f64, *a, **kw)
    p = Q.problem("P3")                                             # a batch of three against three single calls
    for fn, tag in ((J.proposed_algorithm_std_f64, "std64"), (J.proposed_algorithm_f64, "alg2")):
        cut = lambda s: (p["subY"][s], p["Omega"][s], p["A"], p["B"][s], p["Imax"], p["tau_Y"][s], p["tau_S"][s], p["rho"][s])
        three = [_np(o) for o in fn(*cut(slice(0, 3)), indx_S=p["indx_S"][:3])]
        ones = [[_np(o) for o in fn(*cut(slice(t, t + 1)), indx_S=p["indx_S"][t:t + 1])] for t in range(3)]
        for i, o in enumerate(three):
            yield "%s/P3/batch3/%d" % (tag, i), o
            yield "%s/P3/batch3_equals_singles/%d" % (tag, i), np.array(
                [o[t].tobytes() == ones[t][i].reshape(o[t].shape).tobytes() for t in range(3)])
    for name in ("proposed_small", "proposed_small_lowsnr", "proposed_refnative"):
        g = load_golden(name)
        a = (g["subY"], g["Omega"], g["A"], g["B"], int(g["Imax"]), float(g["tau_Y"]), float(g["tau_Z"]), float(g["rho"]))
        yield from both("alg2/%s/approximate" % name, J.proposed_algorithm_f64, *a)
        yield from both("alg2/%s/angles" % name, J.proposed_algorithm_f64, *a, indx_S=np.asarray(g["indx_S"]))
    import resume_problems as RP                                    # the resumed entries: from zero, legs (2, 4), from a foreign state
    for name, shared in ((n, s) for n in ("R1", "R2") for s in (False, True)):
        p = RP.problem(name, shared)
        a, prm = (p["subY"], p["Omega"], p["A"], p["B"]), (p["tau_Y"], p["tau_S"], p["rho"])
        for kind in ("approx", "angles", "std"):
            fn = J.proposed_algorithm_std_resume_f64 if kind == "std" else J.proposed_algorithm_resume_f64
            kw = {"indx_S": p["indx_S"]} if kind == "angles" else {}
            tag = "resume64/%s/%s/%s" % (name, "sharedB" if shared else "ownB", kind)
            yield from both(tag + "/zero6", lambda *x, **k: fn(*x[:4], 6, *x[4:], **k), *a, *prm, **kw)

            def legs(*x, **k):
                first = fn(*x[:4], 2, *x[4:], **k)
                return first + fn(*x[:4], 4, *x[4:], state=first[3], it0=2, **k)
            yield from both(tag + "/legs24", legs, *a, *prm, **kw)
            if (name, shared) != ("R2", True):                      # tests/test_gpu_resume64.py: test_from_the_halved_state_of_another_trial
                st = 0.5 * np.roll(_np(fn(*a, 3, *prm, **kw)[3]), -1, axis=0)
                yield from both(tag + "/halved", lambda *x, **k: fn(*x[:4], 3, *x[4:], it0=3, **k), *a, *prm, state=st, **kw)


def policy_cases():
    """jstsp_proposed_refresh_f64 on the policies of tests/test_gpu_refresh64.py (from zero, and a second leg from the returned state
    and order) and jstsp_proposed_until_f64 on the configurations and tolerances of tests/until_ref.py, at three values of `check`"""
    import test_gpu_refresh64 as TR
    import test_gpu_until64 as TU
    import until_ref as U
    for name, shared in (("R1", False), ("R1", True), ("R2", False)):
        for mem in ("host", "device"):
            for start, period, prior in TR.POLICIES:
                tag = "refresh64/%s/%s/%s/start%d_period%d_prior%d" % (name, "sharedB" if shared else "ownB", mem, start, period, prior)
                leg1 = TR._refresh(name, shared, mem, 3, start, period, prior)
                leg2 = TR._refresh(name, shared, mem, 3, start, period, prior, state=leg1[3], it0=3)
                for i, o in enumerate(tuple(leg1) + tuple(leg2)):
                    if o is not None:
                        yield "%s/%d" % (tag, i), _np(o)
    for name, shared, use_indx, refresh in U.CONFIGS:
        for mem in ("host", "device"):
            for tname, tols in sorted(U.TOLS.items()) + [("none", (0.0, 0.0, 0.0))]:
                for check in TU.CHECKS if tname == "abc" else (3,):
                    tag = "until64/%s/%s/indx%d/%s/%s/%s/check%d" % (name, "sharedB" if shared else "ownB", use_indx, refresh, mem, tname, check)
                    out = TU._until(name, shared, mem, np.asarray(tols, np.float64), use_indx=use_indx, refresh=refresh, min_iters=U.MIN_ITERS,
                                    check=check)
                    for i, o in enumerate(out):
                        if o is not None:
                            yield "%s/%d" % (tag, i), o


def entry_refusal_cases():
    """status, message and the outputs written (none) of every row of tests/test_gpu_admm_refusals.py for the float64 entries"""
    import test_gpu_admm_refusals as R
    for name in sorted(n for n, e in R.ENTRIES.items() if e[1] == "f64"):
        for mem in (R.HOST, R.DEVICE):
            c = R.Call(name, mem)
            for label, over, _ in R.rows_for(name):
                rc, msg, written = c(over)
                yield "entry_refused/%s/mem%d/%s" % (name, mem, label), np.frombuffer(("%d: %s %s" % (rc, msg, sorted(written))).encode(), np.uint8)


def refusal_cases():
    """the message of every refused big shape: it names the largest batch that fits, i.e. the measured workspace"""
    import test_gpu_f64_workspace as W
    lib, ctx = _lib.load(), _lib.default_context(0)
    p, d, big, one = W._p, W._d, W.BIG, W.DUMMY
    entries = dict(W.ENTRIES)
    entries["proposed_std_f64"] = lambda lib, h, mem, _: lib.jstsp_proposed_std_f64(
        h, 512, 512, 512, 512, big, p(one), p(one), p(one), 512 * 512, p(one), 512 * 512, None, None, 3, d(W.ONES), d(W.ONES), d(W.ONES), None,
        p(one), p(one), p(one), None, mem)
    # the resumed entries, with both state blocks in the layout
    entries["proposed_resume_f64"] = lambda lib, h, mem, _: lib.jstsp_proposed_resume_f64(
        h, 512, 512, 512, 512, big, p(one), p(one), p(one), 512 * 512, p(one), 512 * 512, 3, d(W.ONES), d(W.ONES), d(W.ONES), 0, None,
        p(one), p(one), p(one), 0, p(one), p(one), mem)
    entries["proposed_std_resume_f64"] = lambda lib, h, mem, _: lib.jstsp_proposed_std_resume_f64(
        h, 512, 512, 512, 512, big, p(one), p(one), p(one), 512 * 512, p(one), 512 * 512, None, None, 3, d(W.ONES), d(W.ONES), d(W.ONES), None,
        p(one), p(one), p(one), None, 0, p(one), p(one), mem)
    for name in sorted(entries):
        for mem in (W.HOST, W.DEVICE):
            rc = entries[name](lib, ctx.handle, mem, True)
            msg = ("%d: " % rc).encode() + lib.jstsp_last_error()
            yield "refusal/%s/%d" % (name, mem), np.frombuffer(msg, np.uint8)


def cases():
    for gen in (omp_cases, mmv_cases, admm_cases, policy_cases, refusal_cases, entry_refusal_cases):
        yield from gen()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--dump", metavar="FILE")
    g.add_argument("--against", metavar="FILE")
    ap.add_argument("--report", metavar="JSON", help="with --against: write the counts here")
    a = ap.parse_args()
    got = {}
    for k, v in cases():
        assert k not in got, k
        got[k] = np.ascontiguousarray(v)
    if a.dump:
        np.savez(a.dump, **got)
        print(json.dumps({"library": os.path.relpath(_lib.LIB_PATH, ROOT), "arrays": len(got)}))
        return 0
    with np.load(a.against, allow_pickle=False) as z:
        ref = {k: z[k] for k in z.files}
    diff = sorted(k for k in set(ref) | set(got) if k not in ref or k not in got or ref[k].dtype != got[k].dtype or
                  ref[k].shape != got[k].shape or ref[k].tobytes() != got[k].tobytes())
    diff += sorted(k for k in got if "equals_singles" in k and not got[k].all())
    rep = {"library": os.path.relpath(_lib.LIB_PATH, ROOT), "against": os.path.basename(a.against), "arrays_compared": len(set(ref) | set(got)),
           "bytes_compared": int(sum(v.nbytes for v in got.values())), "differences": len(diff), "differing": diff}
    print(json.dumps(rep))
    if a.report:
        with open(a.report, "w") as f:
            json.dump(rep, f, indent=1)
            f.write("\n")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
