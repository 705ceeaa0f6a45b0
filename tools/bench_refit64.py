#!/usr/bin/env python
"""What the re-fit costs: BASELINE configs[1] (or --small), --trials trials built by the library, float64.

  solve            proposed_algorithm_f64 at --imax, want_ce off, estimates/s
  refit            refit_f64 alone on that estimate, for every (K, iters) of --K x --iters
  solve_refit      the two back to back
  parent / new     with --parent-lib: jstsp_proposed_algorithm_f64 of that library and of the tree's, called through the C ABI in
                   the same process in pairs whose order alternates, --reps times each after --warmup unmeasured calls; medians and
                   the spread

Every time is taken around a synchronised stream.  Prints ONE JSON line and writes it to --out.  No threshold is asserted."""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import jstsp19_amd as J
from jstsp19_amd import _lib
from jstsp19_amd.system_model import SweepParams, build_trials

ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=256)
ap.add_argument("--imax", type=int, nargs="+", default=[30, 100])
ap.add_argument("--K", type=int, nargs="+", default=None, help="default: 2048 4096 (--small: 64 160)")
ap.add_argument("--iters", type=int, nargs="+", default=[5, 20])
ap.add_argument("--snr-db", type=float, default=5.0)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--seed", type=int, default=20190913)
ap.add_argument("--small", action="store_true", help="Nt=4, Nr=32, L=4, T=35, Mr=4 instead of BASELINE configs[1]")
ap.add_argument("--parent-lib", default=None, help="a libjstsp_mi355x.so of the parent commit, for the solver's own rate beside the tree's")
ap.add_argument("--out", default=None)
a = ap.parse_args()

dev = torch.device("cuda:0")
p = SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4, snr_db=a.snr_db) if a.small else SweepParams(Nt=64, Nr=64, L=8, T=64, Mr=8, snr_db=a.snr_db)
N, M, Gr, G2 = p.solver_shape
Ks = a.K or ([64, 160] if a.small else [2048, 4096])
inp = build_trials(p, 0, a.trials, seed=a.seed, sweep_idx=0, device=dev)
wide = lambda x: J.colmajor(x.to(torch.complex128))
args = (wide(inp["subY"]), J.colmajor(inp["Omega"].to(torch.float64)), wide(inp["A"]), wide(inp["B"]))
prm = (inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())


def once(fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def timed(fn):
    for _ in range(a.warmup):
        fn()
    return [once(fn) for _ in range(a.reps)]


def stat(ts):
    return {"seconds_median": float(np.median(ts)), "seconds_min": float(min(ts)), "seconds_max": float(max(ts)),
            "estimates_per_s": a.trials / float(np.median(ts))}


res = {"tool": "bench_refit64", "shape": [N, M, Gr, G2], "trials": a.trials, "snr_db": a.snr_db, "seed": a.seed, "reps": a.reps,
       "warmup": a.warmup, "results": []}
for imax in a.imax:
    solve = lambda: J.proposed_algorithm_f64(*args, imax, *prm, want_ce=False)
    row = {"Imax": imax, "solve": stat(timed(solve)), "refit": []}
    S = solve()[0]
    for k in Ks:
        for n in a.iters:
            row["refit"].append({"K": k, "iters": n, "refit": stat(timed(lambda: J.refit_f64(*args, S, k, n))),
                                 "solve_refit": stat(timed(lambda: J.refit_f64(*args, solve()[0], k, n)))})
    res["results"].append(row)

if a.parent_lib:
    # the solver's own entry of both libraries through the C ABI, on the same device arrays and torch's stream, alternating
    ctx_new = _lib.default_context(0)
    lib_new, lib_old = ctx_new._lib, C.CDLL(a.parent_lib)
    sig = _lib.SIGNATURES["jstsp_proposed_algorithm_f64"]
    lib_old.jstsp_proposed_algorithm_f64.restype, lib_old.jstsp_proposed_algorithm_f64.argtypes = sig
    h_old = C.c_void_p()
    assert lib_old.jstsp_create(0, C.byref(h_old)) == 0
    assert lib_old.jstsp_set_stream(h_old, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)) == 0
    ctx_new.use_torch_stream()
    S_out = J.empty_colmajor(a.trials, Gr, G2, torch.complex128, dev)
    Y_out = J.empty_colmajor(a.trials, N, M, torch.complex128, dev)
    dp = C.POINTER(C.c_double)
    sc = [np.ascontiguousarray(v, dtype=np.float64) for v in prm]
    imax = a.imax[-1]

    def raw(lib, h):
        rc = lib.jstsp_proposed_algorithm_f64(h, N, M, Gr, G2, a.trials, args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), 0,
                                              args[3].data_ptr(), G2 * M, imax, *[v.ctypes.data_as(dp) for v in sc], 0, None,
                                              S_out.data_ptr(), Y_out.data_ptr(), None, 1)
        assert rc == 0, rc

    pair = {"parent": (lib_old, h_old), "new": (lib_new, ctx_new.handle)}
    ts = {"parent": [], "new": []}
    bits = {}
    for _ in range(a.warmup):
        for k, (lib, h) in pair.items():
            raw(lib, h)
    for r in range(a.reps):                     # the order within a pair alternates, so that neither library always runs second
        for k in (("parent", "new"), ("new", "parent"))[r % 2]:
            lib, h = pair[k]
            ts[k].append(once(lambda: raw(lib, h)))
            bits[k] = S_out.clone()
    res["solver_parent_vs_new"] = {"Imax": imax, "parent": stat(ts["parent"]), "new": stat(ts["new"]),
                                   "same_bits": bool(torch.equal(torch.view_as_real(bits["parent"]), torch.view_as_real(bits["new"])))}
    lib_old.jstsp_destroy(h_old)

print(json.dumps(res))
if a.out:
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
