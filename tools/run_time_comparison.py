#!/usr/bin/env python3
"""plot_time_comparisions.m on the device: its seven estimators (LS, OMP, VAMP, CoSaMP, OMP-MMV, Proposed, Proposed-PAI) at
its parameters (:8-25: Nt = 4, Nr = 32, L = 4, T = 35, Mr = 4, numOfnz = 100, noise variance 10^(-5/10), Imax = 100), each
timed ON ITS OWN (the reference's tocs at :86, :98, :103 reuse a stale tic) between two stream synchronisations, inputs
resident on the GPU.  Prints one JSON line: seconds per solver and trial (a call solves --batch trials at once; --trials
are split into such calls).  It reports; nothing asserts a time."""
import argparse, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jstsp19_amd as J
from jstsp19_amd import montecarlo as mc
from jstsp19_amd.system_model import SweepParams, build_trials

ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=64)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--seed", type=int, default=20190913)
ap.add_argument("--omp-f64", action="store_true", help="OMP column from the float64 entry (jstsp_omp_kron_f64) instead of the fp32 kernels")
a = ap.parse_args()
p = SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4, snr_db=5.0)          # :8-24
K, Imax = 100, 100                                                    # :20, :25
dev = torch.device("cuda", 0)
tot = {k: 0.0 for k in ("ls", "omp", "vamp", "cosamp", "omp_mmv", "proposed", "proposed_pai")}


def timed(name, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    tot[name] += time.perf_counter() - t0
    return out


done = 0
for rep in range(2):                                                  # the first pass warms every path up and is not counted
    for t0_ in range(0, a.trials, a.batch):
        b = min(a.batch, a.trials - t0_)
        inp = build_trials(p, t0_, b, seed=a.seed, device=dev, with_hbf=True)
        Y, A, B = inp["Y_hbf"], inp["A_hbf"], inp["B_hbf"]
        Gb, Ym = mc._times_h(B, B), mc._times_h(Y, B)                 # B*B', Y_hbf_nr*B'  (:74-75)
        y = Ym.transpose(1, 2).reshape(b, -1).contiguous()            # vec
        tY, tZ, rho = inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy()
        timed("ls", lambda: J.ls_estimate(Y, A, B))                   # :79
        if a.omp_f64:
            timed("omp", lambda: J.omp_kron_f64(A, Gb, y, K))         # :83-85 in float64
        else:
            timed("omp", lambda: J.omp_kron(A, Gb, y, K))             # :83-85
        timed("vamp", lambda: J.vamp_kron(Ym, A, Gb, 1.0, K))         # :91
        timed("cosamp", lambda: J.cosamp_kron(A, Gb, y, K))           # :96
        timed("omp_mmv", lambda: J.mmv_omp(A, mc._times(None, Y, J.pinv(B)), K))   # :101-102
        timed("proposed", lambda: J.proposed_algorithm(inp["subY"], inp["Omega"], inp["A"], inp["B"], Imax, tY, tZ, rho,
                                                       "approximate", want_ce=False))                                  # :120
        timed("proposed_pai", lambda: J.proposed_algorithm_angles(inp["subY"], inp["Omega"], inp["indx_S"], inp["A"], inp["B"],
                                                                  Imax, tY, tZ, rho, "approximate", K, want_ce=False))  # :125
        done += b
    if rep == 0:
        tot = {k: 0.0 for k in tot}
        done = 0
print(json.dumps({"driver": "plot_time_comparisions", "trials": done, "batch": a.batch, **({"omp_precision": "f64"} if a.omp_f64 else {}),
                  "seconds_per_trial": {k: v / done for k, v in tot.items()}}))
