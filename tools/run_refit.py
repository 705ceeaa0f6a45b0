#!/usr/bin/env python
"""What a least-squares re-fit after the solve buys: BASELINE configs[1] (Nt = Nr = 64, L = 8, T = 64,
Mr = 8; or --small: the reference's own driver shape), --trials trials built by the library at --snr-db, float64.

  plain    proposed_algorithm_f64 at Imax in --imax (run as legs of proposed_algorithm_resume_f64, which return its bits)
  genie    the same with the builder's indx_S, the true support order (plot_errorVSsnr.m:143-145): the column a receiver cannot have
  refit    refit_f64 of the plain estimate for every K of --K and every step count of --iters; K <= 4096 through the selection
           kernel inside the entry, a larger K through support_order_f64 of the estimate handed in as indx_S

Every estimate is scored by nmse_spectral_f64 against the trial's Zbar; per cell the mean NMSE over the trials and its standard
error.  Prints ONE JSON line and writes it to --out.  No threshold is asserted."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import jstsp19_amd as J
from jstsp19_amd.system_model import SweepParams, build_trials

ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=256)
ap.add_argument("--snr-db", type=float, default=5.0)
ap.add_argument("--imax", type=int, nargs="+", default=[10, 30, 50, 100])
ap.add_argument("--K", type=int, nargs="+", default=None, help="default: 512 2048 4096 8192 (--small: 32 64 160 512)")
ap.add_argument("--iters", type=int, nargs="+", default=[5, 10, 20])
ap.add_argument("--lam", type=float, default=0.0)
ap.add_argument("--seed", type=int, default=20190913)
ap.add_argument("--batch", type=int, default=256, help="trials built and solved per call")
ap.add_argument("--small", action="store_true", help="Nt=4, Nr=32, L=4, T=35, Mr=4 instead of BASELINE configs[1]")
ap.add_argument("--out", default=None, help="also write the JSON to this file")
a = ap.parse_args()

dev = torch.device("cuda:0")
p = SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4, snr_db=a.snr_db) if a.small else SweepParams(Nt=64, Nr=64, L=8, T=64, Mr=8, snr_db=a.snr_db)
N, M, Gr, G2 = p.solver_shape
g = Gr * G2
Ks = a.K or ([32, 64, 160, 512] if a.small else [512, 2048, 4096, 8192])
if any(not 1 <= k <= g for k in Ks) or min(a.iters) < 1 or sorted(set(a.imax)) != a.imax:
    ap.error("need 1 <= K <= Gr*G2 = %d, iters >= 1 and --imax ascending" % g)
wide = lambda x: J.colmajor(x.to(torch.complex128))
cols = {("plain", i): [] for i in a.imax}
cols.update({("genie", i): [] for i in a.imax})
cols.update({("refit", i, k, n): [] for i in a.imax for k in Ks for n in a.iters})

for t0 in range(0, a.trials, a.batch):
    nb = min(a.batch, a.trials - t0)
    inp = build_trials(p, t0, nb, seed=a.seed, sweep_idx=0, device=dev)
    args = (wide(inp["subY"]), J.colmajor(inp["Omega"].to(torch.float64)), wide(inp["A"]), wide(inp["B"]))
    prm = (inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())
    zb = wide(inp["Zbar"])
    score = lambda S: torch.as_tensor(J.nmse_spectral_f64(S, zb)).double().cpu().numpy()
    st, st_g, done = None, None, 0
    for i in a.imax:
        S, _, _, st = J.proposed_algorithm_resume_f64(*args, i - done, *prm, want_ce=False, state=st, it0=done)
        Sg, _, _, st_g = J.proposed_algorithm_resume_f64(*args, i - done, *prm, want_ce=False, state=st_g, it0=done, indx_S=inp["indx_S"])
        done = i
        cols[("plain", i)].append(score(S))
        cols[("genie", i)].append(score(Sg))
        order = J.support_order_f64(S) if any(J._lib.SUPPORT_TOP_MAX < k < g for k in Ks) else None
        for k in Ks:
            ix = order[:, :k].contiguous() if J._lib.SUPPORT_TOP_MAX < k < g else None
            for n in a.iters:
                cols[("refit", i, k, n)].append(score(J.refit_f64(*args, S, k, n, a.lam, indx_S=ix)[0]))


def cell(v):
    e = np.concatenate(v)
    return {"mean_nmse": float(e.mean()), "sem": float(e.std(ddof=1) / np.sqrt(e.size)) if e.size > 1 else None}


res = {"tool": "run_refit", "shape": [N, M, Gr, G2], "trials": a.trials, "snr_db": a.snr_db, "seed": a.seed, "lam": a.lam, "K": Ks,
       "iters": a.iters, "results": []}
for i in a.imax:
    row = {"Imax": i, "plain": cell(cols[("plain", i)]), "genie": cell(cols[("genie", i)]), "refit": []}
    for k in Ks:
        for n in a.iters:
            row["refit"].append(dict(K=k, iters=n, **cell(cols[("refit", i, k, n)])))
    res["results"].append(row)
print(json.dumps(res))
if a.out:
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
