#!/usr/bin/env python
"""What the stopping rule of proposed_algorithm_until (fp32) saves: BASELINE configs[1] (Nt = Nr = 64, L = 8,
T = 64, Mr = 8), 256 trials built by the library at 5 dB, complex64, Imax = 100, no convergence_error, tol in {1e-3, 1e-4, 1e-5}.
The sibling of tools/bench_until64.py.  Per tol:

  iters                    the distribution of the iterations the trials ran (min, quartiles, mean, max, how many reached Imax)
  until_check{1,2,4,8,16}  estimates/s of the new entry at each check
  resume_at_max            estimates/s of proposed_algorithm_resume - the code without the rule - at Imax = max(iters)
  resume_at_mean           the same at Imax = round(mean(iters))
  given_back_check{..}     (t_until - t_ideal) / (t_full - t_ideal): the share of the saved time that the stop tests, captures,
                           synchronisations and - the fp32 batch is not compacted - the iterations between mean(iters) and the
                           loop's exit give back, with t_full the resumed solve at Imax = 100 and t_ideal = t_full * mean(iters) / 100
and once, as "hook": the entry at tol = 1e-30, which no trial reaches, against the resumed solve at Imax = 100 - the price of Y
stored by every iteration, the tests, the captures and the synchronisations (check = 1 and the largest check).

Every time is the median of --reps solves after one warm-up; the stream is synchronised around each.  Prints ONE JSON line and
writes it to --out (default profiles/until64_rate.json).  No threshold is asserted."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import jstsp19_amd as J
from jstsp19_amd.system_model import SweepParams, build_trials

ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=256)
ap.add_argument("--imax", type=int, default=100)
ap.add_argument("--tols", type=float, nargs="+", default=[1e-3, 1e-4, 1e-5])
ap.add_argument("--checks", type=int, nargs="+", default=[1, 2, 4, 8, 16])
ap.add_argument("--min-iters", type=int, default=2)
ap.add_argument("--snr-db", type=float, default=5.0)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--seed", type=int, default=20190913)
ap.add_argument("--small", action="store_true", help="Nt=4, Nr=32, L=4, T=35, Mr=4 instead of BASELINE configs[1]")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "until32_rate.json"))
a = ap.parse_args()

dev = torch.device("cuda:0")
p = SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4, snr_db=a.snr_db) if a.small else SweepParams(Nt=64, Nr=64, L=8, T=64, Mr=8, snr_db=a.snr_db)
inp = build_trials(p, 0, a.trials, seed=a.seed, sweep_idx=0, device=dev)
args = (inp["subY"], inp["Omega"], inp["A"], inp["B"])
prm = (inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())


def timed(fn):
    fn()
    ts = []
    for _ in range(a.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def resume(imax):
    return timed(lambda: J.proposed_algorithm_resume(*args, imax, *prm, want_ce=False, return_state=False))[0]


t_full = resume(a.imax)
res = {"tool": "bench_until32", "shape": list(p.solver_shape), "trials": a.trials, "Imax": a.imax, "min_iters": a.min_iters, "snr_db": a.snr_db,
       "seed": a.seed, "reps": a.reps, "resume_at_Imax": {"seconds": t_full, "estimates_per_s": a.trials / t_full}, "results": []}
# (unmeasured solves first, as tools/bench_until64.py: the first calls at a new workspace size run slow)
for _ in range(2):
    J.proposed_algorithm_until(*args, a.imax, *prm, tol=a.tols[0], min_iters=a.min_iters, check=a.checks[0], return_state=False)
for tol in a.tols:
    row = {"tol": tol}
    for check in a.checks:
        t, out = timed(lambda: J.proposed_algorithm_until(*args, a.imax, *prm, tol=tol, min_iters=a.min_iters, check=check,
                                                              return_state=False))
        it = out[5].cpu().numpy()
        if "iters" not in row:
            q = np.percentile(it, [25, 50, 75])
            row["iters"] = {"min": int(it.min()), "q25": float(q[0]), "median": float(q[1]), "q75": float(q[2]), "mean": float(it.mean()),
                            "max": int(it.max()), "at_Imax": int((it == a.imax).sum())}
            mean_it = float(it.mean())
        else:
            assert np.array_equal(it, first_it)                 # check never changes a result
        first_it = it
        t_ideal = t_full * mean_it / a.imax
        row["until_check%d" % check] = {"seconds": t, "estimates_per_s": a.trials / t}
        row["given_back_check%d" % check] = (t - t_ideal) / (t_full - t_ideal) if t_full > t_ideal else None
    for name, imax in (("resume_at_max", row["iters"]["max"]), ("resume_at_mean", int(round(row["iters"]["mean"])))):
        t = resume(imax)
        row[name] = {"Imax": imax, "seconds": t, "estimates_per_s": a.trials / t}
    res["results"].append(row)

hook = {}
for check in (a.checks[0], a.checks[-1]):
    t, out = timed(lambda: J.proposed_algorithm_until(*args, a.imax, *prm, tol=1e-30, min_iters=a.min_iters, check=check, return_state=False))
    assert int(out[5].min()) == a.imax
    hook["check%d" % check] = {"seconds": t, "estimates_per_s": a.trials / t, "over_resume_at_Imax": t / t_full - 1.0}
res["hook"] = hook
print(json.dumps(res))
if a.out:
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
