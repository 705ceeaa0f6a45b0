#!/usr/bin/env python
"""What the refresh inside the fp32 ADMM costs, at BASELINE configs[1] (64 x 512 x 64 x 512), 256 trials,
Imax 100, device arrays:
  * proposed_algorithm_resume (the plain resumed call from zero) beside proposed_algorithm_refresh at (start, period) = (0, 1) - a
    refresh in every iteration - and (0, 10), in estimates/s, with and without convergence_error (with it the gradient step runs
    beside a resident eigen-decomposition), the calls alternating, wall time around a synchronised call;
  * support_top beside support_order on the v of a solver state (Imax 5, no mask), in microseconds per trial at count 110 and
    4096, by HIP events around one call for the batch; every list is checked against the head of the full order.
JSTSP_LIB names another build of the library (as tools/f32_frame_bits.py).  Prints ONE JSON line; no bound is asserted."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jstsp19_amd import _lib
if os.environ.get("JSTSP_LIB"):
    _lib.LIB_PATH = os.environ["JSTSP_LIB"]
import numpy as np
import torch
import jstsp19_amd as J
from jstsp19_amd.system_model import SweepParams, build_trials

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--imax", type=int, default=100)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--policies", nargs="+", default=["0,1", "0,10"], metavar="START,PERIOD")
ap.add_argument("--counts", type=int, nargs="+", default=[110, 4096])
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
a = ap.parse_args()

p = SweepParams(Nt=64, Nr=64, L=8, T=64, Mr=8, snr_db=5.0)                  # BASELINE configs[1]
N, M, Gr, G2 = p.solver_shape
dev = torch.device("cuda:0")
inp = build_trials(p, 0, a.batch, device=dev)
args = (inp["subY"], inp["Omega"], inp["A"], inp["B"])
prm = (inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())
policies = [tuple(int(x) for x in s.split(",")) for s in a.policies]


def timed(fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


res = {"tool": "bench_refresh32", "library": os.environ.get("JSTSP_LIB", "in-tree"), "shape": [N, M, Gr, G2], "batch": a.batch,
       "Imax": a.imax, "solver": [], "selection": []}
for want_ce in (False, True):
    calls = [("resume", lambda: J.proposed_algorithm_resume(*args, a.imax, *prm, want_ce=want_ce, return_state=False))]
    for s, q in policies:
        calls.append(("refresh %d,%d" % (s, q), lambda s=s, q=q: J.proposed_algorithm_refresh(*args, a.imax, *prm, start=s, period=q,
                                                                                          want_ce=want_ce, return_state=False)))
    for _, fn in calls:                                                     # warm-up: workspace, packs, tuning
        fn()
    secs = {name: [] for name, _ in calls}
    for _ in range(a.reps):                                                 # alternating
        for name, fn in calls:
            secs[name].append(timed(fn))
    base = float(np.median(secs["resume"]))
    for name, _ in calls:
        med = float(np.median(secs[name]))
        res["solver"].append({"call": name, "want_ce": want_ce, "estimates_per_s": a.batch / med,
                              "runs_estimates_per_s": [a.batch / x for x in secs[name]], "rate_relative_to_resume": base / med})

st = J.proposed_algorithm_resume(*args, 5, *prm, want_ce=False)[3]
v = st[:, 4 * N * M:4 * N * M + Gr * G2].contiguous().reshape(a.batch, G2, Gr).transpose(1, 2)      # (batch, Gr, G2), column-major


def device_us_per_trial(fn):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return 1e3 * float(np.median(ms)) / a.batch


full = J.support_order(v)
res["selection"].append({"method": "support_order", "us_per_trial": device_us_per_trial(lambda: J.support_order(v))})
for count in a.counts:
    same = bool(torch.equal(J.support_top(v, count), full[:, :count]))
    res["selection"].append({"method": "support_top", "count": count, "equals_head_of_support_order": same,
                             "us_per_trial": device_us_per_trial(lambda: J.support_top(v, count))})
print(json.dumps(res))
if a.out:
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
