#!/usr/bin/env python
"""What the refresh inside the float64 ADMM pays for its order: support_top_f64 at counts 110, 510 and 4096
beside support_order_f64 in the same session, on 256 x (64 x 512) - once on a solver's dense v (what the loop hands the kernel:
proposed_algorithm_resume_f64, Imax 5, no mask) and once on a solver's sparse S (Imax 20 with the true indx_S: 110 non-zeros, so
counts above 110 end inside the tie class of exact zeros) - timed by HIP events around one call for the batch.  Every list is
checked against the head of the full order.  Prints ONE JSON line; no bound is asserted."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import jstsp19_amd as J
from jstsp19_amd.system_model import SweepParams, build_trials

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--counts", type=int, nargs="+", default=[110, 510, 4096])
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
a = ap.parse_args()

p = SweepParams(Nt=64, Nr=64, L=8, T=64, Mr=8, snr_db=5.0)                  # BASELINE configs[1]: Gr x G2 = 64 x 512
N, M, Gr, G2 = p.solver_shape
dev = torch.device("cuda:0")
dense, sparse = [], []
for t0 in range(0, a.batch, 16):
    nb = min(16, a.batch - t0)
    inp = build_trials(p, t0, nb, device=dev)
    wide = lambda x: J.colmajor(x.to(torch.complex128))
    args = (wide(inp["subY"]), J.colmajor(inp["Omega"].to(torch.float64)), wide(inp["A"]), wide(inp["B"]))
    prm = (inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())
    st = J.proposed_algorithm_resume_f64(*args, 5, *prm, want_ce=False)[3]
    dense.append(st[:, 4 * N * M:4 * N * M + Gr * G2].contiguous().reshape(nb, G2, Gr))
    S = J.proposed_algorithm_resume_f64(*args, 20, *prm, indx_S=inp["indx_S"], want_ce=False, return_state=False)[0]
    sparse.append(S.transpose(1, 2).contiguous())
cat = lambda xs: torch.cat(xs).transpose(1, 2)                              # (batch, Gr, G2), column-major per trial
inputs = {"dense_v": cat(dense), "sparse_S": cat(sparse)}


def device_ms(fn, x):
    for _ in range(a.warmup):
        fn(x)
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(x)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
            "us_per_trial": float(1e3 * np.median(ms) / a.batch), "reps": int(ms.size)}


res = {"tool": "support_top_rate", "shape": [Gr, G2], "batch": a.batch, "results": []}
for name, x in inputs.items():
    nnz = float((x != 0).sum(dim=(1, 2)).double().mean())
    full = J.support_order_f64(x)
    res["results"].append(dict(input=name, mean_nonzeros_per_trial=nnz, method="support_order_f64", **stats(device_ms(J.support_order_f64, x))))
    for count in a.counts:
        same = bool(torch.equal(J.support_top_f64(x, count), full[:, :count]))
        res["results"].append(dict(input=name, mean_nonzeros_per_trial=nnz, method="support_top_f64", count=count,
                                   equals_head_of_support_order_f64=same, **stats(device_ms(lambda z: J.support_top_f64(z, count), x))))
print(json.dumps(res))
if a.out:
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
