#!/usr/bin/env python
"""What the runner's pai_prev modes pay per frame for the order of a support: support_order_f64 and
support_order on 256 x (64 x 512), once on a solver's sparse S (proposed_algorithm_resume_f64, Imax 20, with the true indx_S: at
most 110 non-zeros per trial) and once on a dense Zbar, timed by HIP events - beside the only alternative without them, a copy of
S to the host and a stable numpy argsort of -|z|^2 per trial on 16 threads.  In the same run, what the pai_wide_prev modes pay
(DESIGN.md section 9q): support_order_wide_f64 and support_order_wide at Gt = 64 and --widen WR,WT (default 1,1), "neighbourhood"
and "ties".  Prints ONE JSON line; no bound is asserted."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import torch
import jstsp19_amd as J
from jstsp19_amd.system_model import SweepParams, build_trials

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--widen", default="1,1", metavar="WR,WT", help="the radii of the support_order_wide rows")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
a = ap.parse_args()
wr, wt = (int(x) for x in a.widen.split(","))

p = SweepParams(Nt=64, Nr=64, L=8, T=64, Mr=8, snr_db=5.0)                  # BASELINE configs[1]: Gr x G2 = 64 x 512
dev = torch.device("cuda:0")
zbar, sparse = [], []
for t0 in range(0, a.batch, 16):
    nb = min(16, a.batch - t0)
    inp = build_trials(p, t0, nb, device=dev)
    wide = lambda x: J.colmajor(x.to(torch.complex128))
    S = J.proposed_algorithm_resume_f64(wide(inp["subY"]), J.colmajor(inp["Omega"].to(torch.float64)), wide(inp["A"]), wide(inp["B"]), 20,
                                        inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy(), indx_S=inp["indx_S"],
                                        want_ce=False, return_state=False)[0]
    zbar.append(wide(inp["Zbar"]).transpose(1, 2).contiguous())
    sparse.append(S.transpose(1, 2).contiguous())
cat = lambda xs: torch.cat(xs).transpose(1, 2)                              # (batch, Gr, G2), column-major per trial
inputs = {"sparse_S": cat(sparse), "dense_Zbar": cat(zbar)}


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


def host_ms(x):
    """D2H of S, then one stable argsort per trial over a pool of threads (numpy releases the GIL while it sorts)."""
    def one(v):
        return np.argsort(-(v.real * v.real + v.imag * v.imag), kind="stable").astype(np.int32) + 1
    ms, out = [], None
    with ThreadPoolExecutor(a.threads) as ex:
        for _ in range(2 + a.reps):
            torch.cuda.synchronize()
            c0 = time.perf_counter()
            h = x.transpose(1, 2).contiguous().cpu().numpy().reshape(x.shape[0], -1)      # vec(S) per trial
            out = np.stack(list(ex.map(one, h)))
            ms.append(1e3 * (time.perf_counter() - c0))
    return ms[2:], out


def stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
            "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)), "reps": int(ms.size)}


res = {"tool": "support_order_rate", "shape": [64, 512], "batch": a.batch, "threads": a.threads, "widen": [wr, wt], "results": []}
for name, x in inputs.items():
    nnz = float((x != 0).sum(dim=(1, 2)).double().mean())
    narrow = J.colmajor(x.to(torch.complex64))
    hms, href = host_ms(x)
    same = bool(np.array_equal(J.support_order_f64(x).cpu().numpy(), href))
    for label, fn, arg in (("support_order_f64", J.support_order_f64, x), ("support_order", J.support_order, narrow)):
        res["results"].append(dict(input=name, mean_nonzeros_per_trial=nnz, method=label, **stats(device_ms(fn, arg))))
    for primary in ("neighbourhood", "ties"):
        for label, fn, arg in (("support_order_wide_f64", J.support_order_wide_f64, x), ("support_order_wide", J.support_order_wide, narrow)):
            wide = lambda z, fn=fn, primary=primary: fn(z, p.Gt, wr, wt, primary=primary)
            res["results"].append(dict(input=name, mean_nonzeros_per_trial=nnz, method=label, primary=primary,
                                       **stats(device_ms(wide, arg))))
    res["results"].append(dict(input=name, mean_nonzeros_per_trial=nnz, method="d2h_plus_numpy_stable_argsort",
                               equals_support_order_f64=same, **stats(hms)))
print(json.dumps(res))
if a.out:
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
