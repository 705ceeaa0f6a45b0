#!/usr/bin/env python3
"""Times of Alg. 1 in float64 (proposed_algorithm_std_f64) beside the fp32 'std' branch and the host oracle: after a warm-up
call, the median of 5 device-resident calls between two synchronisations.  Cases: tests/std64_problems.py P3; the
reference-native shape (32, 140, 32, 16) at batch 64, Imax 50; BASELINE configs[1] (64, 4096, 64, 512), 4 trials, Imax 10, with
per-trial B - the call inverting its factors itself, and with PB = pinv_f64(B) precomputed (the 512 x 4096 inversions, about
0.1 s each, are why the factors are arguments).  Writes one JSON object (--out) and prints it.

    python tools/bench_std64.py --out build/std64_times.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(f, reps=5):
    f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "std64_times.json"))
    ap.add_argument("--no-oracle", action="store_true", help="skip the host oracle columns")
    a = ap.parse_args()
    import jstsp19_amd as J
    from jstsp19_amd.system_model import SweepParams, TrainingParams, build_trials, build_trials_training
    from oracle import solvers as O
    import std64_problems as P
    dev = torch.device("cuda", 0)
    cm = lambda x: J.colmajor(torch.from_numpy(np.ascontiguousarray(x)).to(dev))
    wide = lambda x: J.colmajor(x.to(torch.complex128))
    res = {"threads": os.environ.get("OMP_NUM_THREADS", "")}

    def case(name, subY, Om, A, B, Imax, tY, tS, rho, pb=False):
        """subY, A, B: complex128 column-major CUDA tensors, Om float64; tY, tS, rho: numpy (batch,)."""
        r = {}
        r["f64_std_s"] = timed(lambda: J.proposed_algorithm_std_f64(subY, Om, A, B, Imax, tY, tS, rho, want_ce=False))
        if pb:
            PB = J.pinv_f64(B)
            r["pinv_f64_B_s"] = timed(lambda: J.pinv_f64(B))
            r["f64_std_PB_given_s"] = timed(lambda: J.proposed_algorithm_std_f64(subY, Om, A, B, Imax, tY, tS, rho, PB=PB, want_ce=False))
        r["f64_approximate_s"] = timed(lambda: J.proposed_algorithm_f64(subY, Om, A, B, Imax, tY, tS, rho, want_ce=False))
        n = lambda x: J.colmajor(x.to(torch.complex64))
        s32 = (n(subY), J.colmajor(Om.to(torch.float32)), n(A), n(B))
        try:
            r["fp32_std_s"] = timed(lambda: J.proposed_algorithm(*s32, Imax, tY, tS, rho, "std", want_ce=False))
        except J.JstspError as e:
            r["fp32_std_s"] = None
            r["fp32_std_refused"] = "code %s" % e.code
        if not a.no_oracle:
            h = [x.cpu().numpy() for x in (subY, Om, A, B)]
            t0 = time.perf_counter()
            for t in range(h[0].shape[0]):
                O.proposed_algorithm(h[0][t], h[1][t], h[2] if h[2].ndim == 2 else h[2][t], h[3] if h[3].ndim == 2 else h[3][t], Imax,
                                     float(tY[t]), float(tS[t]), float(rho[t]), "std", want_ce=False)
            r["host_oracle_s"] = time.perf_counter() - t0
        r["batch"] = int(subY.shape[0])
        res[name] = r

    p = P.problem("P3")
    case("P3 16x40x12x24 batch 5 Imax 20", cm(p["subY"]), cm(p["Omega"]), cm(p["A"]), cm(p["B"]), 20, p["tau_Y"], p["tau_S"], p["rho"])
    inp = build_trials_training(TrainingParams(Nt=4, Nr=32, L=4, T=140, ratio=0.75, snr_db=5.0), 0, 64, device=dev)
    case("refnative 32x140x32x16 batch 64 Imax 50", wide(inp["subY"]), J.colmajor(inp["Omega"].to(torch.float64)), wide(inp["A"]), wide(inp["B"]), 50,
         inp["tau_X"].numpy(), inp["tau_S"].numpy(), inp["rho"].numpy())
    inp = build_trials(SweepParams(Nt=64, Nr=64, L=8, T=64, Mr=8, snr_db=5.0), 0, 4, device=dev)
    case("configs[1] 64x4096x64x512 batch 4 Imax 10 per-trial B", wide(inp["subY"]), J.colmajor(inp["Omega"].to(torch.float64)), wide(inp["A"]),
         wide(inp["B"]), 10, inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy(), pb=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
