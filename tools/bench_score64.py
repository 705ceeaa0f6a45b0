#!/usr/bin/env python3
"""Trials per second of the device scoring of float64 estimates (nmse_spectral_f64 / rate_f64) beside montecarlo._score_f64 on the
host for the same operands, at 64 x 512 x 256 (the estimate of BASELINE configs[1], one sweep point's trials) and 32 x 16 x 1024
(the reference-native estimate).  The operands are device-resident, as in the sweeps: the device figure is the call up to a
device synchronise plus the copy of `batch` doubles, the host figure is _score_f64 as the sweep runs it (copy of both operands,
then numpy on the threads the process was given).  Warm-up, repeated timings, median; writes profiles/score64_rate.json.  A
record, not a threshold."""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jstsp19_amd as J
from jstsp19_amd import montecarlo as mc

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--host-threads", type=int, default=16)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "score64_rate.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_score64 needs an MI355X"
torch.set_num_threads(a.host_threads)
dev = torch.device("cuda", 0)
NOISE_VAR = 0.1


def timed(fn):
    for _ in range(a.warmup):
        fn()
    ts = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


results = []
for rows, cols, batch in ((64, 512, 256), (32, 16, 1024)):
    g = torch.Generator(device="cpu").manual_seed(rows * 1000 + cols)
    Z = torch.randn(batch, rows, cols, dtype=torch.complex128, generator=g) * 0.3
    S = Z + 1e-3 * torch.randn(batch, rows, cols, dtype=torch.complex128, generator=g)
    Zd, Sd = J.colmajor(Z.to(dev)), J.colmajor(S.to(dev))
    for metric in ("nmse", "rate"):
        d = lambda: mc._score_f64_device(Sd, Zd, metric, NOISE_VAR)
        h = lambda: mc._score_f64(Sd, Zd, metric, NOISE_VAR)
        err = float(((d() - h()).abs() / h().abs()).max())
        td, th = timed(d), timed(h)
        row = dict(rows=rows, cols=cols, batch=batch, metric=metric, device_trials_per_s=batch / td[0], host_trials_per_s=batch / th[0],
                   device_ms_median=1e3 * td[0], device_ms_min=1e3 * td[1], device_ms_max=1e3 * td[2],
                   host_ms_median=1e3 * th[0], host_ms_min=1e3 * th[1], host_ms_max=1e3 * th[2], max_rel_device_vs_host=err)
        print(json.dumps(row))
        results.append(row)
out = dict(tool="tools/bench_score64.py", gpu=torch.cuda.get_device_name(0), host_threads=a.host_threads, warmup=a.warmup, repeats=a.repeats,
           noise_var=NOISE_VAR, note="operands device-resident; median of `repeats` timings after `warmup` calls, each ended by a device synchronise",
           results=results)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
