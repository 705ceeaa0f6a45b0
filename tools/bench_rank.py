#!/usr/bin/env python3
"""Rate of the rank sweep on one GPU: the six panels of plot_rankR.m (3 points each, --trials realisations per point, 32
singular values kept), after one small warm-up call, and the rate of the float64 numpy restatement (tests/rank_ref.py, the
reference's samplers and numpy's SVD) on a sample.  Prints one JSON line and writes it to --out."""
import argparse, json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from jstsp19_amd import montecarlo as mc

ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=10000)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--numpy-sample", type=int, default=20, help="realisations of the numpy restatement per point")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_bench.json"))
a = ap.parse_args()

mc.run_rank(mc.rank_points(1)[:1], 64, batch=64, sweep0=999)                 # warm-up: library load, first launches
torch.cuda.synchronize()
per = []
t0 = time.perf_counter()
for panel in sorted(mc.RANK_PANELS):
    t1 = time.perf_counter()
    mc.run_rank(mc.rank_points(panel), a.trials, batch=min(a.batch, a.trials), sweep0=500 + 10 * panel)
    torch.cuda.synchronize()
    per.append(time.perf_counter() - t1)
wall = time.perf_counter() - t0
n_real = 6 * 3 * a.trials

import rank_ref as R                                                         # noqa: E402
rng = np.random.default_rng(1)
t1 = time.perf_counter()
for panel in sorted(R.PANELS):
    R.monte_carlo(panel, a.numpy_sample, rng)
np_rate = 18 * a.numpy_sample / (time.perf_counter() - t1)

res = dict(what="plot_rankR (6 panels x 3 points), 32 singular values of the noise-free Y per realisation", trials_per_point=a.trials,
           batch=a.batch, realisations=n_real, wall_s=round(wall, 3), realisations_per_s=round(n_real / wall, 1),
           per_panel_s=[round(x, 3) for x in per], numpy_float64_realisations_per_s=round(np_rate, 1),
           numpy_sample=18 * a.numpy_sample, device=torch.cuda.get_device_name(0))
line = json.dumps(res)
print(line)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
