#!/usr/bin/env python3
"""Rate of the capacity / EE sweep on one GPU: the full plot_capacity.m (3 panels x 11 points x --trials realisations, four
designs each) plus plot_ee.m (11 x --trials), after one small warm-up call, and the rate of the float64 numpy restatement
(tests/capacity_ref.py, the reference's samplers) on a sample.  Prints one JSON line and writes it to --out."""
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
ap.add_argument("--numpy-sample", type=int, default=200, help="realisations of the numpy restatement per panel")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capacity_bench.json"))
a = ap.parse_args()

mc.run_capacity(mc.capacity_points(1)[:1], 64, batch=64, sweep0=999)         # warm-up: library load, first launches
torch.cuda.synchronize()
legs = [(p, 100 * p) for p in (1, 2, 3)] + [(2, 400)]                        # the three panels, then plot_ee
per = []
t0 = time.perf_counter()
for panel, sw in legs:
    t1 = time.perf_counter()
    mc.run_capacity(mc.capacity_points(panel), a.trials, batch=min(a.batch, a.trials), sweep0=sw)
    torch.cuda.synchronize()
    per.append(time.perf_counter() - t1)
wall = time.perf_counter() - t0
n_real = len(legs) * 11 * a.trials

import capacity_ref as R                                                     # noqa: E402
rng = np.random.default_rng(1)
t1 = time.perf_counter()
for panel in (1, 2, 3):
    Nr, Mr_e = mc.CAPACITY_PANELS[panel]
    R.monte_carlo(Nr, Mr_e, 16, a.numpy_sample, rng)
np_rate = 3 * a.numpy_sample / (time.perf_counter() - t1)

res = dict(what="plot_capacity (3 panels) + plot_ee, 11 points each, 4 designs per realisation", trials_per_point=a.trials,
           batch=a.batch, realisations=n_real, wall_s=round(wall, 3), realisations_per_s=round(n_real / wall, 1),
           per_leg_s=[round(x, 3) for x in per], numpy_float64_realisations_per_s=round(np_rate, 1),
           numpy_sample=3 * a.numpy_sample, device=torch.cuda.get_device_name(0))
line = json.dumps(res)
print(line)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
