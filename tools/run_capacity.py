#!/usr/bin/env python3
"""plot_capacity.m (--figure capacity: three panels, ASE against the number of RF chains for DBF, HBF-PS, HBF-ZC and the
proposed design) and plot_ee.m (--figure ee: panel 2's shape, + the power model and the energy efficiency) on the HIP path.
Per Mr point one row: Mr, the four mean ASE values (bits/s/Hz) and, for ee, the four powers and the four EE values."""
import argparse, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jstsp19_amd import montecarlo as mc

ap = argparse.ArgumentParser()
ap.add_argument("--figure", choices=("capacity", "ee"), default="capacity")
ap.add_argument("--panels", default="1,2,3", help="capacity: which panels of plot_capacity.m")
ap.add_argument("--trials", type=int, default=10000, help="realisations per point (the reference's maxMCRealizations)")
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--seed", type=int, default=20190913)
ap.add_argument("--dist", action="store_true",
                help="one rank per GPU (start with python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 "
                     "tools/run_capacity.py --dist ...): (point, trial) pairs sharded, one all-reduce of the sums")
a = ap.parse_args()
dist = None
rank = 0
if a.dist:
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    rank = dist.get_rank()

# every panel / figure has its own sweep indices, so that no two of them share draws (the reference draws afresh)
panels = [2] if a.figure == "ee" else [int(x) for x in a.panels.split(",")]
results = []
t0 = time.perf_counter()
for panel in panels:
    pts = mc.capacity_points(panel)
    mean, se = mc.run_capacity(pts, a.trials, batch=min(a.batch, a.trials), seed=a.seed,
                               sweep0=400 if a.figure == "ee" else 100 * panel, dist=dist)
    results.append((panel, pts, mean, se))
torch.cuda.synchronize()
dt = time.perf_counter() - t0
if dist is not None:
    dist.barrier()
    dist.destroy_process_group()
if rank != 0:
    sys.exit(0)
names = " ".join("%11s" % n for n in mc.CAPACITY_DESIGNS)
for panel, pts, mean, se in results:
    Nr, Mr_e = mc.CAPACITY_PANELS[panel]
    if a.figure == "ee":
        print("plot_ee: Nr=%d Mr_e=%d, %d realisations per point" % (Nr, Mr_e, a.trials))
        print("%3s %s | power (mW): %s | EE (bits/Joule): %s" % ("Mr", names, names, names))
    else:
        print("plot_capacity panel %d: Nr=%d Mr_e=%d, %d realisations per point, ASE (bits/s/Hz), max standard error %.2g"
              % (panel, Nr, Mr_e, a.trials, se.max()))
        print("%3s %s" % ("Mr", names))
    for p, m in zip(pts, mean):
        row = "%3d " % p.Mr + " ".join("%11.6f" % v for v in m)
        if a.figure == "ee":
            pw = mc.power_model(p.Nr, p.Mr, p.Mr_e)
            row += " | " + " ".join("%11.4f" % v for v in pw) + " | " + " ".join("%13.6e" % (v / w) for v, w in zip(m, pw))
        print(row.replace(" | ", "   "))
print("wall time %.2f s (%d realisations x 4 designs)" % (dt, len(panels) * 11 * a.trials))
