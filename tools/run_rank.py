#!/usr/bin/env python3
"""plot_rankR.m on the HIP path: the singular values of the noise-free receive signal Y (Nr x 50) of one panel of the figure
(--panel 1..6: Nr = 32, 64, 128 with 2 clusters x 3 rays, then the same with 3 x 12), one curve of min(Nr, Mr_e) = 32 values
per L = 1, 4, 8, and the index min(Np, L*Nt) + 1 the figure marks.  The reference plots ONE realisation per curve (its mean
over a third dimension acts on a 2-D array); --trials K > 1 gives the curve averaged over K realisations."""
import argparse, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jstsp19_amd import montecarlo as mc

ap = argparse.ArgumentParser()
ap.add_argument("--panel", type=int, choices=sorted(mc.RANK_PANELS), default=1)
ap.add_argument("--trials", type=int, default=1, help="realisations per curve (the reference: 1)")
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--seed", type=int, default=20190913)
ap.add_argument("--dist", action="store_true",
                help="one rank per GPU (start with python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 "
                     "tools/run_rank.py --dist ...): (point, trial) pairs sharded, one all-reduce of the sums")
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

pts = mc.rank_points(a.panel)
t0 = time.perf_counter()
# every panel has its own sweep indices, so that no two of them share draws (the reference draws afresh)
mean, marker = mc.run_rank(pts, a.trials, batch=min(a.batch, a.trials), seed=a.seed, sweep0=500 + 10 * a.panel, dist=dist)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
if dist is not None:
    dist.barrier()
    dist.destroy_process_group()
if rank != 0:
    sys.exit(0)
Nr, clusters, rays = mc.RANK_PANELS[a.panel]
print("plot_rankR panel %d: Nr=%d Mr_e=32 Np=%d T=50, singular values 1..%d of Y, %d realisation(s) per curve"
      % (a.panel, Nr, clusters * rays, mean.shape[1], a.trials))
for p, m, r in zip(pts, mean, marker):
    print("L=%d " % p.L + " ".join("%.6e" % v for v in m))
for p, m, r in zip(pts, mean, marker):
    nxt = "sigma_%d/sigma_1 = %.3g" % (r + 1, m[r] / m[0]) if r < len(m) else "no value beyond it is kept"
    print("marked at L=%d: min(Np, L*Nt) = %d, sigma_%d/sigma_1 = %.3g, %s" % (p.L, r, r, m[r - 1] / m[0], nxt))
print("wall time %.2f s" % dt)
