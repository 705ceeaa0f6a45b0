#!/usr/bin/env python3
"""plot_rankR.m on the HIP path: the singular values of the noise-free receive signal Y (Nr x 50) of one panel of the figure
(--panel 1..6: Nr = 32, 64, 128 with 2 clusters x 3 rays, then the same with 3 x 12), one curve of min(Nr, Mr_e) = 32 values
per L = 1, 4, 8, and the index min(Np, L*Nt) + 1 the figure marks.  The reference plots ONE realisation per curve (its mean
over a third dimension acts on a 2-D array); --trials K > 1 gives the curve averaged over K realisations.

--shape Nr,Nt,L,T_prop[,clusters,rays] computes one curve at a point that is not a panel of the figure, at any size
jstsp_spectrum_trials_c32 takes (min(Nr, T_prop) <= 64 up to 65536 on the long side, or <= 512 up to 8192).  --channel FILE
(.npy / .npz / .mat, (Nr_src, Nt_src, L)) replaces the drawn channel by a supplied one, cut and scaled per --channel-normalize as
tools/run_driver.py does; with a panel, the curve of that panel's Nr whose L is the file's."""
import argparse, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jstsp19_amd import montecarlo as mc

ap = argparse.ArgumentParser()
ap.add_argument("--panel", type=int, choices=sorted(mc.RANK_PANELS), default=1)
ap.add_argument("--trials", type=int, default=1, help="realisations per curve (the reference: 1)")
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--seed", type=int, default=20190913)
ap.add_argument("--shape", default=None, metavar="Nr,Nt,L,T_prop[,clusters,rays]", help="one point instead of a panel")
ap.add_argument("--channel", default=None, metavar="FILE", help="a supplied channel (Nr_src, Nt_src, L) instead of the drawn one")
ap.add_argument("--channel-normalize", default="reference", choices=("asis", "reference", "unit"))
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
H = mc.load_channel(a.channel) if a.channel else None
if a.shape:
    v = [int(x) for x in a.shape.split(",")]
    if len(v) not in (4, 6):
        ap.error("--shape takes Nr,Nt,L,T_prop or Nr,Nt,L,T_prop,clusters,rays")
    Nr, Nt, L, Tp = v[:4]
    clusters, rays = v[4:] if len(v) == 6 else (2, 3)
    pts = [mc.SweepParams(Nt=Nt, Nr=Nr, L=L, T=Tp, Mr=min(4, Nr), Mr_e=min(32, Nr), clusters=clusters, rays=rays, T_prop=Tp)]
elif H is not None:
    pts = [mc.SweepParams(Nt=p.Nt, Nr=p.Nr, L=H.shape[2], T=50, Mr=4, Mr_e=32, clusters=p.clusters, rays=p.rays, T_prop=50) for p in pts[:1]]
if a.shape or H is not None:
    t0 = time.perf_counter()
    mean, marker = mc.run_rank(pts, a.trials, batch=min(a.batch, a.trials), seed=a.seed, sweep0=500 + 10 * a.panel, dist=dist, channel=H,
                               channel_normalize=a.channel_normalize)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rank != 0:
        sys.exit(0)
    p = pts[0]
    print("spectrum of Y: Nr=%d Nt=%d L=%d T=%d, %s, singular values 1..%d, %d realisation(s) per curve"
          % (p.Nr, p.Nt, p.L, p.T_prop, "channel %s (%s)" % (a.channel, a.channel_normalize) if H is not None else
             "Np=%d" % (p.clusters * p.rays), mean.shape[1], a.trials))
    for p, m, r in zip(pts, mean, marker):
        print("L=%d " % p.L + " ".join("%.6e" % x for x in m))
        nxt = "sigma_%d/sigma_1 = %.3g" % (r + 1, m[r] / m[0]) if r < len(m) else "no value beyond it is kept"
        print("marked at L=%d: rank bound %d, %s" % (p.L, r, nxt))
    print("wall time %.2f s" % dt)
    sys.exit(0)
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
