#!/usr/bin/env python3
"""Rates of the spectrum entries on one GPU (jstsp_spectrum_c32 / _c64 / jstsp_spectrum_trials_c32, csrc/svdvals.hip), after one
warm-up call per shape, device-resident operands, a host clock around calls that end in a device synchronise:

  - 64 x 4096 (BASELINE configs[1] / [3]), batch 256 and 4096, complex64 and complex128: matrices/s, beside the time one read of
    the operand from HBM would take at the 6.3 TB/s a streaming copy reaches on this chip - the route reads the operand twice
    (the scale pre-pass and the QR), the second time mostly from the caches, and is bound by the Householder updates in LDS,
    not by that read: the ratio says how far;
  - the trial sweep at the configs[1] shape (Nt = Nr = 64, L = 8, Y is 64 x 4096), Y formed entry by entry on load;
  - one call at 64 x 65536 (configs[4]), batch 8;
  - 128 x 128 (configs[2]), batch 1024, the global-memory route;
  - numpy.linalg.svd in float64 on this host's threads at 64 x 4096, for scale.
Prints one JSON line and writes it to --out."""
import argparse, json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import jstsp19_amd as J
from jstsp19_amd import montecarlo as mc
from jstsp19_amd.system_model import spectrum_trials

HBM_BYTES_PER_S = 6.3e12        # a float4 copy on MI355X (peak 8.0e12)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--numpy-sample", type=int, default=8)
ap.add_argument("--sweep-batch", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_bench.json"))
a = ap.parse_args()
dev = torch.device("cuda:0")


def operand(batch, rows, cols, dt):
    g = torch.Generator(device=dev).manual_seed(rows * 7 + cols)
    re = torch.randn((batch, cols, rows, 2), generator=g, device=dev, dtype=torch.float32 if dt == torch.complex64 else torch.float64)
    return torch.view_as_complex(re).transpose(1, 2)                 # column-major per matrix


def timed(fn):
    fn()
    torch.cuda.synchronize()                                         # warm-up of this shape
    best = float("inf")
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, hbm_bytes_per_s_assumed=HBM_BYTES_PER_S, matrices=[])
for rows, cols, batches in ((64, 4096, (256, 4096)), (64, 65536, (8,)), (128, 128, (1024,))):
    for dt in (torch.complex64, torch.complex128):
        for batch in batches:
            Y = operand(batch, rows, cols, dt)
            t = timed(lambda: J.spectrum(Y))
            nbytes = Y.numel() * Y.element_size()
            res["matrices"].append(dict(rows=rows, cols=cols, batch=batch, dtype=str(dt).split(".")[1], seconds=round(t, 6),
                                        matrices_per_s=round(batch / t, 1), operand_read_s=round(nbytes / HBM_BYTES_PER_S, 6),
                                        ratio_to_one_read=round(t / (nbytes / HBM_BYTES_PER_S), 1)))
            del Y
p = mc.SweepParams(Nt=64, Nr=64, L=8, T=64, Mr=8, Mr_e=64)
assert p.T_prop == 4096
t = timed(lambda: spectrum_trials(p, 0, a.sweep_batch, seed=1, sweep_idx=0, n_keep=64))
res["sweep_configs1"] = dict(Nr=64, Nt=64, L=8, T_prop=4096, batch=a.sweep_batch, seconds=round(t, 6), trials_per_s=round(a.sweep_batch / t, 1),
                             complex_macs_per_entry=p.L * p.Nt)
rng = np.random.default_rng(1)
Yh = rng.standard_normal((a.numpy_sample, 64, 4096)) + 1j * rng.standard_normal((a.numpy_sample, 64, 4096))
t0 = time.perf_counter()
np.linalg.svd(Yh, compute_uv=False)
res["numpy_float64_64x4096_matrices_per_s"] = round(a.numpy_sample / (time.perf_counter() - t0), 1)
res["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
line = json.dumps(res)
print(line)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
