#!/usr/bin/env python3
"""bench.py — channel-estimates/sec of the batched proposed_algorithm on MI355X.

One "step" = one pass of the hot path over one batch of synthetic Monte-Carlo trials:
`batch` independent proposed_algorithm solves (Imax = 100, 'approximate', all three outputs
S, Y, convergence_error) at BASELINE.json configs[1]:
    Nt = Nr = 64, Nrf (Mr) = 8, K (T) = 64, L = 8  =>  N = 64, M = T*Nt = 4096, Gr = 64, G2 = L*Gt = 512
(symbol binding per SURVEY.md §8), 256 trials per GPU, inputs generated on the device
(jstsp19_amd.system_model, per-trial pilots => per-trial B) and resident in HBM before the
timed region starts.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

Trials shard embarrassingly over ranks (weak scaling: `batch` trials per GPU, global trial
ids keyed into the RNG so inputs do not depend on N); the only collective is one RCCL
all-reduce of the NMSE sum (plus the timing MAX).  Rank 0 prints ONE JSON line.

--dump-outputs DIR writes what the last timed step returned, so that two builds can be compared output for output on the
same inputs (they depend on the arguments only: the generator is keyed by seed and global trial id).

A plain run does what the headline needs and no more: inputs, priming call, warm-up, timed steps, the dump, the mean NMSE,
the line.  --full adds the measurement legs after the timed steps (end_to_end, strict_fp32_mfma, roofline, cpu_baseline,
parity, host_path, configs4); they never touch the timed region, so `value` and `ms_per_step` mean the same in both.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md: dense fp32 matrix peak
HBM_PEAK_GBS = 8000.0              # same guide: HBM3E peak (6.3 TB/s measured achievable)
MFMA_F16_PEAK_TFLOPS = 2500.0      # same guide: dense BF16/FP16 MFMA peak (2495 TF measured with 32x32x16)
# What the f16 pipe SUSTAINS with nothing but MFMAs in flight and uniform-random operands in registers (tools/ubench/mfma_f16_rate.cpp,
# profiles/r05b_mfma_f16_rate.txt: v_mfma_f32_16x16x32_f16, 8 accumulators, two waves per SIMD on all 256 CUs): 1592-1678 TFLOP/s
# over two boxes (the higher one is used here) - 1985-1996 on zero operands, 2459-2476 for 32x32x16 on zeros (the nominal peak),
# 1635-1681 for 32x32x16 on random data; one wave per SIMD: 1332 / 1624.  Reported beside the nominal roof, never instead of it.
MFMA_F16_SUSTAINED_TFLOPS = 1678.0
IMAX = 100
DUMP_LIMIT_BYTES = 64 * 10 ** 6    # --dump-outputs: all files together stay below this
DUMP_SEED = 20190913               # --dump-outputs: the trial sample when the outputs do not fit


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=256, help="Monte-Carlo trials per GPU per step")
    ap.add_argument("--snr-db", type=float, default=5.0)
    ap.add_argument("--no-ce", action="store_true", help="skip convergence_error (2-output call)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, run the measurement legs too: end_to_end, strict_fp32_mfma, roofline, cpu_baseline, "
                         "parity, host_path, configs4 (the --no-* / --cpu-* / --parity-trials options below select among them)")
    ap.add_argument("--cpu-trials", type=int, default=-1,
                    help="--full: trials timed on the host baseline (rank 0, N=1); -1 = three per thread (at most the batch), 0 = none")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="--full: OpenMP threads of the host baseline (0 = min(physical cores, the cgroup's CPU quota))")
    ap.add_argument("--shared-pilots", action="store_true", help="one pilot set for all trials (B shared, stride 0)")
    ap.add_argument("--small", action="store_true", help="reference-native shape (plumbing check)")
    ap.add_argument("--sweep", action="store_true",
                    help="BASELINE configs[3] instead of the headline step: the plot_errorVSsnr sweep at the configs[1] shape, "
                         "10 SNR points x --sweep-trials realisations, (point, trial) pairs sharded over the ranks, ONE "
                         "all-reduce of the NMSE sums (plot_errorVSsnr.m:48-51,170)")
    ap.add_argument("--sweep-trials", type=int, default=500, help="realisations per SNR point in --sweep mode")
    ap.add_argument("--no-host-path", action="store_true", help="skip the JSTSP_HOST (PCIe-inclusive) measurement")
    ap.add_argument("--parity-trials", type=int, default=0,
                    help="--full: besides the bench batch (always checked against the committed float64 fixture), this many trials "
                         "of the configs[3] sweep (10 SNR points, up to 2560) against the same fixture: about 3.5 s per 100")
    ap.add_argument("--no-strict-fp32", action="store_true", help="skip the informational JSTSP_H2=0 (strict complex-fp32 MFMA) rate")
    ap.add_argument("--no-configs4", action="store_true",
                    help="skip the informational BASELINE configs[4] leg (proposed_algorithm_angles at N=64 M=65536 G2=4096, 32 trials, one call)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned (rank 0's trials) as DIR/<name>.npy: S, Y and "
                         "the three columns of convergence_error as convergence_error_V1 / _V2 / _v (--sweep: mean_nmse), complex "
                         "as a trailing (real, imag) axis, at most 64 MB in all (beyond that, the same seeded sample of trials "
                         "from each array)")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be >= 1")
    if not a.full and (a.parity_trials > 0 or a.cpu_trials > 0 or a.cpu_threads > 0):
        ap.error("--parity-trials, --cpu-trials and --cpu-threads size legs that only --full runs")
    return a


def dump_outputs(path, arrays):
    """--dump-outputs: save `arrays` (name -> torch tensor or None, all with the same leading trial axis) as path/<name>.npy in
    float32 / float64, complex as a trailing (real, imag) axis.  When the whole of them exceeds DUMP_LIMIT_BYTES, every array
    keeps the same trials: a sorted sample drawn with DUMP_SEED, so two runs with the same arguments write the same trials.
    Returns what the result line records about the dump."""
    arrays = {k: torch.as_tensor(v) for k, v in arrays.items() if v is not None}
    rows = next(iter(arrays.values())).shape[0]
    per_row = sum(v[0].numel() * v.element_size() for v in arrays.values())
    keep = min(rows, (DUMP_LIMIT_BYTES - 1024 * len(arrays)) // per_row)        # (1 KiB per file for the .npy header)
    if keep < 1:
        raise ValueError("--dump-outputs: one trial of the outputs is larger than %d bytes" % DUMP_LIMIT_BYTES)
    idx = None if keep == rows else np.sort(np.random.default_rng(DUMP_SEED).choice(rows, keep, replace=False))
    os.makedirs(path, exist_ok=True)
    shapes = {}
    for name, v in arrays.items():
        if idx is not None:
            v = v[torch.as_tensor(idx, device=v.device)]
        v = v.detach().cpu()
        if v.is_complex():
            v = torch.view_as_real(v.contiguous())
        x = v.numpy().astype(np.float64 if v.dtype == torch.float64 else np.float32, copy=False)
        np.save(os.path.join(path, name + ".npy"), x)
        shapes[name] = list(x.shape)
    return {"dir": path, "trials": "all" if idx is None else idx.tolist(), "shapes": shapes, "seed": DUMP_SEED}


class HipHooks:
    """What bench.py calls to build inputs, solve and score: the HIP library (the product).  tests/bench_stub.py replaces it
    (JSTSP_BENCH_HOOKS=module:attr, CPU tier only) with a deterministic stand-in over the gloo backend, so that the rank /
    partition / barrier / all-reduce code of THIS file runs under world_size 2 without a GPU (tests/test_bench_gloo.py); a
    line produced that way carries "data": "stub" and is not a measurement."""
    stub = False
    backend = "nccl"

    @staticmethod
    def device(local):
        torch.cuda.set_device(local)
        return torch.device("cuda", local)

    @staticmethod
    def sync():
        torch.cuda.synchronize()

    @staticmethod
    def make_inputs(p, ids, device, shared_pilots):
        return make_inputs(p, ids, device, shared_pilots)

    @staticmethod
    def solve(inp, imax, want_ce):
        import jstsp19_amd as J
        return J.proposed_algorithm(inp["subY"], inp["Omega"], inp["A"], inp["B"], imax, inp["tau_Y"], inp["tau_Z"], inp["rho"],
                                    "approximate", want_ce=want_ce)

    @staticmethod
    def nmse(S, inp):
        import jstsp19_amd as J
        return J.nmse_spectral(S, J.colmajor(inp["Zbar"].to(torch.complex64)))

    @staticmethod
    def sweep_kw():
        return {}


def load_hooks():
    spec = os.environ.get("JSTSP_BENCH_HOOKS")
    if not spec:
        return HipHooks
    import importlib
    mod, attr = spec.split(":")
    return getattr(importlib.import_module(mod), attr)


def launch_ranks(a):
    """`python bench.py --gpus N` without a launcher: start the N rank processes ourselves (torch.distributed.run, one
    per GPU, rendezvous on 127.0.0.1) BEFORE anything touches the GPU, pass their output through and return their exit
    code.  Fails loudly when the node has fewer than N GPUs - it never prints a line with another n_gpus."""
    import socket
    import subprocess
    have = torch.cuda.device_count()            # (does not initialise the GPU on this image)
    if have < a.gpus:
        sys.stderr.write("bench.py: --gpus %d requested but this node has %d GPU(s); not running\n" % (a.gpus, have))
        return 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def make_inputs(p, trial_ids, device, shared_pilots=False):
    """The batch's solver inputs, built in HBM by the library's own kernels (jstsp_build_trials_c32)."""
    from jstsp19_amd.solvers import colmajor
    from jstsp19_amd.system_model import build_trials
    o = build_trials(p, trial_ids[0], len(trial_ids), device=device, shared_pilots=shared_pilots)
    if shared_pilots:
        o["B"] = colmajor(o["B"][0].clone())                   # 2-D => shared dictionary (strideB = 0)
    return dict(subY=o["subY"], Omega=o["Omega"], A=o["A"], B=o["B"], Zbar=o["Zbar"], tau_Y=o["tau_Y"].numpy(),
                tau_Z=o["tau_Z"].numpy(), rho=o["rho"].numpy())


def configs4_leg(device, batch=32):
    """BASELINE configs[4]'s proposed_algorithm_angles (proposed_algorithm_angles.m:36-75) at its full frame - Nt=256 Nr=64 K=256 L=16:
    N=64, M=65 536, Gr=64, G2=4096, ONE pilot set for the batch (the 2-GiB dictionary), inputs built on the device - ONE timed call
    of Imax iterations after a one-iteration priming call.  Informational (the line's metric is configs[1]'s); per GPU: configs[4]
    shards its trials like configs[3]."""
    import jstsp19_amd as J
    from jstsp19_amd.system_model import SweepParams, build_trials
    p4 = SweepParams(Nt=256, Nr=64, L=16, T=256, Mr=8, snr_db=5.0)
    o = build_trials(p4, 0, batch, device=device, shared_pilots=True)
    B = J.colmajor(o["B"][0].clone())
    del o["B"]
    torch.cuda.empty_cache()
    ty, tz, rho = o["tau_Y"].numpy(), o["tau_Z"].numpy(), o["rho"].numpy()
    call = lambda im: J.proposed_algorithm_angles(o["subY"], o["Omega"], o["indx_S"], o["A"], B, im, ty, tz, rho, "approximate", None)
    call(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    S, _, _ = call(IMAX)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    nm = J.nmse_spectral(S, J.colmajor(o["Zbar"].to(torch.complex64)))
    out = {"value": round(batch / dt, 3), "unit": "channel-estimates/s per GPU", "trials": batch, "seconds": round(dt, 4), "Imax": IMAX,
           "mean_nmse": float(nm.mean().item()), "dictionary_block": int(J.default_context(device.index).last_dictionary_block()),
           "workload": "BASELINE configs[4]: proposed_algorithm_angles approximate, Nt=256 Nr=64 K=256 L=16 (N=64 M=65536 Gr=64 G2=4096), "
                       "one pilot set per batch, three outputs",
           "note": "informational; three-kernel iteration, both big contractions through hgemm_pair_kernel (DESIGN.md section 7)"}
    del o, B, S
    torch.cuda.empty_cache()
    return out


def headline_line(a, world, dt, workload, want_ce, mean_nmse, dumped):
    """The line's headline fields, the same in a plain and a --full run (which adds its legs to them)."""
    return {
        "metric": "channel-estimates/sec (batched MC) at Nt=Nr=64,K=64; NMSE vs ref",
        "value": round(a.batch * world * a.steps / dt, 3), "unit": "channel-estimates/s", "n_gpus": world, "steps": a.steps,
        "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "c32 (storage and results fp32 complex; big contractions as split-f16 MFMA with fp32 accumulation, fp32-equivalent)", "data": "synthetic",
        "config": {"workload": workload, "trials_per_gpu_per_step": a.batch, "Imax": IMAX,
                   "outputs": "S,Y,convergence_error" if want_ce else "S,Y", "snr_db": a.snr_db,
                   "pilots": "shared (one B)" if a.shared_pilots else "per-trial (B per trial)", "parallelism": "trials sharded, dp%d" % world},
        "mean_nmse": mean_nmse, "full": a.full, "dump_outputs": dumped,
    }


def emit(line, dist, rank):
    """Rank 0 prints the JSON line as the LAST line of stdout (RCCL writes its banner through C stdio, which is fully
    buffered on a pipe and would otherwise be flushed at exit, after the line)."""
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except OSError:
            pass
        sys.stdout.flush()
        print(json.dumps(line), flush=True)


def sweep_mode(a, rank, world, dist, device, hooks=HipHooks):
    """BASELINE configs[3]: the plot_errorVSsnr.m:48-180 sweep at the configs[1] shape - 10 SNR points x `sweep_trials`
    realisations, each solved by proposed_algorithm (:137) and proposed_algorithm_angles (:144), the (point, trial) pairs
    in contiguous blocks per rank, inputs built on the device, ONE all-reduce of the per-point NMSE sums (:170)."""
    from jstsp19_amd.montecarlo import run_sweep
    from jstsp19_amd.system_model import SweepParams
    if a.small:
        base, snrs = SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4), list(range(-15, 16, 3))      # plot_errorVSsnr.m:8-25
        shape = "reference-native Nr=32 Nt=4 L=4 T=35"
    else:
        base, snrs = SweepParams(Nt=64, Nr=64, L=8, T=64, Mr=8), list(range(-15, 15, 3))
        shape = "Nt=Nr=64 Nrf=8 K=64 L=8 (N=64 M=4096 Gr=64 G2=512)"
    kw = dict(Imax=IMAX, batch=a.batch, device=device, dist=dist, **hooks.sweep_kw())
    run_sweep(base, snrs[:1], min(a.batch, 8) * world, **kw)     # priming: workspace + kernels (setup, not timed)
    hooks.sync()
    if dist is not None:
        dist.barrier()
    hooks.sync()
    t0 = time.perf_counter()
    out = run_sweep(base, snrs, a.sweep_trials, **kw)
    hooks.sync()
    if dist is not None:
        dist.barrier()
    hooks.sync()
    dt = time.perf_counter() - t0
    tmax = torch.tensor([dt], dtype=torch.float64, device=device)
    if dist is not None:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())
    solves = 2 * len(snrs) * a.sweep_trials
    line = None
    if rank == 0:
        dumped = dump_outputs(a.dump_outputs, {"mean_nmse": out}) if a.dump_outputs else None
        line = {"metric": "channel-estimates/sec (batched MC) at Nt=Nr=64,K=64; NMSE vs ref",
                "value": round(solves / dt, 3), "unit": "channel-estimates/s", "n_gpus": world, "steps": 1, "warmup": 0,
                "ms_per_step": round(dt * 1e3, 3), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
                "dtype": "c32", "data": "stub" if hooks.stub else "synthetic",
                "config": {"workload": "plot_errorVSsnr sweep (BASELINE configs[3]): %s, %d SNR points x %d realisations, "
                                       "proposed_algorithm + proposed_algorithm_angles per realisation, Imax=%d, (point, trial) "
                                       "pairs sharded over ranks, one all-reduce of the NMSE sums" % (shape, len(snrs),
                                                                                                   a.sweep_trials, IMAX),
                           "trials_per_call": a.batch, "parallelism": "trials sharded, dp%d" % world},
                "snr_db": snrs, "mean_nmse_proposed": [round(v, 6) for v in out[:, 0].tolist()],
                "mean_nmse_angles": [round(v, 6) for v in out[:, 1].tolist()], "dump_outputs": dumped}
    emit(line, dist, rank)


def main():
    a = parse()
    if a.gpus < 1:
        sys.exit("bench.py: --gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        sys.exit(launch_ranks(a))               # we are the launcher: the ranks are child processes
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus:
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d: launch one rank per GPU (python -m torch.distributed.run "
                 "--nproc-per-node %d ... bench.py --gpus %d), or run `python bench.py --gpus %d` without a launcher"
                 % (a.gpus, world, a.gpus, a.gpus, a.gpus))
    hooks = load_hooks()
    device = hooks.device(local)
    # JSTSP_BENCH_FORCE_DIST=1: initialise the process group even for one rank (exercises the RCCL path on a 1-GPU box)
    if world > 1 or os.environ.get("JSTSP_BENCH_FORCE_DIST"):
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if hooks.backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(hooks.backend)
    else:
        dist = None

    from jstsp19_amd.system_model import SweepParams

    if a.small:   # plot_errorVSsnr.m:8-25
        p = SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4, snr_db=a.snr_db)
        workload = "proposed_algorithm approximate Imax=100, reference-native Nr=32 Nt=4 L=4 T=35 (N=32 M=140 Gr=32 G2=16)"
    else:         # BASELINE.json configs[1]
        p = SweepParams(Nt=64, Nr=64, L=8, T=64, Mr=8, snr_db=a.snr_db)
        workload = "proposed_algorithm approximate Imax=100, Nt=Nr=64 Nrf=8 K=64 L=8 (N=64 M=4096 Gr=64 G2=512)"
    N, M, Gr, G2 = p.solver_shape
    want_ce = not a.no_ce

    if a.sweep:
        sweep_mode(a, rank, world, dist, device, hooks)
        return

    ids = list(range(rank * a.batch, (rank + 1) * a.batch))
    inp = hooks.make_inputs(p, ids, device, a.shared_pilots)

    def step():
        return hooks.solve(inp, IMAX, want_ce)

    def barrier():
        if dist is not None:
            dist.barrier()

    # one-iteration priming call: sizes the library's workspace and loads the kernels (setup, not a step), so that
    # the timing does not depend on --warmup being >= 1
    hooks.solve(inp, 1, want_ce)
    for _ in range(a.warmup):
        out = step()
    hooks.sync()
    barrier()
    hooks.sync()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = step()
    hooks.sync()
    barrier()
    hooks.sync()
    dt = time.perf_counter() - t0
    tmax = torch.tensor([dt], dtype=torch.float64, device=device)
    if dist is not None:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())

    S, Y, ce = out
    dumped = None
    if a.dump_outputs and rank == 0:
        outs = {"S": S, "Y": Y}
        if ce is not None:
            # convergence_error (batch, Imax, 3) holds three quantities per iteration: |V1|^2 / |X|^2 (:67), |V2|^2 / |X|^2 (:69) and
            # the change of v relative to the previous v (:51).  The last one starts from v = 0, so its first entry is Inf in every
            # trial by definition; it is written from iteration 2 on, and every file is finite unless a computed value is not.
            outs.update(convergence_error_V1=ce[:, :, 0], convergence_error_V2=ce[:, :, 1], convergence_error_v=ce[:, 1:, 2])
        dumped = dump_outputs(a.dump_outputs, outs)
    # NMSE per trial (plot_errorVSsnr.m:138-141), one all-reduce of the sum (:170 takes the mean)
    nmse = hooks.nmse(S, inp)
    acc = torch.stack([nmse.sum(), torch.tensor(float(a.batch), dtype=torch.float64, device=device)])
    if dist is not None:
        dist.all_reduce(acc, op=dist.ReduceOp.SUM)
    mean_nmse = float(acc[0] / acc[1])

    if hooks.stub:      # CPU-tier run of this file's distributed plumbing: no library, no measurement legs
        line = None
        if rank == 0:
            line = {"metric": "channel-estimates/sec (batched MC) at Nt=Nr=64,K=64; NMSE vs ref", "value": round(a.batch * world * a.steps / dt, 3),
                    "unit": "channel-estimates/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
                    "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                    "dtype": "stub", "data": "stub", "config": {"workload": workload, "trials_per_gpu_per_step": a.batch},
                    "mean_nmse": mean_nmse, "trial_ids_rank0": [ids[0], ids[-1]], "dump_outputs": dumped}
        emit(line, dist, rank)
        return

    if not a.full:
        emit(headline_line(a, world, dt, workload, want_ce, mean_nmse, dumped) if rank == 0 else None, dist, rank)
        return

    import jstsp19_amd as J
    ctx = J.default_context(device.index)           # (= LOCAL_RANK; tests/bench_stub.py's one-GPU hooks put every rank on device 0)
    extra = {}
    # ---- the metric as SURVEY section 8(d) / BASELINE.md section 3 item 4 define it: solves / wall time of the WHOLE Monte-Carlo
    # step - fresh trials built on the device every step (plot_errorVSsnr.m:57-136: channel, pilots, measurement, hyper-
    # parameters), the solve (:137), the spectral NMSE (:138-141) and the estimate S copied to the host.  The headline `value`
    # above re-solves resident inputs (the contract of this file: inputs in HBM when the timed region starts); `host_path`
    # below is the third variant (host arrays in and out through PCIe, what a MEX call pays).
    e2e_steps = max(1, min(a.steps, 5))
    def e2e_step(k):
        ids_k = list(range((world * (1 + k) + rank) * a.batch, (world * (1 + k) + rank + 1) * a.batch))      # never the resident batch's ids
        inp_k = hooks.make_inputs(p, ids_k, device, a.shared_pilots)
        S_k, _, _ = hooks.solve(inp_k, IMAX, want_ce)
        nm_k = hooks.nmse(S_k, inp_k)
        return S_k.cpu(), float(nm_k.sum().item())          # D2H of S (and of the NMSE sum): both synchronise
    e2e_step(0)                                              # (first build: its kernels and workspace)
    hooks.sync(); barrier(); hooks.sync()
    t1 = time.perf_counter()
    e2e_nmse = 0.0
    for k in range(e2e_steps):
        e2e_nmse += e2e_step(1 + k)[1]
    hooks.sync(); barrier(); hooks.sync()
    e2e_dt = time.perf_counter() - t1
    tm2 = torch.tensor([e2e_dt], dtype=torch.float64, device=device)
    if dist is not None:
        dist.all_reduce(tm2, op=dist.ReduceOp.MAX)
    e2e_dt = float(tm2.item())
    extra["end_to_end"] = {"value": round(a.batch * world * e2e_steps / e2e_dt, 3), "unit": "channel-estimates/s", "steps": e2e_steps,
                           "ms_per_step": round(e2e_dt / e2e_steps * 1e3, 3), "mean_nmse_rank0": e2e_nmse / (a.batch * e2e_steps),
                           "includes": "jstsp_build_trials_c32 (fresh trial ids every step) + proposed_algorithm (Imax=%d, %s) + "
                                       "nmse_spectral + D2H of S" % (IMAX, "three outputs" if want_ce else "two outputs"),
                           "note": "SURVEY section 8(d)'s definition of the metric (the whole Monte-Carlo step); the headline `value` "
                                   "re-solves inputs that are already resident in HBM"}

    # Informational: the same step on the strict complex-fp32 MFMA path (v_mfma_f32_32x32x2_f32 everywhere, JSTSP_H2=0) - what
    # BASELINE.json's north_star literally names.  The headline runs the big contractions as split-f16 MFMA with fp32
    # accumulation (fp32-equivalent: the `dtype` field says so; same float64 parity, see `parity`).
    if not a.small and world == 1 and not a.no_strict_fp32:
        os.environ["JSTSP_H2"] = "0"
        try:
            step(); torch.cuda.synchronize()
            t1 = time.perf_counter()
            step(); torch.cuda.synchronize()
            strict = {"value": round(a.batch / (time.perf_counter() - t1), 1), "unit": "channel-estimates/s",
                      "env": "JSTSP_H2=0", "note": "informational; every contraction on the fp32 matrix pipe (157 TFLOP/s peak)"}
            # its own roofline: one more step with HIP events around the two big contractions of the three-kernel iteration,
            # K B^H (proposed_algorithm.m:47) and (A S) B with the C / V2 update (:58,:61,:65), both cgemm_kernel instances on
            # v_mfma_f32_32x32x2_f32.  Algorithmic flops per launch = 8 N M G2 per trial, priced against
            # the dense fp32-MFMA peak: "complex-fp32 MFMA as specified" beside "split-f16 as shipped" (`roofline` below).
            ctx.set_profiling(True)
            step(); torch.cuda.synchronize()
            prof = {k: ctx.get_profile(k) for k in ("correlate", "synthesize")}
            ctx.set_profiling(False)
            fl = 8.0 * N * M * G2 * a.batch
            rl = {}
            for k, what in (("correlate", "K B^H (:47), Gauss 3-multiplication complex products, fp64 master accumulators"),
                            ("synthesize", "(A S) B + C / V2 update in the epilogue (:58,:61,:65)")):
                n_k, ms_k = prof[k]
                if n_k:
                    avg = ms_k / n_k
                    rl[k] = {"kernel": "cgemm_kernel (v_mfma_f32_32x32x2_f32): " + what, "avg_launch_ms": round(avg, 4), "launches": n_k,
                             "achieved": round(fl / (avg * 1e-3) / 1e12, 1), "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                             "frac": round(fl / (avg * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4), "flops_per_launch": fl}
            if rl:
                dom = max(rl, key=lambda k: rl[k]["avg_launch_ms"])
                strict["roofline"] = dict(rl[dom], bound="mfma", other={k: v for k, v in rl.items() if k != dom})
                # whole-estimate view: SURVEY section 8d counts 262 GFLOP per estimate (2.62 per iteration)
                strict["whole_estimate_tflops"] = round(strict["value"] * 262.0e9 / 1e12, 1)
                strict["whole_estimate_frac_of_fp32_mfma_peak"] = round(strict["value"] * 262.0e9 / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4)
                strict["kernel_table"] = "profiles/r05_strict_fp32_kernel_stats.csv (rocprofv3 --kernel-trace --stats of `JSTSP_H2=0 python bench.py`)"
            extra["strict_fp32_mfma"] = strict
        finally:
            os.environ.pop("JSTSP_H2", None)
            ctx.set_profiling(False)

    # ---- roofline of the dominant kernel: one extra untimed step with HIP events on the launch stream
    ctx.set_profiling(True)
    step()
    torch.cuda.synchronize()
    n_f, ms_f = ctx.get_profile("fused_pass")
    n_l, ms = ctx.get_profile("correlate")
    n_s, ms_s = ctx.get_profile("synthesize")
    ctx.set_profiling(False)
    nB = 1 if a.shared_pilots else a.batch                         # per-trial pilots in the headline workload
    flops_per_launch = 8.0 * N * M * G2 * a.batch              # either contraction, 8 real flops per complex MAC
    # HBM traffic of the same kernels from the committed PMC measurement (separate rocprofv3 --pmc passes,
    # FETCH_SIZE doubled as the microarch guide prescribes for gfx950); only valid for the profiled shape
    pm, pm_src = {}, None
    if not a.small and a.batch == 256:
        for name in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03b_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json"):      # the newest committed measurement
            try:
                with open(os.path.join(ROOT, "profiles", name)) as f:
                    pm = json.load(f)
                pm_src = "profiles/%s (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of `python bench.py` on the build " \
                         "%s; a committed measurement, not collected in this run)" % (name, pm.get("build", "of that round"))
                break
            except (OSError, ValueError):
                pm = {}
    # The PMC passes cannot run inside this process: the figure is a committed measurement.  It is tied to the kernel it was taken
    # on by the hash of csrc/fused.hip recorded with it; when the source has changed since, `traffic` is reported as stale.
    import hashlib
    with open(os.path.join(ROOT, "jstsp19_amd", "csrc", "fused.hip"), "rb") as f:
        fused_hash = hashlib.sha256(f.read()).hexdigest()[:16]
    pm_stale = bool(pm) and pm.get("fused_hip_sha256_16") != fused_hash
    traffic_of = lambda key: pm.get(key, {}).get("hbm_bytes_per_launch")
    roofline = None
    if n_f:
        parts = int(os.environ.get("JSTSP_FUSED_PARTS", "4"))
        avg_f = ms_f / n_f
        gt = ctx.last_dictionary_block()                           # block height of the block-Toeplitz structure found in B (0: none)
        toep = int(os.environ.get("JSTSP_TOEPLITZ", "2"))
        window = gt == 64 and toep >= 2
        # executed MFMA work of the pass: both contractions (8 N G2 M real flops each) as three f16 products (h h + h l + l h)
        # + Y = (I - Q) Z (8 N N M, three products)
        mfma_flop = 3.0 * (2 * flops_per_launch + 8.0 * N * N * M * a.batch)
        mfma = {"executed_tflops": round(mfma_flop / (avg_f * 1e-3) / 1e12, 1), "peak": MFMA_F16_PEAK_TFLOPS,
                "frac": round(mfma_flop / (avg_f * 1e-3) / 1e12 / MFMA_F16_PEAK_TFLOPS, 4),
                "sustained_on_random_operands": {"tflops": MFMA_F16_SUSTAINED_TFLOPS,
                                                 "frac": round(mfma_flop / (avg_f * 1e-3) / 1e12 / MFMA_F16_SUSTAINED_TFLOPS, 4),
                                                 "source": "tools/ubench/mfma_f16_rate.cpp (profiles/r05b_mfma_f16_rate.txt): the same "
                                                           "instruction alone, operands in registers, uniform-random f16 data (1592-1678 over two boxes, the higher used); 1985-1996 on zeros"},
                "note": "v_mfma_f32_16x16x32_f16, split-f16 (three products per fp32-equivalent one); dense f16 peak of "
                        "MI355X_MICROARCH.md"}
        # what the reference's algorithm moves per iteration in this formulation: the whole dictionary once (8 B per complex
        # entry as four f16 planes), the state (X, V1, V2, subY, Z, 1/D read; X, V1, V2, Z written: 76 B per entry of N x M),
        # (A S) fragments and partial sums of K B^H - fused_pass_kernel's bytes, the figure of rounds 2 and 3
        bytes_full = 8.0 * G2 * M * nB + 76.0 * N * M * a.batch + 2.0 * parts * 8.0 * N * G2 * a.batch
        if window:
            # Dominant kernel: fused_pass64_kernel (csrc/fused.hip).  The dictionary of this workload is block-Toeplitz (probed, exact):
            # only block 0 is streamed (8 B per complex entry of Gt x M), Z is formed from X and V1 in the kernel (neither read
            # nor, with convergence_error, written).  Algorithmic bytes per launch =
            #   window image   8 * Gt*M * nB
            # + state: read X, V1, V2, subY (8 B each), 1/D (4 B); write X, V1, V2 (8 B each) [+ Z without convergence_error]
            # + (A S) fragments read once per column range, partial sums of K B^H written     2 * parts * N*G2*8 * batch
            st = 60.0 if not a.no_ce else 68.0
            bytes_pass = 8.0 * gt * M * nB + st * N * M * a.batch + 2.0 * parts * 8.0 * N * G2 * a.batch
            ach = bytes_pass / (avg_f * 1e-3) / 1e9
            hbm = {"achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
                   "bytes_per_launch": bytes_pass}
            full = bytes_full / (avg_f * 1e-3) / 1e9
            kname = ("fused_pass64_kernel ((A S) B, element-wise ADMM updates incl. Y = (I - Q) Z, K B^H in one pass; block-Toeplitz "
                     "dictionary: 20-KiB window of block 0 in LDS, operands of the next tile prefetched into LDS; split-f16 MFMA)")
            # the kernel sits between its two roofs (both within a factor 3): report the nearer one as `bound`, the other beside it
            if mfma["frac"] >= hbm["frac"]:
                roofline = {"bound": "mfma", "kernel": kname, "achieved": mfma["executed_tflops"], "peak": MFMA_F16_PEAK_TFLOPS,
                            "unit": "TFLOP/s", "frac": mfma["frac"], "sustained_on_random_operands": mfma["sustained_on_random_operands"],
                            "hbm": hbm}
            else:
                roofline = {"bound": "hbm", "kernel": kname, **hbm, "mfma": mfma}
            roofline.update({"traffic": traffic_of("fused_pass64"), "avg_launch_ms": round(avg_f, 4), "launches": n_f,
                             "bytes_per_launch": bytes_pass, "dictionary_block": gt,
                             "algorithmic_tflops": round((2 * flops_per_launch + 8.0 * N * N * M * a.batch) / (avg_f * 1e-3) / 1e12, 1),
                             "algorithmic_frac_of_f16_peak": round((2 * flops_per_launch + 8.0 * N * N * M * a.batch) / (avg_f * 1e-3) / 1e12 / MFMA_F16_PEAK_TFLOPS, 4),
                             "algorithmic_note": "8 real flops per complex MAC of (A S) B, K B^H and Y = (I - Q) Z, counted ONCE - `frac` above counts the three f16 "
                                                 "products each fp32-equivalent product is executed as (split-f16); against the 157.3-TFLOP/s fp32 matrix roof "
                                                 "that the same contractions would otherwise run on, the algorithmic rate is %.2f x that roof" % (
                                                     (2 * flops_per_launch + 8.0 * N * N * M * a.batch) / (avg_f * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS),
                             "full_dictionary_equivalent": {"bytes_per_launch": bytes_full, "achieved": round(full, 1), "unit": "GB/s",
                                                            "frac": round(full / HBM_PEAK_GBS, 4),
                                                            "note": "the bytes an unstructured dictionary needs (fused_pass_kernel, the figure "
                                                                    "of rounds 2-3) over this kernel's duration - a speed comparison, "
                                                                    "not traffic"},
                             "note": "section timings (tools/pass_breakdown.py, profiles/r03_pass64_sections.txt): the two product phases run "
                                     "at the MFMA issue rate and take 53 % of a tile, the element-wise section 22 %, Y 11 %, barriers 8 %"})
        else:
            # Dominant kernel: fused_pass_kernel (csrc/fused.hip) - per iteration ONE read of the dictionary: Xs = (A S) B (:58), the
            # V2 / X / V1 / k updates (:61-65, :38-43 of the next iteration, Y = (I - Q) Z formed in the kernel) and the first factor
            # K B^H of the next :47.  HBM-bound by construction (per trial at configs[1]: 16.0 MiB + 19.0 MiB + 2.0 MiB).
            bytes_pass = bytes_full - (8.0 * (G2 - gt) * M * nB if gt else 0.0)
            ach = bytes_pass / (avg_f * 1e-3) / 1e9
            roofline = {"bound": "hbm", "kernel": "fused_pass_kernel ((A S) B, element-wise ADMM updates incl. Y = (I - Q) Z, K B^H: one read of "
                                                  "the dictionary per iteration; split-f16 MFMA, tile in LDS)",
                        "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
                        "traffic": traffic_of("fused_pass"), "avg_launch_ms": round(avg_f, 4), "launches": n_f,
                        "bytes_per_launch": bytes_pass, "dictionary_block": gt, "mfma": mfma,
                        "algorithmic_tflops": round(2 * flops_per_launch / (avg_f * 1e-3) / 1e12, 1),
                        "note": "the three kernels this pass replaces (JSTSP_FUSED=0) run at 0.66-0.68 of the HBM peak each but move "
                                "16.5 GB per iteration instead of 9.9 GB"}
        roofline["traffic_source"] = pm_src if roofline["traffic"] else None
        if roofline["traffic"]:
            roofline["traffic_build"] = {"fused_hip_sha256_16_measured": pm.get("fused_hip_sha256_16"), "fused_hip_sha256_16_now": fused_hash,
                                         "git_sha_measured": pm.get("git_sha"), "stale": pm_stale}
        if roofline["traffic"]:     # measured bytes (PMC) over the same duration: what the memory system actually delivers
            roofline["traffic_rate"] = round(roofline["traffic"] / (avg_f * 1e-3) / 1e9, 1)
            roofline["traffic_frac"] = round(roofline["traffic"] / (avg_f * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
    elif n_s:
        # Three-kernel path (JSTSP_FUSED=0 or a shape the fused pass does not take): dominant kernel hgemm2_kernel<EPI_UPDATE_C>
        # = Xs = (A S) B with the C / V2 update in its epilogue (:58,:61,:65); algorithmic bytes per launch = packed dictionary
        # G2*M*8 * nB + a operand N*G2*8 * batch + epilogue (X read, V2 read + write, Xs write) 4 * N*M*8 * batch
        bytes_synth = 8.0 * G2 * M * nB + 8.0 * N * G2 * a.batch + 4 * 8.0 * N * M * a.batch
        bytes_corr = 8.0 * G2 * M * nB + 8.0 * N * M * a.batch + 8.0 * N * G2 * a.batch     # K B^H: B pack + K + result
        avg_ms = ms_s / n_s
        ach = bytes_synth / (avg_ms * 1e-3) / 1e9
        roofline = {"bound": "hbm", "kernel": "hgemm2_kernel<EPI_UPDATE_C> ((A S) B + C/V2 update, split-f16 MFMA, dictionary HBM -> registers)",
                    "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": traffic_of("synthesize_update_c"),
                    "avg_launch_ms": round(avg_ms, 4), "launches": n_s, "bytes_per_launch": bytes_synth,
                    "algorithmic_tflops": round(flops_per_launch / (avg_ms * 1e-3) / 1e12, 1)}
        if n_l:
            avg_c = ms / n_l
            roofline["correlate"] = {"kernel": "hgemm_kernel<EPI_NONE> (K B^H)", "avg_launch_ms": round(avg_c, 4),
                                     "achieved": round(bytes_corr / (avg_c * 1e-3) / 1e9, 1), "unit": "GB/s",
                                     "frac": round(bytes_corr / (avg_c * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                     "bytes_per_launch": bytes_corr, "traffic": traffic_of("correlate"),
                                     "algorithmic_tflops": round(flops_per_launch / (avg_c * 1e-3) / 1e12, 1)}

    # ---- CPU baseline + parity on a bounded sample (rank 0, single-GPU runs only) -------------
    # cpu_baseline: oracle/cpu_port.cpp - the float64 C++ restatement of proposed_algorithm.m with OpenMP over the trials
    # (the reference's parfor), one trial per core, on `cpu_trials` of the same trials.  The same
    # outputs are the float64 side of the parity check; ONE trial is also solved by the numpy oracle to tie the two.
    cpu = None
    parity = None
    if rank == 0 and world == 1 and not a.no_cpu_baseline and a.cpu_trials != 0:
        import tempfile
        from oracle import build_cpu_port as bp
        from oracle import solvers as O
        ncore = os.cpu_count() or 1
        phys = max(1, ncore // 2)                                  # SMT siblings do not add FMA throughput
        quota = None                                               # CPU time this process may use (cgroup v2 cpu.max)
        try:
            q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
            if q != "max":
                quota = max(1, int(int(q) / int(per)))
        except (OSError, ValueError):
            pass
        nthr = a.cpu_threads or (min(phys, quota) if quota else phys)
        nt = min(a.batch, a.cpu_trials if a.cpu_trials > 0 else min(3 * nthr, 64))     # about 15-20 s of host work
        try:                                                       # tuned for the host it is timed on
            lib = bp.load(bp.build(native=True, out=os.path.join(tempfile.mkdtemp(prefix="jstsp_cpu_"), "libjstsp_cpu_port.so")))
            tuned = "-march=native"
        except (RuntimeError, OSError):
            lib = bp.load()
            tuned = "-march=x86-64-v4 (prebuilt)"
        h = {k: inp[k][:nt].cpu().numpy() for k in ("subY", "Omega", "Zbar")}
        Bh = inp["B"].cpu().numpy() if inp["B"].ndim == 2 else inp["B"][:nt].cpu().numpy()
        A_h = inp["A"].cpu().numpy()
        S_h = S[:nt].cpu().numpy().astype(np.complex128)
        tY, tZ, rh = (np.asarray(inp[k][:nt], dtype=np.float64) for k in ("tau_Y", "tau_Z", "rho"))
        bp.proposed_algorithm(lib, h["subY"][:1], h["Omega"][:1], A_h, Bh if Bh.ndim == 2 else Bh[:1], 2, tY[:1], tZ[:1], rh[:1],
                              want_ce=want_ce, threads=1)          # load + first-touch, not timed
        t0 = time.perf_counter()
        Sc, Yc, cec, used = bp.proposed_algorithm(lib, h["subY"], h["Omega"], A_h, Bh, IMAX, tY, tZ, rh, want_ce=want_ce,
                                                  threads=nthr)
        cdt = time.perf_counter() - t0
        try:
            model = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
        except (OSError, IndexError):
            model = "unknown"
        cpu = {"value": round(nt / cdt, 4), "unit": "channel-estimates/s", "cores": used, "kind": "port",
               "cpu_model": model, "logical_cpus": ncore, "cgroup_cpu_quota": quota, "seconds": round(cdt, 2),
               "sample": "%d of the %d trials of this workload, Imax=%d, ce=%s: float64 C++ structured restatement of "
                         "proposed_algorithm.m (oracle/cpu_port.cpp, %s), OpenMP over trials, one trial per thread, %d "
                         "threads; timing includes the float64 conversion of the inputs (about 2 %%)" % (nt, a.batch, IMAX,
                                                                                                       want_ce, tuned, used)}
        dn = [(O.nmse_capped(S_h[t], h["Zbar"][t]), O.nmse_capped(Sc[t], h["Zbar"][t]),
               float(np.max(np.abs(S_h[t] - Sc[t])) / np.max(np.abs(Sc[t])))) for t in range(nt)]
        parity = {"trials": nt, "against": "oracle/cpu_port.cpp (float64)",
                  "max_abs_dNMSE": float(max(abs(x[0] - x[1]) for x in dn)),
                  "mean_abs_dNMSE": float(np.mean([abs(x[0] - x[1]) for x in dn])),
                  "max_rel_dS": float(max(x[2] for x in dn))}
        if want_ce:
            cg = ce[:nt].cpu().numpy()
            fin = np.isfinite(cec)
            parity["max_rel_dce"] = float(np.max(np.abs(cg[fin] - cec[fin]) / np.abs(cec[fin])))
        # one trial by the numpy oracle (23 s): the C++ port and the line-cited restatement agree at full size
        from threadpoolctl import threadpool_limits
        with threadpool_limits(limits=min(32, ncore)):
            So, _, _ = O.proposed_algorithm(h["subY"][0].astype(np.complex128), h["Omega"][0].astype(np.float64),
                                            A_h.astype(np.complex128), (Bh if Bh.ndim == 2 else Bh[0]).astype(np.complex128),
                                            IMAX, float(tY[0]), float(tZ[0]), float(rh[0]), "approximate", want_ce=False)
        parity["numpy_oracle_vs_cpu_port_rel_dS"] = float(np.max(np.abs(So - Sc[0])) / np.max(np.abs(So)))
        parity["numpy_oracle_abs_dNMSE"] = float(abs(O.nmse_capped(S_h[0], h["Zbar"][0]) - O.nmse_capped(So, h["Zbar"][0])))
        del h, Bh, Sc, Yc

    # ---- parity over the WHOLE batch (and more on request) against the committed float64 fixture: tests/golden/fullsize_port.npz
    # holds oracle/cpu_port.cpp's NMSE for exactly these trials (generator key: seed 20190913, sweep 0, trials 0..255, 5 dB) -
    # computed once on a GPU box's host cores (tools/parity_tail.py), so all 256 cost a second here instead of 90 core-minutes.
    if rank == 0 and world == 1 and not a.small and not a.shared_pilots and a.batch == 256 and a.snr_db == 5.0:
        from oracle.fullsize_fixture import fixture, solve_group
        fx = fixture()
        stat = lambda d: {"trials": int(len(d)), "max_abs_dNMSE": float(np.abs(d).max()), "rms_dNMSE": float(np.sqrt(np.mean(d ** 2))),
                          "p99_abs_dNMSE": float(np.quantile(np.abs(d), 0.99)), "mean_dNMSE": float(d.mean()),
                          "over_1e-6": int(np.sum(np.abs(d) > 1e-6)), "over_5e-7": int(np.sum(np.abs(d) > 5e-7))}
        nm, _ = solve_group(fx, "bench_proposed", np.arange(256), want_ce=want_ce, angles=False)
        d = nm - fx["bench_proposed/nmse_port"]
        full = stat(d)
        full["worst_trials"] = [{"trial": int(t), "dNMSE": float(d[t])} for t in np.argsort(-np.abs(d))[:5]]
        full["against"] = "tests/golden/fullsize_port.npz: float64 oracle/cpu_port.cpp on the same generator keys (hyper-parameters as recorded there)"
        if a.parity_trials > 0:
            n = min(int(a.parity_trials), 2560)
            nb = max(1, n // 64)
            starts = np.linspace(0, 2560 - 64, nb).astype(int) // 64 * 64
            rows = np.unique(np.concatenate([np.arange(s_, s_ + 64) for s_ in starts]))
            nm2, _ = solve_group(fx, "sweep_proposed", rows, want_ce=want_ce, angles=False)
            d2 = nm2 - fx["sweep_proposed/nmse_port"][rows]
            full["sweep"] = stat(d2)
            full["sweep"]["snr_points_db"] = sorted(set(float(x) for x in fx["sweep_proposed/snr_db"][rows]))
            full["sweep"]["worst_trials"] = [{"sweep_idx": int(fx["sweep_proposed/sweep_idx"][rows[t]]), "trial": int(fx["sweep_proposed/trial"][rows[t]]),
                                              "dNMSE": float(d2[t])} for t in np.argsort(-np.abs(d2))[:5]]
        parity = dict(parity or {}, whole_batch=full)
        # the held-out fixtures (other generator seeds; 2560 + 1280 trials each, three- and two-output calls): committed measurements,
        # asserted by tests/test_gpu_parity_tail.py on every GPU test run - not recomputed here.  heldout2 (round 6, seed 20261003) was
        # generated once on the frozen numerics and looked at once; heldout (round 5) has informed a choice of defaults since.
        try:
            with open(os.path.join(ROOT, "profiles", "r06_parity_heldout2.json")) as f:
                h2 = json.load(f)["results"]
            parity["heldout2_fixture"] = {k: {"trials": v["trials"], "max_abs_dNMSE": v["max"], "rms_dNMSE": v["rms"], "p99_abs_dNMSE": v["p99"]}
                                          for k, v in h2.items()}
            parity["heldout2_fixture"]["source"] = "profiles/r06_parity_heldout2.json (committed measurement, first and only look; tests/golden/fullsize_port_heldout2.npz)"
        except (OSError, ValueError, KeyError):
            pass
        try:
            with open(os.path.join(ROOT, "profiles", "r05_parity_heldout_and_setA.json")) as f:
                ho = json.load(f)["runs"]
            parity["heldout_fixture"] = {k[4:]: {"trials": v["results"]["default"]["trials"], "max_abs_dNMSE": v["results"]["default"]["max"],
                                                 "rms_dNMSE": v["results"]["default"]["rms"], "over_1e-6": v["results"]["default"]["over_1e-6"]}
                                         for k, v in ho.items() if k.startswith("r05_heldout")}
            parity["heldout_fixture"]["source"] = "profiles/r05_parity_heldout_and_setA.json (committed measurement of round 5; tests/golden/fullsize_port_heldout.npz)"
        except (OSError, ValueError, KeyError):
            pass

    # ---- the drop-in call: the same trials through JSTSP_HOST (host arrays in and out, PCIe inside the call) --------
    host = None
    if rank == 0 and world == 1 and not a.no_host_path and not a.shared_pilots:
        hs = {k: inp[k].cpu().numpy() for k in ("subY", "Omega", "B")}      # column-major host arrays, as MATLAB holds them
        hA = inp["A"].cpu().numpy()
        gib = sum(v.nbytes for v in hs.values()) / 2 ** 30
        best = None
        for rep in range(2):                                                # (the first call grows the workspace)
            t0 = time.perf_counter()
            So_, Yo_, ceo_ = J.proposed_algorithm(hs["subY"], hs["Omega"], hA, hs["B"], IMAX, inp["tau_Y"], inp["tau_Z"],
                                                  inp["rho"], "approximate", want_ce=want_ce)
            hdt = time.perf_counter() - t0
            best = hdt if best is None else min(best, hdt)
        same = bool(np.array_equal(np.asarray(So_), S.cpu().numpy()))
        host = {"value": round(a.batch / best, 2), "unit": "channel-estimates/s", "seconds": round(best, 4),
                "h2d_gib": round(gib, 3), "d2h_gib": round((So_.nbytes + Yo_.nbytes + (ceo_.nbytes if want_ce else 0)) / 2 ** 30, 3),
                "bit_identical_to_device_call": same,
                "note": "jstsp_proposed_algorithm_c32 with memspace JSTSP_HOST: pageable numpy arrays in (subY, Omega, B per trial), "
                        "S, Y, convergence_error out - what a MEX call pays; never the headline value"}
        del hs

    if rank == 0 and world == 1 and not a.small and not a.no_configs4:
        del inp, out, S, Y, ce
        torch.cuda.empty_cache()
        try:                                    # (informational: whatever happens here, the line's own metric is printed)
            extra["configs4"] = configs4_leg(device)
        except Exception as e:                  # noqa: BLE001
            extra["configs4"] = {"error": "%s: %s" % (type(e).__name__, e)}

    if rank == 0:
        line = headline_line(a, world, dt, workload, want_ce, mean_nmse, dumped)
        line.update(roofline=roofline, cpu_baseline=cpu, parity=parity, host_path=host, **extra)
    emit(line if rank == 0 else None, dist, rank)


if __name__ == "__main__":
    main()
