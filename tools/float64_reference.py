#!/usr/bin/env python3
"""The float64 side of tools/parity_tail.py computed ON THE DEVICE by jstsp_proposed_algorithm_f64.

Same trials as parity_tail.py (BASELINE configs[1] shape N=64, M=4096, Gr=64, G2=512, Imax=100; the SNR points of the
configs[3] sweep x `--trials` realisations, `--bench-trials` of the bench workload at 5 dB, `--angles-trials` of
proposed_algorithm_angles), same options for seed, SNR points, trials and groups, and the same `fixture.npz` layout
(`<group>/snr_db`, `sweep_idx`, `trial`, `fingerprint`, `nmse_port`, `ce_port`, `seed`), so that
tests/golden/make_fullsize_port_fixture.py reads its output unchanged.  `--ls` adds the LS column in float64 per trial
(`S_ls`, `nmse_ls`: `pinv(A_hbf)*Y_hbf*pinv(B_hbf)` by jstsp_ls_f64), `--tssr IMAX,RHO` the TSSR and SVT-based columns
(`S_tssr`, `S_svt`, `nmse_tssr`, `nmse_svt` by tssr_f64: jstsp_mc_svt_f64, jstsp_pinv_f64, jstsp_mmv_omp_f64), `--std IMAX`
Alg. 1 (`S_std`, `nmse_std`: proposed_algorithm 'std' in float64 by jstsp_proposed_std_f64, on the trial's own indx_S in the
_angles groups).  The host port needs 5-6 core-seconds per trial; this
needs milliseconds.  It does not replace parity_tail.py (which measures the fp32 path against the host port) and the committed
fixtures are not regenerated from it.

Prints one JSON line: trials, seconds and trials/s of the device solves (a warm-up call first; every chunk timed on its own
between two synchronisations).  `--host-port N` also solves the first N trials of the first chunk with oracle/cpu_port.cpp
(built for the host's own instruction set, `--threads` threads) and reports its trials/s and the largest |dNMSE| between the two.

    python tools/float64_reference.py --trials 64 --snrs 5 --bench-trials 0 --angles-trials 0 --out build/f64_reference
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMAX = 100


def fingerprint(inp):
    """A few float64 numbers that pin a trial's inputs (as tools/parity_tail.py)."""
    f = torch.stack([inp["subY"].abs().double().sum((1, 2)), inp["B"].abs().double().sum((1, 2)),
                     inp["Omega"].double().sum((1, 2))], 1).cpu().numpy()
    return np.concatenate([f, np.stack([inp[k].numpy() for k in ("tau_Y", "tau_Z", "rho")], 1)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=256, help="realisations per SNR point")
    ap.add_argument("--snrs", type=str, default="-15,-12,-9,-6,-3,0,3,6,9,12")
    ap.add_argument("--bench-trials", type=int, default=256, help="trials of the bench workload (5 dB, sweep index 0)")
    ap.add_argument("--angles-trials", type=int, default=64, help="proposed_algorithm_angles trials per point of --angles-snrs")
    ap.add_argument("--angles-snrs", type=str, default="-15,0,12", help="SNR points (members of --snrs) of the _angles trials")
    ap.add_argument("--seed", type=int, default=20190913)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--no-ce", action="store_true", help="skip convergence_error (ce_port is then absent from the fixture)")
    ap.add_argument("--ls", action="store_true", help="also the float64 least-squares estimate pinv(A_hbf)*Y_hbf*pinv(B_hbf) per trial "
                    "(jstsp_ls_f64): S_ls (complex128, Gr x G2 per trial) and nmse_ls in the fixture")
    ap.add_argument("--tssr", type=str, default="", metavar="IMAX,RHO", help="also the float64 TSSR recipe of plot_errorVSsnr.m:151-162 per trial "
                    "(tssr_f64 with K = 200): S_tssr, S_svt (complex128, Gr x G2 per trial), nmse_tssr and nmse_svt in the fixture")
    ap.add_argument("--std", type=int, default=0, metavar="IMAX", help="also Alg. 1 ('std') in float64 per trial at this Imax "
                    "(proposed_algorithm_std_f64): S_std (complex128, Gr x G2 per trial) and nmse_std in the fixture")
    ap.add_argument("--host-port", type=int, default=0, help="also solve this many trials with oracle/cpu_port.cpp and compare")
    ap.add_argument("--threads", type=int, default=16, help="threads of the host port")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "build", "f64_reference"),
                    help="directory of fixture.npz and rate.json (build/ is not tracked)")
    a = ap.parse_args()

    import jstsp19_amd as J
    from jstsp19_amd.system_model import SweepParams, build_trials
    from oracle import solvers as O

    os.makedirs(a.out, exist_ok=True)
    dev = torch.device("cuda", 0)
    snrs = [float(s) for s in a.snrs.split(",") if s]
    work = []
    for t0 in range(0, a.bench_trials, a.chunk):
        work.append(("bench", "proposed", 5.0, 0, t0, min(a.chunk, a.bench_trials - t0)))
    for t0 in range(0, a.angles_trials, a.chunk):
        for s in [float(x) for x in a.angles_snrs.split(",") if x]:
            if s in snrs:
                work.append(("sweep", "angles", s, snrs.index(s), t0, min(a.chunk, a.angles_trials - t0)))
    for t0 in range(0, a.trials, a.chunk):
        for i, s in enumerate(snrs):
            work.append(("sweep", "proposed", s, i, t0, min(a.chunk, a.trials - t0)))

    def solve(inp, idx):
        hyp = [inp[k].numpy() for k in ("tau_Y", "tau_Z", "rho")]
        S, _, ce = J.proposed_algorithm_f64(inp["subY"], inp["Omega"], inp["A"], inp["B"], IMAX, *hyp, "approximate", indx_S=idx,
                                            want_ce=not a.no_ce)
        torch.cuda.synchronize()
        return S, ce

    groups, secs, trials, host = {}, [], 0, None
    for n, (tag, solver, snr, sidx, t0, cnt) in enumerate(work):
        p = SweepParams(Nt=64, Nr=64, L=8, T=64, Mr=8, snr_db=snr)
        inp = build_trials(p, t0, cnt, seed=a.seed, sweep_idx=sidx, device=dev, with_hbf=a.ls)
        idx = inp["indx_S"] if solver == "angles" else None
        if n == 0:                                  # warm-up: allocations, code objects, clocks
            solve({k: (v[:2] if k != "A" or v.ndim == 3 else v) for k, v in inp.items()}, None if idx is None else idx[:2])
        torch.cuda.synchronize()
        tc = time.perf_counter()
        S, ce = solve(inp, idx)
        secs.append(time.perf_counter() - tc)
        trials += cnt
        Sh = S.cpu().numpy()
        zb = inp["Zbar"].cpu().numpy().astype(np.complex128)
        nm = np.array([O.nmse_capped(Sh[t], zb[t]) for t in range(cnt)])
        g = groups.setdefault(tag + "_" + solver, {})
        rec = {"snr_db": np.full(cnt, snr), "sweep_idx": np.full(cnt, sidx), "trial": np.arange(t0, t0 + cnt), "fingerprint": fingerprint(inp),
               "seed": np.full(cnt, a.seed, dtype=np.int64), "nmse_port": nm}
        if not a.no_ce:
            rec["ce_port"] = ce.cpu().numpy().astype(np.float64)
        if a.ls:                                    # plot_errorVSsnr.m:83 on the conventional-HBF measurement, nothing narrowed
            wide = lambda x: x.to(torch.complex128)
            Sl = J.ls_estimate_f64(wide(inp["Y_hbf"]), wide(inp["A_hbf"]), wide(inp["B_hbf"])).cpu().numpy()
            rec["S_ls"] = np.ascontiguousarray(Sl)
            rec["nmse_ls"] = np.array([O.nmse_capped(Sl[t], zb[t]) for t in range(cnt)])
        if a.tssr:                                  # plot_errorVSsnr.m:151-162 on the proposed scheme's measurement, nothing narrowed
            ti, tr = a.tssr.split(",")
            St, _, Sv = J.tssr_f64(inp["subY"], inp["Omega"], inp["A"], inp["B"], int(ti), inp["tau_Y"].numpy(), float(tr), 200)
            for nm_, Sx in (("tssr", St.cpu().numpy()), ("svt", Sv.cpu().numpy())):
                rec["S_" + nm_] = np.ascontiguousarray(Sx)
                rec["nmse_" + nm_] = np.array([O.nmse_capped(Sx[t], zb[t]) for t in range(cnt)])
        if a.std:                                   # proposed_algorithm.m:29,53 on the same trial, nothing narrowed
            hyp = [inp[k].numpy() for k in ("tau_Y", "tau_Z", "rho")]
            Ss = J.proposed_algorithm_std_f64(inp["subY"], inp["Omega"], inp["A"], inp["B"], a.std, *hyp, indx_S=idx, want_ce=False)[0].cpu().numpy()
            rec["S_std"] = np.ascontiguousarray(Ss)
            rec["nmse_std"] = np.array([O.nmse_capped(Ss[t], zb[t]) for t in range(cnt)])
        for k, v in rec.items():
            g.setdefault(k, []).append(v)
        if n == 0 and a.host_port > 0:
            import tempfile
            from oracle import build_cpu_port as bp
            try:
                lib = bp.load(bp.build(native=True, out=os.path.join(tempfile.mkdtemp(prefix="jstsp_cpu_"), "libjstsp_cpu_port.so")))
            except (RuntimeError, OSError):
                lib = bp.load()
            m = min(a.host_port, cnt)
            hyp = [inp[k].numpy()[:m] for k in ("tau_Y", "tau_Z", "rho")]
            Ah = inp["A"].cpu().numpy()
            th = time.perf_counter()
            Sc, _, _, used = bp.proposed_algorithm(lib, inp["subY"][:m].cpu().numpy(), inp["Omega"][:m].cpu().numpy(), Ah if Ah.ndim == 2 else Ah[:m],
                                                   inp["B"][:m].cpu().numpy(), IMAX, *hyp, indx_S=None if idx is None else idx[:m].cpu().numpy(),
                                                   want_ce=not a.no_ce, threads=a.threads)
            th = time.perf_counter() - th
            nh = np.array([O.nmse_capped(Sc[t], zb[t]) for t in range(m)])
            host = {"host_port_trials": m, "host_port_threads": int(used), "host_port_seconds": th, "host_port_trials_per_s": m / th,
                    "max_abs_dNMSE_device_vs_host_port": float(np.max(np.abs(nh - nm[:m]))),
                    "max_rel_dS_device_vs_host_port": float(max(np.max(np.abs(Sh[t] - Sc[t])) / np.max(np.abs(Sc[t])) for t in range(m)))}
        del inp, S, ce
    fix = {}
    for gname, g in groups.items():
        for k, v in g.items():
            fix[gname + "/" + k] = np.concatenate(v, 0)
    np.savez_compressed(os.path.join(a.out, "fixture.npz"), **fix)
    total = float(np.sum(secs))
    line = {"tool": "float64_reference", "trials": trials, "seconds": total, "trials_per_s": trials / total if total > 0 else 0.0,
            "chunk": a.chunk, "chunk_seconds": [round(s, 4) for s in secs], "convergence_error": not a.no_ce, "seed": a.seed}
    if host:
        line.update(host)
    with open(os.path.join(a.out, "rate.json"), "w") as f:
        json.dump(line, f, indent=1)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
