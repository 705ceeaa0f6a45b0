#!/usr/bin/env python3
"""The float64 side of BASELINE configs[4] at the reference's Imax = 100 (tests/golden/cfg5_fullframe_port.npz).

configs[4]'s full frame: N = 64, M = 65 536, Gr = 64, G2 = 4096, one pilot set for the batch; the inputs of bench.py's configs4 leg
(SweepParams(Nt=256, Nr=64, L=16, T=256, Mr=8, snr_db=5), seed 20190913, sweep index 0, trials 0-31).  Three phases, each its own
process, so that a phase cut short by a time limit loses nothing:

  inputs   (GPU)  build the 32 trials with the library's generator; write A, a piece of B and the inputs of some trials to --out,
                  with the fingerprint / hyper-parameters of all 32 (a few tens of MiB per run: see phase_inputs).
  solve    (CPU)  oracle.solvers.proposed_algorithm, Imax = 100, three outputs, one trial at a time, B B' formed once for the shared
                  pilots; one file per trial, trials already solved are skipped.  Never initialises HIP.
  (converter)     tests/golden/make_cfg5_fullframe_fixture.py.

The exact commands and the measured cost are in the converter's docstring.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED, SWEEP_IDX, SNR_DB, BATCH, IMAX = 20190913, 0, 5.0, 32, 100


def params():
    from jstsp19_amd.system_model import SweepParams
    return SweepParams(Nt=256, Nr=64, L=16, T=256, Mr=8, snr_db=SNR_DB)


def fingerprint(inp, B0):
    """per trial: sum|subY|, sum|B| (the shared pilot set), sum Omega, tau_Y, tau_Z, rho, sum|Zbar| (float64)."""
    import torch
    b = inp["subY"].shape[0]
    f = torch.stack([inp["subY"].abs().double().sum((1, 2)), B0.abs().double().sum().expand(b),
                     inp["Omega"].double().sum((1, 2))], 1).cpu().numpy()
    h = np.stack([inp[k].numpy() for k in ("tau_Y", "tau_Z", "rho")], 1)
    z = inp["Zbar"].abs().double().sum((1, 2)).cpu().numpy()[:, None]
    return np.concatenate([f, h, z], 1)


def phase_inputs(a):
    """Writes what the float64 side needs in a compact, exact form, in pieces of a few tens of MiB per run (the 2-GiB dictionary
    and the trials are written by several runs into one directory): ``meta.npz`` (fingerprints and hyper-parameters of all 32 trials,
    A, the first L columns of B), ``Bblock_<c0>.npy`` (columns c0:c1 of B's first block row - B is block-Toeplitz, checked here
    entry by entry, so that block is all of B) and ``trial_<t>.npz`` (Omega as bits, subY on the support of Omega - checked to be
    zero elsewhere - Zbar and indx_S(1 : 10 + 5 Imax))."""
    import torch
    import jstsp19_amd as J
    from jstsp19_amd.system_model import build_trials
    os.makedirs(a.out, exist_ok=True)
    p = params()
    inp = build_trials(p, 0, BATCH, seed=SEED, sweep_idx=SWEEP_IDX, device=torch.device("cuda", 0), shared_pilots=True)
    B0 = J.colmajor(inp["B"][0].clone())
    del inp["B"]
    torch.cuda.empty_cache()
    G2, M = B0.shape
    Gt, L = p.Gt, G2 // p.Gt
    for ld in range(1, L):                     # B(ld Gt + g, m) == B(g, m - ld) for m >= ld, bit for bit (proposed_hbf.m:17)
        assert torch.equal(B0[ld * Gt:(ld + 1) * Gt, ld:], B0[:Gt, :M - ld]), "B is not block-Toeplitz"
    np.savez(os.path.join(a.out, "meta.npz"), fingerprint=fingerprint(inp, B0), seed=SEED, sweep_idx=SWEEP_IDX, snr_db=SNR_DB,
             A=inp["A"].cpu().numpy(), Bhead=B0[:, :L].cpu().numpy(), G2=G2, M=M, Gt=Gt)
    if a.b_cols:
        c0, c1 = (int(c) for c in a.b_cols.split(":"))
        np.save(os.path.join(a.out, "Bblock_%05d.npy" % c0), B0[:Gt, c0:c1].cpu().numpy())
    for t in sorted({int(t) for t in a.save_trials.split(",") if t}):
        om, sy = inp["Omega"][t], inp["subY"][t]
        assert bool(((om == 0) | (om == 1)).all()) and bool((sy[om == 0] == 0).all())
        mask = (om == 1).cpu().numpy().reshape(-1, order="F")
        np.savez(os.path.join(a.out, "trial_%02d.npz" % t), Omega_bits=np.packbits(mask),
                 subY_on_Omega=sy.cpu().numpy().reshape(-1, order="F")[mask], Zbar=inp["Zbar"][t].cpu().numpy(),
                 indx_S_head=inp["indx_S"][t, :10 + 5 * IMAX].cpu().numpy())
    print("written to %s: %s" % (a.out, sorted(os.listdir(a.out))), flush=True)


def load_B(out):
    """the dictionary (complex128) from meta.npz and the Bblock_*.npy pieces, checked against the fingerprint's sum|B|."""
    meta = np.load(os.path.join(out, "meta.npz"))
    G2, M, Gt = int(meta["G2"]), int(meta["M"]), int(meta["Gt"])
    L = G2 // Gt
    blk = np.zeros((Gt, M), dtype=np.complex128)
    c = 0
    for f in sorted(f for f in os.listdir(out) if f.startswith("Bblock_")):
        assert int(f[7:12]) == c, "a piece of B is missing before column %d" % c
        piece = np.load(os.path.join(out, f))
        blk[:, c:c + piece.shape[1]] = piece
        c += piece.shape[1]
    assert c == M, "pieces of B cover %d of %d columns" % (c, M)
    B = np.empty((G2, M), dtype=np.complex128, order="F")
    for ld in range(L):
        B[ld * Gt:(ld + 1) * Gt, ld:] = blk[:, :M - ld]
        B[ld * Gt:(ld + 1) * Gt, :ld] = meta["Bhead"][ld * Gt:(ld + 1) * Gt, :ld]
    # (the fingerprint takes |.| of the complex64 entries in fp32: 1e-8 relative from that alone)
    np.testing.assert_allclose(np.abs(B).sum(), meta["fingerprint"][0, 1], rtol=1e-7)
    return B


def load_trial(out, t, N, M):
    z = np.load(os.path.join(out, "trial_%02d.npz" % t))
    mask = np.unpackbits(z["Omega_bits"], count=N * M).astype(bool)
    subY = np.zeros(N * M, dtype=np.complex128)
    subY[mask] = z["subY_on_Omega"]
    return (subY.reshape(N, M, order="F"), mask.astype(np.float64).reshape(N, M, order="F"), z["Zbar"].astype(np.complex128),
            z["indx_S_head"])


def phase_solve(a):
    from threadpoolctl import threadpool_limits
    from oracle import solvers as O
    meta = np.load(os.path.join(a.out, "meta.npz"))
    fp = meta["fingerprint"]
    work = []                                           # (solver, trial)
    for item in a.trials.split():
        solver, ts = item.split(":")
        work += [(solver, int(t)) for t in ts.split(",")]
    todo = [(s, t) for s, t in work if not os.path.exists(os.path.join(a.out, "port_%s_%02d.npz" % (s, t)))]
    if not todo:
        print("nothing to do", flush=True)
        return
    t_start = time.perf_counter()
    with threadpool_limits(limits=a.threads):
        A = meta["A"].astype(np.complex128)
        B = load_B(a.out)
        Bh = B.conj().T
        tg = time.perf_counter()
        GB = B @ Bh
        t_gb = time.perf_counter() - tg
        print("B B' formed in %.1f s on %d threads" % (t_gb, a.threads), flush=True)
        for solver, t in todo:
            if time.perf_counter() - t_start > a.budget_s:
                break
            subY, Omega, Zbar, head = load_trial(a.out, t, A.shape[0], B.shape[1])
            np.testing.assert_allclose([np.abs(subY).sum(), Omega.sum(), np.abs(Zbar).sum()], fp[t, [0, 2, 6]], rtol=1e-7)
            ty, tz, rho = (float(x) for x in fp[t, 3:6])
            # (indx_S beyond its first 10 + 5 Imax entries is never read: proposed_algorithm_angles.m:36)
            idx = head if solver == "angles" else None
            tc = time.perf_counter()
            S, _, ce = O.proposed_algorithm(subY, Omega, A, B, a.imax, ty, tz, rho, "approximate", indx_S=idx, want_ce=True,
                                            Bh=Bh, GB=GB)
            dt = time.perf_counter() - tc
            nm = O.nmse_capped(S, Zbar)
            np.savez(os.path.join(a.out, "port_%s_%02d%s.npz" % (solver, t, "" if a.imax == IMAX else "_imax%d" % a.imax)),
                     S=S, ce=ce, nmse=nm, trial=t, imax=a.imax, seconds=dt, gb_seconds=t_gb, threads=a.threads)
            print(json.dumps({"solver": solver, "trial": t, "imax": a.imax, "nmse": nm, "seconds": round(dt, 1),
                              "threads": a.threads}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("phase", choices=("inputs", "solve"))
    ap.add_argument("--out", required=True, help="directory of the inputs and of the per-trial float64 results")
    ap.add_argument("--save-trials", default="", help="inputs: trials whose arrays are written, e.g. 0,1,9")
    ap.add_argument("--b-cols", default="", help="inputs: columns c0:c1 of B's first block row to write")
    ap.add_argument("--trials", default="angles:0 proposed:0", help="solve: e.g. 'angles:0,1,9 proposed:0'")
    ap.add_argument("--imax", type=int, default=IMAX, help="solve: fewer iterations only to time a trial")
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--budget-s", type=float, default=1e9, help="solve: start no trial after this many seconds")
    a = ap.parse_args()
    phase_inputs(a) if a.phase == "inputs" else phase_solve(a)


if __name__ == "__main__":
    main()
