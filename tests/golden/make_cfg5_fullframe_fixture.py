#!/usr/bin/env python3
"""tests/golden/cfg5_fullframe_port.npz from the output of tools/cfg5_imax100_fixture.py: BASELINE configs[4]'s full frame
(N=64, M=65 536, Gr=64, G2=4096, one pilot set), the inputs of bench.py's configs4 leg (seed 20190913, sweep index 0, 5 dB,
trials 0-31), solved in float64 by oracle.solvers.proposed_algorithm at Imax = 100 with three outputs.

    # (a) on an MI355X, one run per piece (each writes a few tens of MiB): the library's generator builds the 32 trials (13 s)
    #     and writes a quarter of the first block row of B, the inputs of some trials to solve and the fingerprints of all 32
    for piece in "0:16384 0,1,19" "16384:32768 9,16,31" "32768:49152 2,3,4,5,6,7" "49152:65536 8,10,11,12,17,18"; do
        set -- $piece
        timeout -k 10 300 python tools/cfg5_imax100_fixture.py inputs --b-cols $1 --save-trials $2 --out DIR
    done
    # (b) on any host, never touching HIP: one file per trial, trials already solved are skipped (re-run to resume); these
    #     lists were stopped when the time given to them ran out (what finished is listed below)
    python tools/cfg5_imax100_fixture.py solve --out DIR --threads 4 --trials 'angles:0,19,9'  &
    python tools/cfg5_imax100_fixture.py solve --out DIR --threads 4 --trials 'proposed:0 angles:1,16'  &
    python tools/cfg5_imax100_fixture.py solve --out DIR --threads 2 --trials 'proposed:1 angles:31'  &
    python tools/cfg5_imax100_fixture.py solve --out DIR --threads 4 --trials 'angles:2,4,6,8,10'       # (as the first two end)
    python tools/cfg5_imax100_fixture.py solve --out DIR --threads 4 --trials 'angles:3,5,7,11,12'
    # (c) here
    python tests/golden/make_cfg5_fullframe_fixture.py DIR

Measured cost of (b) on an 8-core host: B B' (8.8 TFLOP, once per process) 28 s on 4 threads; one trial of Imax = 100 (three
outputs) 467 s on 4 threads with two solves side by side, 626-805 s with three (4, 4 and 2 threads).  One iteration is two
137-GFLOP contractions plus the SVD of the 64 x 65 536 iterate and the two spectral norms of the convergence record (0.9 s each,
hardly faster on more threads).  All 40 trials would be about 4 hours of that host: the fixture holds the trials solved in the
time given to it - proposed_algorithm_angles trials 0, 1, 2, 3, 19 and 31, proposed_algorithm trials 0 and 1 - chosen so
that the test's calls put fixture trials in both halves of a pair (0, 1), into both calls of 16 and into the lone last pair of
the odd batch 3-19 (trial 19).  Adding trials: fetch their inputs with (a), solve them with (b), convert again.

Contents (data only):
  fingerprint (32, 7)   per trial of the batch: sum|subY|, sum|B|, sum Omega, tau_Y, tau_Z, rho, sum|Zbar| - the test rebuilds
                        the trials and checks them; the hyper-parameters are the ones the float64 side was given
  seed, sweep_idx, snr_db, imax
  angles/trial, proposed/trial           the generator's trial index of each solved trial
  */nmse_port                            float64 O.nmse_capped of the float64 S
  */ce_port (n, 100, 3)                  float32 convergence_error of the float64 solve
  angles/indx_S_head (n, 510)            indx_S(1 : 10 + 5 Imax) of the trial (1-based): every nonzero of S lies there
  angles/S_head (n, 510)                 complex128 S at those positions - all of S
  proposed/S_idx, proposed/S_val (n, k)  0-based column-major linear index and complex128 value of the nonzeros of S (the
                                         16 384 largest if there are more; padded with -1 / 0), proposed/S_nnz, proposed/S_absmax
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KEEP = 16384


def main(src):
    meta = np.load(os.path.join(src, "meta.npz"))
    imax = 100
    out = {"fingerprint": meta["fingerprint"], "seed": meta["seed"], "sweep_idx": meta["sweep_idx"], "snr_db": meta["snr_db"],
           "imax": np.int64(imax)}
    ports = {}
    for f in sorted(os.listdir(src)):
        if f.startswith("port_") and f.count("_") == 2:
            solver, t = f[5:-4].split("_")
            ports.setdefault(solver, []).append((int(t), np.load(os.path.join(src, f))))
    head = 10 + 5 * imax
    for solver, rows in ports.items():
        rows.sort(key=lambda r: r[0])
        g = solver + "/"
        out[g + "trial"] = np.array([t for t, _ in rows], dtype=np.int32)
        out[g + "nmse_port"] = np.array([float(z["nmse"]) for _, z in rows])
        out[g + "ce_port"] = np.stack([z["ce"] for _, z in rows]).astype(np.float32)
        if solver == "angles":
            ix = np.stack([np.load(os.path.join(src, "trial_%02d.npz" % t))["indx_S_head"][:head] for t, _ in rows]).astype(np.int32)
            Sv = np.stack([z["S"].reshape(-1, order="F")[ix[i] - 1] for i, (_, z) in enumerate(rows)])
            for i, (_, z) in enumerate(rows):         # all of S is there
                assert np.count_nonzero(z["S"]) == np.count_nonzero(Sv[i])
            out[g + "indx_S_head"], out[g + "S_head"] = ix, Sv
        else:
            idx = np.full((len(rows), KEEP), -1, dtype=np.int32)
            val = np.zeros((len(rows), KEEP), dtype=np.complex128)
            nnz = np.zeros(len(rows), dtype=np.int64)
            amax = np.zeros(len(rows))
            for i, (_, z) in enumerate(rows):
                s = z["S"].reshape(-1, order="F")
                nz = np.flatnonzero(s)
                nnz[i], amax[i] = len(nz), np.max(np.abs(s))
                if len(nz) > KEEP:
                    nz = np.sort(nz[np.argsort(-np.abs(s[nz]), kind="stable")[:KEEP]])
                idx[i, :len(nz)], val[i, :len(nz)] = nz, s[nz]
            k = max(1, int((idx >= 0).sum(1).max()))
            out[g + "S_idx"], out[g + "S_val"] = idx[:, :k], val[:, :k]
            out[g + "S_nnz"], out[g + "S_absmax"] = nnz, amax
        print(solver, "trials", out[g + "trial"].tolist(), "seconds", [round(float(z["seconds"]), 1) for _, z in rows])
    path = os.path.join(HERE, "cfg5_fullframe_port.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_cfg5_fullframe_fixture.py DIR   (the --out directory of tools/cfg5_imax100_fixture.py)")
    main(sys.argv[1])
