#!/usr/bin/env python3
"""Rates of svd_f64 (jstsp_svd_f64, csrc/svd64.hip) on one GPU, U, s and V all asked for, device-resident operands, after one
warm-up call per shape, a host clock around a quarter second of calls that ends in a device synchronise (best of --reps windows):

  - 1024 matrices of 32 x 140 (the reference-native receive signal) and of 64 x 64: the single-launch LDS route;
  - 64 matrices of 64 x 160 and of 96 x 300: the global-memory route (one launch per round, one stream wait per sweep);
  - numpy.linalg.svd (float64, vectors) on the same shapes beside them, the matrices spread over the granted CPUs
    (OMP_NUM_THREADS of the caller, 16 at most), one LAPACK thread each.

--tall: svd_tall_f64 (jstsp_svd_tall_f64, the QR route with the reflectors kept) instead, on 8 matrices of 64 x 65536 and 64 of
32 x 16384, written to profiles/svd64_tall_rate.json.

Every measurement runs in a child process of its own under `timeout -k 10`; the first one that fails ends the run.  Prints one
JSON line and writes it to --out.  A record: there is no threshold and no earlier number for a new entry."""
import argparse, json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(32, 140, 1024, "lds"), (64, 64, 1024, "lds"), (64, 160, 64, "global"), (96, 300, 64, "global")]
CASES_TALL = [(64, 65536, 8, "qr"), (32, 16384, 64, "qr")]

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--numpy-sample", type=int, default=64)
ap.add_argument("--limit", type=int, default=120, help="seconds each child may take")
ap.add_argument("--tall", action="store_true", help="svd_tall_f64 on 8 x (64 x 65536) and 64 x (32 x 16384)")
ap.add_argument("--out", default=None, help="default: profiles/svd64_rate.json, with --tall profiles/svd64_tall_rate.json")
ap.add_argument("--device-case", default=None, help=argparse.SUPPRESS)
ap.add_argument("--numpy-case", default=None, help=argparse.SUPPRESS)
a = ap.parse_args()
if a.out is None:
    a.out = os.path.join(ROOT, "profiles", "svd64_tall_rate.json" if a.tall else "svd64_rate.json")


def operand(rows, cols, batch):
    import numpy as np
    rng = np.random.default_rng(rows * 7 + cols)
    return (rng.standard_normal((batch, rows, cols)) + 1j * rng.standard_normal((batch, rows, cols))) * 0.3


if a.device_case:
    import torch
    sys.path.insert(0, ROOT)
    import jstsp19_amd as J
    rows, cols, batch = (int(x) for x in a.device_case.split(","))
    svd = J.svd_tall_f64 if a.tall else J.svd_f64
    A = J.colmajor(torch.from_numpy(operand(rows, cols, batch)).to("cuda:0"))
    U, s, V, rank, conv = svd(A, info=True)                          # warm-up of this shape
    torch.cuda.synchronize()
    assert bool((conv == 1).all()) and bool((rank == min(rows, cols)).all())
    t0 = time.perf_counter()
    svd(A)
    torch.cuda.synchronize()
    calls = max(1, min(200, int(0.25 / max(time.perf_counter() - t0, 1e-4)) + 1))      # a timed window of about a quarter second
    best = float("inf")
    for _ in range(a.reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            svd(A)
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / calls)
    print(json.dumps(dict(seconds=round(best, 6), calls_per_window=calls, matrices_per_s=round(batch / best, 1),
                          device=torch.cuda.get_device_name(0))))
    sys.exit(0)

if a.numpy_case:
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    rows, cols, count, threads = (int(x) for x in a.numpy_case.split(","))
    A = operand(rows, cols, count)
    np.linalg.svd(A[:2], full_matrices=False)
    parts = [A[i::threads] for i in range(threads) if A[i::threads].size]
    done, t0 = 0, time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as ex:
        while done == 0 or time.perf_counter() - t0 < 0.25:            # about a quarter second of whole passes over the sample
            list(ex.map(lambda p: np.linalg.svd(p, full_matrices=False), parts))
            done += count
    t = time.perf_counter() - t0
    print(json.dumps(dict(seconds=round(t, 6), matrices=done, matrices_per_s=round(done / t, 1))))
    sys.exit(0)


def child(args, env=None):
    r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit("bench_svd64: %s ended with status %d; nothing more is started" % (" ".join(args), r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


threads = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "16") or 16)))
one = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
res = dict(entry="svd_tall_f64" if a.tall else "svd_f64", reps=a.reps, host_threads=threads, shapes=[])
for rows, cols, batch, route in CASES_TALL if a.tall else CASES:
    d = child(["--device-case", "%d,%d,%d" % (rows, cols, batch), "--reps", str(a.reps)] + (["--tall"] if a.tall else []))
    res["device"] = d.pop("device")
    count = min(batch, max(a.numpy_sample, threads))
    h = child(["--numpy-case", "%d,%d,%d,%d" % (rows, cols, count, threads)], env=one)
    res["shapes"].append(dict(rows=rows, cols=cols, batch=batch, route=route, seconds=d["seconds"], calls_per_window=d["calls_per_window"],
                              matrices_per_s=d["matrices_per_s"],
                              numpy_matrices=h["matrices"], numpy_matrices_per_s=h["matrices_per_s"],
                              ratio=round(d["matrices_per_s"] / h["matrices_per_s"], 1)))
line = json.dumps(res)
print(line)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
