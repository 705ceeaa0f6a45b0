#!/usr/bin/env python3
"""Times of the float64 OMP and sparse_admm entries beside the fp32 entries of the same name and the numpy oracle on the host
(a record, no threshold): device memspace, after a warm-up call, median of 5.  Writes one JSON document (profiles/omp64_times.json).
  omp_kron_f64 / omp_kron at BASELINE configs[0] (N 16, M 64, Gr 16, G2 64, m 24), batch 1 and 256;
  OMP_f64 / OMP dense 1024 x 1024, m 24;  sparse_admm_f64 / sparse_admm 128 x 128, Imax 100, batch 64.
--only NAME runs one row (for a profiler)."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jstsp19_amd as J
from oracle import solvers as O

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--only", default=None)
ap.add_argument("--no-oracle", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
rng = np.random.default_rng(64)
c = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)
cm = lambda x, dt: J.colmajor(torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dt))


def med5(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def host(fn):
    if a.no_oracle:
        return None
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


rows = {}


def row(name, f64, f32, oracle_one, batch):
    if a.only and a.only != name:
        return
    rows[name] = dict(batch=batch, f64_s=med5(f64), f32_s=med5(f32), oracle_host_s_per_problem=host(oracle_one))
    print(name, rows[name], flush=True)


N, M, Gr, G2, m = 16, 64, 16, 64, 24
Af, Bf = c(N, Gr) / np.sqrt(N), c(G2, M) / np.sqrt(M)
Phi = np.kron(Bf.T.astype(complex), Af.astype(complex))
for batch in (1, 256):
    X = np.zeros((batch, Gr * G2), np.complex64)
    for t in range(batch):
        X[t, rng.choice(Gr * G2, 12, replace=False)] = c(12)
    Y = (X @ Phi.T + 0.05 * c(batch, N * M)).astype(np.complex64)
    tA, tB, tY = cm(Af, torch.complex64), cm(Bf, torch.complex64), torch.from_numpy(Y).to(dev)
    wA, wB, wY = tA.to(torch.complex128), tB.to(torch.complex128), tY.to(torch.complex128)
    row("omp_kron_cfg0_b%d" % batch, lambda: J.omp_kron_f64(wA, wB, wY, m), lambda: J.omp_kron(tA, tB, tY, m),
        lambda: O.omp_kron(Af, Bf, Y[0], m), batch)

meas = size_d = 1024
A = c(meas, size_d) / np.sqrt(meas)
x = np.zeros(size_d, np.complex64)
x[rng.choice(size_d, 12, replace=False)] = c(12)
v = (A.astype(complex) @ x + 0.05 * c(meas)).astype(np.complex64)
tA, tv = cm(A, torch.complex64), torch.from_numpy(v).to(dev)
wA, wv = tA.to(torch.complex128), tv.to(torch.complex128)
row("omp_dense_1024x1024_m24", lambda: J.OMP_f64(wA, wv, m, want_target=False), lambda: J.OMP(tA, tv, m, want_target=False),
    lambda: O.omp(A, v, m), 1)

n, batch, Imax = 128, 64, 100
k = np.arange(n)
F = (np.exp(-2j * np.pi * np.outer(k, k) / n) / np.sqrt(n))
H = np.stack([F @ (c(n, n) * (rng.random((n, n)) < 0.01)) @ F.conj().T for _ in range(batch)])
OH = H * (rng.random(H.shape) < 0.7)
t32 = [cm(z, torch.complex64) for z in (H, OH, F, F)]
t64 = [z.to(torch.complex128) for z in t32]
row("sparse_admm_128x128_imax100_b64", lambda: J.sparse_admm_f64(*t64, Imax), lambda: J.sparse_admm(*t32, Imax),
    lambda: O.sparse_admm(H[0], OH[0], F, F, Imax), batch)

doc = dict(device=torch.cuda.get_device_name(0), method="device memspace, one warm-up call, median of 5 (seconds per call)", rows=rows)
print(json.dumps(doc))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
