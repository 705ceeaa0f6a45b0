"""tests/golden/cosamp.npz: the float64 CoSaMP reference (tests/cosamp_ref.py) on the seeded problems of
tests/cosamp_problems.py, with the decision record the GPU test leans on.  Run from the repository root:

    python tests/golden/make_cosamp_fixture.py

The inputs are rebuilt from their seeds by tests/cosamp_problems.py (64 dense 512 x 512 dictionaries do not belong in
git); `<group>.checksum` pins them.  Per group and problem: xs (the K kept coefficients, complex128), support (1-based),
iters, resid, status, decided, beta (the largest of the record), selb (the largest selection budget), rmin.
Class (e) also: nmse (capped spectral NMSE of the reference), p (the perturbation level: the largest selection budget of
the class) and dref (|dNMSE| between the reference on the inputs and on the inputs times (1 + p z), z standard complex
normal): what the algorithm itself makes of decisions flipped at the level where the rule says they may flip."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import cosamp_problems as P  # noqa: E402
import cosamp_ref as R  # noqa: E402

OUT = os.path.join(HERE, "cosamp.npz")


def _checksum(g):
    return float(sum(np.sum(np.abs(g[k].astype(np.complex128))) for k in ("Phi", "Af", "Bf", "y") if k in g))


def build():
    out = {}
    for g in P.groups():
        ref = P.reference(g)
        n, K, nm = len(ref), g["K"], g["name"]
        xs = np.zeros((n, K), np.complex128)
        for t, r in enumerate(ref):
            if r["support"].any():
                xs[t] = r["x"][r["support"] - 1]
        out[nm + ".xs"] = xs
        out[nm + ".support"] = np.stack([r["support"] for r in ref]).astype(np.int32)
        for key, dt in (("iters", np.int32), ("status", np.int32), ("resid", np.float64)):
            out[nm + "." + key] = np.array([r[key] for r in ref], dt)
        out[nm + ".decided"] = np.array([r["record"]["decided"] for r in ref])
        out[nm + ".beta"] = np.array([r["record"]["beta_max"] for r in ref])
        out[nm + ".selb"] = np.array([r["record"]["sel_budget_max"] for r in ref])
        out[nm + ".rmin"] = np.array([r["record"]["r_min"] for r in ref])
        out[nm + ".checksum"] = np.array(_checksum(g))
        if g["cls"] == "e":
            p = float(np.max(out[nm + ".selb"]))
            rng = np.random.default_rng(7999)
            pert = lambda a: a.astype(np.complex128) * (1 + p * (rng.standard_normal(a.shape) + 1j * rng.standard_normal(a.shape)) / np.sqrt(2))
            nmse, dref = np.zeros(n), np.zeros(n)
            for t in range(n):
                r2 = R.cosamp(R.Kron(pert(g["Af"][t]), pert(g["Bf"][t])), pert(g["y"][t]), K, g["iters"], g["tol"])
                nmse[t] = P.nmse_capped(ref[t]["x"], g["Zbar"][t])
                dref[t] = abs(P.nmse_capped(r2["x"], g["Zbar"][t]) - nmse[t])
            out[nm + ".nmse"], out[nm + ".dref"], out[nm + ".p"] = nmse, dref, np.array(p)
    return out


if __name__ == "__main__":
    np.savez(OUT, **build())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
