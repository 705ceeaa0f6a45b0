"""BASELINE configs[4] at the reference's Imax = 100 against float64: the inputs of bench.py's configs4 leg (N=64, M=65 536, Gr=64,
G2=4096, one pilot set for the batch, seed 20190913, sweep index 0, 5 dB, trials 0-31) rebuilt on the device and solved by the
library; tests/golden/cfg5_fullframe_port.npz holds what oracle.solvers.proposed_algorithm returns on the same inputs (made by
tools/cfg5_imax100_fixture.py + tests/golden/make_cfg5_fullframe_fixture.py; no float64 solve runs here).

The calls put fixture trials in both halves of a pair of hgemm_pair_kernel, under both tile counts (batch 32 and 16), in the lone
last pair of an odd batch (trials 3-19: trial 19), under both call forms (_angles and plain) and on the strict fp32-MFMA path."""
import os

import numpy as np
import pytest

from conftest import check_below, ce_rel, load_golden, rel_err, TOL_S, TOL_CE, TOL_NMSE

pytestmark = pytest.mark.gpu

FIXTURE = "cfg5_fullframe_port"


def _np(x, t, dt=np.complex128):
    return x[t].cpu().numpy().astype(dt)


@pytest.fixture(scope="module")
def cfg5():
    """the 32 trials of the configs4 workload on the device, each checked against the fixture's fingerprint."""
    import psutil
    import torch
    import jstsp19_amd as J
    from jstsp19_amd.system_model import SweepParams, build_trials
    if psutil.virtual_memory().available < (24 << 30):
        pytest.skip("needs 24 GiB of free host memory for the float64 references at this size")
    fx = load_golden(FIXTURE)
    p = SweepParams(Nt=256, Nr=64, L=16, T=256, Mr=8, snr_db=float(fx["snr_db"]))
    assert p.solver_shape == (64, 65536, 64, 4096)
    inp = build_trials(p, 0, 32, seed=int(fx["seed"]), sweep_idx=int(fx["sweep_idx"]), shared_pilots=True)
    B = J.colmajor(inp["B"][0].clone())
    del inp["B"]
    torch.cuda.empty_cache()
    fp = np.concatenate([torch.stack([inp["subY"].abs().double().sum((1, 2)), B.abs().double().sum().expand(32),
                                      inp["Omega"].double().sum((1, 2))], 1).cpu().numpy(),
                         np.stack([inp[k].numpy() for k in ("tau_Y", "tau_Z", "rho")], 1),
                         inp["Zbar"].abs().double().sum((1, 2)).cpu().numpy()[:, None]], 1)
    np.testing.assert_allclose(fp, fx["fingerprint"], rtol=1e-9, err_msg="the generator no longer reproduces the fixture's inputs")
    inp["B"] = B
    inp["hyp"] = [np.ascontiguousarray(fx["fingerprint"][:, 3 + k]) for k in range(3)]    # what the float64 side was given
    inp["Zbar_h"] = inp["Zbar"].cpu().numpy().astype(np.complex128)
    yield fx, inp
    del inp
    torch.cuda.empty_cache()


def _solve(inp, t0, t1, *, angles=True, want_ce=True):
    import torch
    import jstsp19_amd as J
    hyp = [h[t0:t1] for h in inp["hyp"]]
    S, _, ce = J.proposed_algorithm(inp["subY"][t0:t1], inp["Omega"][t0:t1], inp["A"], inp["B"], int(100), *hyp, "approximate",
                                    indx_S=inp["indx_S"][t0:t1] if angles else None, want_ce=want_ce)
    torch.cuda.synchronize()
    assert torch.isfinite(torch.view_as_real(S)).all()
    return S.cpu().numpy().astype(np.complex128), (ce.cpu().numpy() if want_ce else None)


def _check_angles(tag, fx, inp, S, ce, t0):
    """every fixture trial in [t0, t0 + len(S)): |dNMSE|, S over the 510 positions of indx_S(1 : 10 + 5 Imax) and nothing outside
    them, convergence_error (when returned); rms and mean of dNMSE over those trials."""
    from oracle import solvers as O
    d = []
    for i, t in enumerate(fx["angles/trial"]):
        if not t0 <= t < t0 + len(S):
            continue
        s = S[t - t0].reshape(-1, order="F")
        pos = fx["angles/indx_S_head"][i].astype(np.int64) - 1
        assert np.array_equal(pos + 1, inp["indx_S"][t, :len(pos)].cpu().numpy())
        ref = fx["angles/S_head"][i]
        check_below("cfg5i100.%s.S" % tag, np.max(np.abs(s[pos] - ref)) / np.max(np.abs(ref)), TOL_S)
        out = np.ones(s.size, bool)
        out[pos] = False
        assert not np.any(s[out]), (tag, int(t), "nonzero outside indx_S(1:510)")
        dn = O.nmse_capped(S[t - t0], inp["Zbar_h"][t]) - fx["angles/nmse_port"][i]
        check_below("cfg5i100.%s.nmse" % tag, abs(dn), TOL_NMSE)
        d.append(dn)
        if ce is not None:
            check_below("cfg5i100.%s.ce" % tag, ce_rel(ce[t - t0], fx["angles/ce_port"][i]), TOL_CE)
    assert d, tag
    check_below("cfg5i100.%s.nmse.rms" % tag, np.sqrt(np.mean(np.square(d))), TOL_NMSE)
    check_below("cfg5i100.%s.nmse.mean" % tag, abs(np.mean(d)), TOL_NMSE)


def test_cfg5_imax100_angles_batch32_three_outputs_is_the_bench_call(cfg5):
    """bench.py's configs4 call (batch 32, three outputs, 8 ... 16 pairs per tile of hgemm_pair_kernel) against float64 at Imax 100."""
    fx, inp = cfg5
    assert int(fx["imax"]) == 100
    S, ce = _solve(inp, 0, 32)
    assert np.all(np.isinf(ce[:, 0, 2]))
    _check_angles("angles.b32", fx, inp, S, ce, 0)


def test_cfg5_imax100_angles_batch16_two_outputs(cfg5):
    """the same trials as two calls of 16 (the other tile count of the pair kernel), without convergence_error."""
    fx, inp = cfg5
    for t0 in (0, 16):
        S, _ = _solve(inp, t0, t0 + 16, want_ce=False)
        _check_angles("angles.b16", fx, inp, S, None, t0)


def test_cfg5_imax100_angles_batch17_odd_last_pair(cfg5):
    """trials 3-19 (batch 17): trial 19 is alone in the last pair, and every trial has another partner and half than at batch 32."""
    fx, inp = cfg5
    S, ce = _solve(inp, 3, 20)
    _check_angles("angles.b17", fx, inp, S, ce, 3)


def test_cfg5_imax100_proposed_batch16(cfg5):
    """proposed_algorithm (no indx_S) on trials 0-15 - batch 16, so that K B^H still takes the pair kernel - against the fixture's
    plain float64 solves: |dNMSE|, S at the stored nonzeros of the float64 S and (where the fixture holds all of them) nowhere
    else above TOL_S of max|S|, convergence_error."""
    from oracle import solvers as O
    fx, inp = cfg5
    S, ce = _solve(inp, 0, 16, angles=False)
    for i, t in enumerate(fx["proposed/trial"]):
        s = S[t].reshape(-1, order="F")
        idx = fx["proposed/S_idx"][i]
        val = fx["proposed/S_val"][i][idx >= 0]
        idx = idx[idx >= 0].astype(np.int64)
        amax = fx["proposed/S_absmax"][i]
        check_below("cfg5i100.proposed.b16.S", np.max(np.abs(s[idx] - val)) / amax, TOL_S)
        if fx["proposed/S_nnz"][i] == len(idx):
            out = np.ones(s.size, bool)
            out[idx] = False
            check_below("cfg5i100.proposed.b16.S", np.max(np.abs(s[out])) / amax, TOL_S)
        check_below("cfg5i100.proposed.b16.nmse", abs(O.nmse_capped(S[t], inp["Zbar_h"][t]) - fx["proposed/nmse_port"][i]), TOL_NMSE)
        check_below("cfg5i100.proposed.b16.ce", ce_rel(ce[t], fx["proposed/ce_port"][i]), TOL_CE)


def test_cfg5_imax100_angles_batch32_strict_fp32_mfma(cfg5):
    """JSTSP_H2=0 (the strict complex-fp32 MFMA path) on the bench call: inside the same contract."""
    fx, inp = cfg5
    old = os.environ.get("JSTSP_H2")
    os.environ["JSTSP_H2"] = "0"
    try:
        S, _ = _solve(inp, 0, 32, want_ce=False)
    finally:
        if old is None:
            os.environ.pop("JSTSP_H2")
        else:
            os.environ["JSTSP_H2"] = old
    _check_angles("angles.b32.h2_0", fx, inp, S, None, 0)


def test_cfg5_full_frame_contractions_through_the_pair_kernel():
    """J.correlate (A' K B') and J.synthesize (A S B) at exactly this shape - N = Gr = 64, M = 65 536 terms in K B', G2 = 4096 in
    (A S) B - on the library-built block-Toeplitz B shared by a batch of 17 with very different scales per trial; trials 0, 15 and
    16 (alone in the last pair) against float64: max|d| / max|ref| < 5e-6 as in tests/test_gpu_hgemm.py, and entry by entry against
    the magnitude of the chain, |d_ij| / (|A|^T |K| |B|^T)_ij (resp. (|A| |S| |B|)_ij), at about 4 x the measured maximum (4.9e-9
    for A' K B', 4.3e-8 for A S B on MI355X).
    Both calls take hgemm_pair_kernel at this batch (rocprofv3 --kernel-trace --stats of this test: hgemm_pair_kernel, two
    launches, and no per-trial contraction kernel)."""
    import psutil
    import torch
    import jstsp19_amd as J
    from jstsp19_amd.system_model import SweepParams, build_trials
    if psutil.virtual_memory().available < (24 << 30):
        pytest.skip("needs 24 GiB of free host memory for the float64 references at this size")
    inp = build_trials(SweepParams(Nt=256, Nr=64, L=16, T=256, Mr=8, snr_db=5.0), 0, 1, shared_pilots=True)
    inp["B"] = J.colmajor(inp["B"][0].clone())
    dev = inp["B"].device
    rng = np.random.default_rng(4096)
    nb, N, M, Gr, G2 = 17, 64, 65536, 64, 4096
    scale = np.ones(nb)
    scale[15], scale[16], scale[1] = 1e-6, 3e4, 1e5
    c = lambda *s: (rng.standard_normal(s, dtype=np.float32) + 1j * rng.standard_normal(s, dtype=np.float32)).astype(np.complex64)
    K = c(nb, N, M) * scale[:, None, None].astype(np.float32)
    S = c(nb, Gr, G2) / scale[::-1, None, None].astype(np.float32)
    cm = lambda a: J.colmajor(torch.from_numpy(a).to(dev))
    Cg = J.correlate(cm(K), inp["A"], inp["B"])
    Xg = J.synthesize(cm(S), inp["A"], inp["B"])
    torch.cuda.synchronize()
    A = inp["A"].cpu().numpy().astype(np.complex128)
    B = inp["B"].cpu().numpy().astype(np.complex128)
    aA, aB = np.abs(A), np.abs(B)
    for t in (0, 15, 16):
        Kt, St = K[t].astype(np.complex128), S[t].astype(np.complex128)
        ref_c = (A.conj().T @ Kt) @ B.conj().T
        ref_s = (A @ St) @ B
        cg, xg = _np(Cg, t), _np(Xg, t)
        check_below("cfg5.pair.correlate", rel_err(cg, ref_c), 5e-6)
        check_below("cfg5.pair.synthesize", rel_err(xg, ref_s), 5e-6)
        check_below("cfg5.pair.correlate.entrywise", np.max(np.abs(cg - ref_c) / ((aA.T @ np.abs(Kt)) @ aB.T)), 2e-8)
        check_below("cfg5.pair.synthesize.entrywise", np.max(np.abs(xg - ref_s) / ((aA @ np.abs(St)) @ aB)), 1.7e-7)
