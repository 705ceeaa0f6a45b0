"""montecarlo.run_tracking(precision="f32", until_f32=True, stop=...): the *_until modes of DESIGN.md section 9t through the fp32
solver (proposed_algorithm_until; section 9u) on the small shape (Nt = 4, Nr = 32, L = 4, T = 35, Mr = 4), 2 sequences of 3 frames:
the cold_until row is restated frame by frame through the public entry the runner is documented to call - the same calls on the
same frames, so the numbers are equal - and the iterations it reports lie in [min_iters, Imax]."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEQS, FRAMES, CORR, IMAX, STOP = 2, 3, 0.9, 30, (1e-3, 2)
KW = dict(imax=(5,), cold_imax=IMAX, batch=SEQS, seed=11, sweep_idx=2)


def _point():
    from jstsp19_amd.system_model import SweepParams
    return SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4, snr_db=5.0)


def _restated(p):
    """(NMSE, iterations), each (scored frames, sequences), of cold_until by direct calls"""
    import jstsp19_amd as J
    from jstsp19_amd.system_model import build_trials
    err, its = [], []
    for f in range(FRAMES):
        inp = build_trials(p, 0, SEQS, seed=11, sweep_idx=2, device=torch.device("cuda:0"), frame=f, corr=CORR)
        prm = (inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())
        S, _, _, _, _, n, _ = J.proposed_algorithm_until(inp["subY"], inp["Omega"], inp["A"], inp["B"], IMAX, *prm, tol=STOP[0], min_iters=STOP[1],
                                                         return_state=False)
        if f:
            err.append(torch.as_tensor(J.nmse_spectral(S, inp["Zbar"])).double().cpu().numpy())
            its.append(n.cpu().numpy())
    return np.stack(err), np.stack(its)


def test_the_until_modes_on_the_fp32_solver():
    from jstsp19_amd.montecarlo import TRACKING_UNTIL_MODES, run_tracking
    p = _point()
    res = run_tracking(p, SEQS, FRAMES, CORR, modes=TRACKING_UNTIL_MODES, precision="f32", until_f32=True, stop=STOP, **KW)
    assert res["precision"] == "f32" and res["until_f32"] is True and res["stop"] == list(STOP)
    got = {(r["mode"], r["Imax"]): r for r in res["results"]}
    assert list(got) == [(m, IMAX) for m in TRACKING_UNTIL_MODES]
    for r in got.values():
        assert len(r["mean_nmse_by_frame"]) == FRAMES - 1 and all(np.isfinite(x) and 0.0 <= x <= 1.0 for x in r["mean_nmse_by_frame"])
        assert STOP[1] <= r["mean_iters"] <= r["max_iters"] <= IMAX and STOP[1] <= r["median_iters"] <= IMAX
        assert all(STOP[1] <= x <= IMAX for x in r["mean_iters_by_frame"])
    err, its = _restated(p)
    cold = got[("cold_until", IMAX)]
    assert cold["mean_nmse_by_frame"] == [float(x) for x in err.mean(axis=1)] and cold["mean_nmse"] == float(err.mean())
    assert cold["mean_iters_by_frame"] == [float(x) for x in its.mean(axis=1)] and cold["max_iters"] == int(its.max())
    assert its.min() >= STOP[1] and its.max() <= IMAX
