"""montecarlo.run_tracking on a channel whose angles walk, with the "Proposed - PAI" modes (pai, pai_prev, warm_pai_prev): every
new mode against its own loop restated here from build_trials(frame=, corr=, drift=), the resume solvers with indx_S= and
support_order*, repeatability, and what must not change - the default call's keys, and drift = 0 against drift = None."""
import numpy as np
import pytest
import torch

from test_gpu_tracking import RESULT_KEYS, TOOL_KEYS, _sp

pytestmark = pytest.mark.gpu

MODES = ("cold", "pai", "pai_prev", "warm_pai_prev")
SEQS, FRAMES, CORR, DRIFT = 4, 3, 0.9, 0.1
KW = dict(imax=(3,), cold_imax=6, batch=4, seed=11, sweep_idx=2)


def _point():
    return _sp(Nt=2, Nr=8, L=2, T=6, Mr=2)                      # Gr*G2 = 32: at Imax 3 the mask holds 25 entries, so it binds


def _strip(d):
    return [{k: v for k, v in r.items() if k != "estimates_per_s"} for r in d["results"]]


def _restated(p, precision):
    """mean_nmse_by_frame of (mode, 3) for the three PAI modes, by the loop the runner is documented to run."""
    import jstsp19_amd as J
    from jstsp19_amd.system_model import build_trials
    f64 = precision == "f64"
    wide = (lambda x: J.colmajor(x.to(torch.complex128))) if f64 else (lambda x: x)
    solve = J.proposed_algorithm_resume_f64 if f64 else J.proposed_algorithm_resume
    score = J.nmse_spectral_f64 if f64 else J.nmse_spectral
    order = J.support_order_f64 if f64 else J.support_order
    err = {m: [] for m in MODES[1:]}
    prev, state = {}, None
    for f in range(FRAMES):
        inp = build_trials(p, 0, SEQS, seed=11, sweep_idx=2, frame=f, corr=CORR, drift=DRIFT)
        args = (wide(inp["subY"]), J.colmajor(inp["Omega"].to(torch.float64)) if f64 else inp["Omega"], wide(inp["A"]), wide(inp["B"]))
        prm = (inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())
        est = {}
        est["pai"] = solve(*args, 3, *prm, indx_S=inp["indx_S"], want_ce=False, return_state=False)[0]
        ix = order(prev["pai_prev"]) if f else None
        est["pai_prev"] = solve(*args, 3, *prm, indx_S=ix, want_ce=False, return_state=False)[0]
        ix = order(prev["warm_pai_prev"]) if f else None
        est["warm_pai_prev"], _, _, state = solve(*args, 3, *prm, indx_S=ix, want_ce=False, state=state, return_state=True)
        prev = est
        if f:
            for m in err:
                err[m].append(torch.as_tensor(score(est[m], wide(inp["Zbar"]))).double().cpu().numpy())
    return {m: [float(x) for x in np.stack(e).mean(axis=1)] for m, e in err.items()}


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_run_tracking_with_drift_and_the_pai_modes(precision):
    from jstsp19_amd.montecarlo import run_tracking
    p = _point()
    res = run_tracking(p, SEQS, FRAMES, CORR, drift=DRIFT, modes=MODES, precision=precision, **KW)
    assert set(res) == TOOL_KEYS | {"drift"} and res["drift"] == DRIFT and res["channel"] == "device"
    got = {(r["mode"], r["Imax"]): r for r in res["results"]}
    assert list(got) == [("cold", 3), ("cold", 6), ("pai", 3), ("pai_prev", 3), ("warm_pai_prev", 3)]
    for r in got.values():
        assert set(r) == RESULT_KEYS and len(r["mean_nmse_by_frame"]) == FRAMES - 1 and r["estimates_per_s"] > 0
        assert all(np.isfinite(x) and 0.0 <= x <= 1.0 for x in r["mean_nmse_by_frame"])
    by_frame = {m: got[(m, 3)]["mean_nmse_by_frame"] for m in MODES}
    assert len({tuple(v) for v in by_frame.values()}) == 4      # the mask binds and the three orders differ: four different columns
    want = _restated(p, precision)
    for m, ref in want.items():
        if precision == "f64":
            assert by_frame[m] == ref, m
        else:
            np.testing.assert_allclose(by_frame[m], ref, rtol=1e-5, err_msg=m)
    assert _strip(run_tracking(p, SEQS, FRAMES, CORR, drift=DRIFT, modes=MODES, precision=precision, **KW)) == _strip(res)


def test_the_default_call_is_unchanged_and_drift_0_is_drift_none():
    from jstsp19_amd.montecarlo import run_tracking
    p = _point()
    base = run_tracking(p, SEQS, FRAMES, CORR, **KW)
    assert set(base) == TOOL_KEYS
    assert [(r["mode"], r["Imax"]) for r in base["results"]] == [("cold", 3), ("cold", 6), ("warm", 3), ("warm_vs", 3)]
    assert all(set(r) == RESULT_KEYS for r in base["results"])
    zero = run_tracking(p, SEQS, FRAMES, CORR, drift=0.0, **KW)
    assert set(zero) == TOOL_KEYS | {"drift"} and zero["drift"] == 0.0
    assert _strip(zero) == _strip(base)                         # float64: the same floats
    moved = run_tracking(p, SEQS, FRAMES, CORR, drift=DRIFT, modes=("cold",), **KW)
    assert _strip(moved)[0]["mean_nmse_by_frame"] != _strip(base)[0]["mean_nmse_by_frame"]
