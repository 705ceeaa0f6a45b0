"""montecarlo.run_tracking(precision="f32", refresh_f32=True): the refresh modes of DESIGN.md section 9r through the fp32 solver
(proposed_algorithm_refresh; section 9s) at the small shape of tests/test_gpu_tracking_drift.py - finite, repeatable, different
columns when the refresh binds, and restated frame by frame through the public entries the runner is documented to call (rtol
1e-5, the bound tests/test_gpu_tracking_drift.py holds the fp32 runner to).  With the one refresh past the last iteration the rows
are those of cold, warm and pai_prev."""
import numpy as np
import pytest
import torch

from test_gpu_tracking import RESULT_KEYS, TOOL_KEYS
from test_gpu_tracking_drift import CORR, DRIFT, FRAMES, KW, SEQS, _point, _strip

pytestmark = pytest.mark.gpu

NEW = ("refresh", "warm_refresh", "pai_prev_refresh")
MODES = ("cold",) + NEW
POLICY = (1, 1)


def _restated(p, start, period):
    """mean_nmse_by_frame of (mode, 3) for the three refresh modes, by the loop the runner is documented to run."""
    import jstsp19_amd as J
    from jstsp19_amd.system_model import build_trials
    err = {m: [] for m in NEW}
    prev_S, state = None, None
    for f in range(FRAMES):
        inp = build_trials(p, 0, SEQS, seed=11, sweep_idx=2, frame=f, corr=CORR, drift=DRIFT)
        args = (inp["subY"], inp["Omega"], inp["A"], inp["B"])
        prm = (inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())
        kw = dict(start=start, period=period, want_ce=False)
        est = {"refresh": J.proposed_algorithm_refresh(*args, 3, *prm, return_state=False, **kw)[0]}
        est["warm_refresh"], _, _, state, _ = J.proposed_algorithm_refresh(*args, 3, *prm, state=state, return_state=True, **kw)
        ix = J.support_order(prev_S) if f else None
        est["pai_prev_refresh"] = prev_S = J.proposed_algorithm_refresh(*args, 3, *prm, indx_S=ix, return_state=False, **kw)[0]
        if f:
            for m in err:
                err[m].append(torch.as_tensor(J.nmse_spectral(est[m], inp["Zbar"])).double().cpu().numpy())
    return {m: [float(x) for x in np.stack(e).mean(axis=1)] for m, e in err.items()}


def test_the_refresh_modes_on_the_fp32_solver():
    from jstsp19_amd.montecarlo import run_tracking
    p = _point()                                                # Gr*G2 = 32: at Imax 3 the mask holds 25 entries, so it binds
    res = run_tracking(p, SEQS, FRAMES, CORR, drift=DRIFT, modes=MODES, precision="f32", refresh_f32=True, refresh=POLICY, **KW)
    assert set(res) == TOOL_KEYS | {"drift", "refresh", "refresh_f32"} and res["refresh"] == list(POLICY) and res["refresh_f32"] is True
    assert res["precision"] == "f32"
    got = {(r["mode"], r["Imax"]): r for r in res["results"]}
    assert list(got) == [("cold", 3), ("cold", 6)] + [(m, 3) for m in NEW]
    for r in got.values():
        assert set(r) == RESULT_KEYS and len(r["mean_nmse_by_frame"]) == FRAMES - 1 and r["estimates_per_s"] > 0
        assert all(np.isfinite(x) and 0.0 <= x <= 1.0 for x in r["mean_nmse_by_frame"])
    by_frame = {m: got[(m, 3)]["mean_nmse_by_frame"] for m in MODES}
    assert len({tuple(v) for v in by_frame.values()}) == 4      # four different columns
    for m, ref in _restated(p, *POLICY).items():
        np.testing.assert_allclose(by_frame[m], ref, rtol=1e-5, err_msg=m)
    again = run_tracking(p, SEQS, FRAMES, CORR, drift=DRIFT, modes=MODES, precision="f32", refresh_f32=True, refresh=POLICY, **KW)
    assert _strip(again) == _strip(res)


def test_a_refresh_past_the_last_iteration_gives_the_rows_it_starts_from():
    from jstsp19_amd.montecarlo import run_tracking
    p = _point()
    old = ("cold", "warm", "pai_prev")
    res = run_tracking(p, SEQS, FRAMES, CORR, drift=DRIFT, modes=old + NEW, precision="f32", refresh_f32=True, refresh=(3, 0), **KW)
    got = {(r["mode"], r["Imax"]): r for r in res["results"]}
    rows = lambda ms: [{k: v for k, v in got[(m, 3)].items() if k not in ("mode", "estimates_per_s")} for m in ms]
    assert rows(NEW) == rows(old)                               # no refresh in any call: the bits of the resumed entry
