"""montecarlo.run_tracking(refit=(K, iters)) at the small shape of tools/run_tracking.py --small, 2 sequences,
3 frames, one Imax: without the option the dictionary is the one the call has always returned; with it every row carries three
more keys, every other number keeps its bits, and mean_nmse_refit is the mean of refit_f64 applied by hand to the same solves.
No threshold is placed on any NMSE."""
import numpy as np
import pytest

from test_gpu_tracking import RESULT_KEYS, TOOL_KEYS

pytestmark = pytest.mark.gpu

SEQS, FRAMES, CORR, IMAX, REFIT = 2, 3, 0.9, 4, (64, 5)
KW = dict(imax=(IMAX,), cold_imax=IMAX, batch=2, seed=7, sweep_idx=1, modes=("cold", "warm"))
NEW_KEYS = {"mean_nmse_refit", "mean_nmse_refit_by_frame", "refit_estimates_per_s"}
TIMES = ("estimates_per_s", "refit_estimates_per_s")


def _point():
    from jstsp19_amd.system_model import SweepParams
    return SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4, snr_db=5.0)


def _strip(res, drop=TIMES):
    return [{k: v for k, v in r.items() if k not in drop} for r in res["results"]]


def test_refit_none_is_the_dictionary_of_before_and_refit_adds_three_keys():
    from jstsp19_amd.montecarlo import run_tracking
    p = _point()
    base = run_tracking(p, SEQS, FRAMES, CORR, **KW)
    none = run_tracking(p, SEQS, FRAMES, CORR, refit=None, **KW)
    assert set(base) == set(none) == TOOL_KEYS and all(set(r) == RESULT_KEYS for r in none["results"])
    assert [(r["mode"], r["Imax"]) for r in none["results"]] == [("cold", IMAX), ("warm", IMAX)]
    assert _strip(none) == _strip(base)
    assert {k: v for k, v in none.items() if k != "results"} == {k: v for k, v in base.items() if k != "results"}
    res = run_tracking(p, SEQS, FRAMES, CORR, refit=REFIT, **KW)
    assert set(res) == TOOL_KEYS | {"refit"} and res["refit"] == list(REFIT)
    for r in res["results"]:
        assert set(r) == RESULT_KEYS | NEW_KEYS and len(r["mean_nmse_refit_by_frame"]) == FRAMES - 1 and r["refit_estimates_per_s"] > 0
        assert all(np.isfinite(x) and 0.0 <= x <= 1.0 for x in r["mean_nmse_refit_by_frame"])
    # the re-fitted estimate is only scored: the chains, warm ones included, keep their bits
    assert _strip(res, TIMES + tuple(NEW_KEYS)) == _strip(base)
    assert _strip(run_tracking(p, SEQS, FRAMES, CORR, refit=REFIT, **KW)) == _strip(res)


def test_mean_nmse_refit_is_refit_f64_by_hand_on_the_same_solves():
    import torch
    import jstsp19_amd as J
    from jstsp19_amd.montecarlo import run_tracking
    from jstsp19_amd.system_model import build_trials
    p = _point()
    res = run_tracking(p, SEQS, FRAMES, CORR, refit=REFIT, **KW)
    got = {r["mode"]: r for r in res["results"]}
    dev = torch.device("cuda:0")
    wide = lambda x: J.colmajor(x.to(torch.complex128))
    plain, fit, state = {"cold": [], "warm": []}, {"cold": [], "warm": []}, None
    for f in range(FRAMES):
        inp = build_trials(p, 0, SEQS, seed=KW["seed"], sweep_idx=KW["sweep_idx"], device=dev, frame=f, corr=CORR)
        args = (wide(inp["subY"]), J.colmajor(inp["Omega"].to(torch.float64)), wide(inp["A"]), wide(inp["B"]))
        prm = (inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())
        zb = wide(inp["Zbar"])
        S_cold = J.proposed_algorithm_resume_f64(*args, IMAX, *prm, want_ce=False, return_state=False)[0]
        S_warm, _, _, state = J.proposed_algorithm_resume_f64(*args, IMAX, *prm, want_ce=False, state=state)
        if not f:
            continue
        for mode, S in (("cold", S_cold), ("warm", S_warm)):
            S_fit, steps = J.refit_f64(*args, S, *REFIT)
            assert steps.dtype == torch.int32 and bool((steps == REFIT[1]).all())
            assert int((S_fit != 0).sum(dim=(1, 2)).max()) <= REFIT[0]
            plain[mode].append(J.nmse_spectral_f64(S, zb).double().cpu().numpy())
            fit[mode].append(J.nmse_spectral_f64(S_fit, zb).double().cpu().numpy())
    for mode in ("cold", "warm"):
        assert got[mode]["mean_nmse"] == float(np.stack(plain[mode]).mean())
        assert got[mode]["mean_nmse_refit"] == float(np.stack(fit[mode]).mean())
        assert got[mode]["mean_nmse_refit_by_frame"] == [float(x) for x in np.stack(fit[mode]).mean(axis=1)]
