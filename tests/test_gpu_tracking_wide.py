"""montecarlo.run_tracking with the widened "Proposed - PAI" modes (pai_wide_prev, warm_pai_wide_prev): radius (0, 0) is pai_prev /
warm_pai_prev number for number, a radius changes the numbers and repeats them, the result names the radii only when a wide mode
ran, and the old modes return what they returned."""
import numpy as np
import pytest

from test_gpu_tracking import RESULT_KEYS, SMALL, TOOL_KEYS, _sp

pytestmark = pytest.mark.gpu

SEQS, FRAMES, CORR, DRIFT = 4, 4, 0.9, 0.1
KW = dict(imax=(3,), cold_imax=6, batch=4, seed=11, sweep_idx=2, drift=DRIFT)
PAIRS = (("pai_prev", "pai_wide_prev"), ("warm_pai_prev", "warm_pai_wide_prev"))
# SMALL has Gt = 2 transmit cells: a ring that the smallest window (3 cells) already meets itself on, so a transmit radius needs
# Gt >= 4.  Gr*G2 = 64 here: at Imax 3 the mask holds 25 entries, so it binds.
WIDER = dict(Nt=4, Nr=8, L=2, T=4, Mr=2)


def _strip(d):
    return [{k: v for k, v in r.items() if k != "estimates_per_s"} for r in d["results"]]


def _by_frame(res):
    return {r["mode"]: r["mean_nmse_by_frame"] for r in res["results"] if r["Imax"] == 3}


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("primary", ["neighbourhood", "ties"])
def test_radius_0_is_the_plain_mode(precision, primary):
    from jstsp19_amd.montecarlo import run_tracking
    p = _sp(**SMALL)
    modes = tuple(m for pair in PAIRS for m in pair)
    res = run_tracking(p, SEQS, FRAMES, CORR, modes=modes, precision=precision, widen=(0, 0), widen_primary=primary, **KW)
    assert set(res) == TOOL_KEYS | {"drift", "widen", "widen_primary"}
    assert res["widen"] == [0, 0] and res["widen_primary"] == primary
    assert [(r["mode"], r["Imax"]) for r in res["results"]] == [(m, 3) for m in ("pai_prev", "warm_pai_prev") + tuple(w for _, w in PAIRS)]
    got = _by_frame(res)
    for plain, wide in PAIRS:
        assert len(got[wide]) == FRAMES - 1 and got[wide] == got[plain], wide      # equal: the same indx_S on the bits


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("shape,widen", [(SMALL, (1, 0)), (WIDER, (1, 1))], ids=["small_1_0", "wider_1_1"])
def test_a_radius_changes_the_numbers_and_repeats(precision, shape, widen):
    from jstsp19_amd.montecarlo import run_tracking
    p = _sp(**shape)
    modes = tuple(m for pair in PAIRS for m in pair)
    res = run_tracking(p, SEQS, FRAMES, CORR, modes=modes, precision=precision, widen=widen, **KW)
    assert res["widen"] == list(widen) and res["widen_primary"] == "neighbourhood"
    got = _by_frame(res)
    for plain, wide in PAIRS:
        assert all(np.isfinite(x) and 0.0 <= x <= 1.0 for x in got[wide]) and all(set(r) == RESULT_KEYS for r in res["results"])
        assert got[wide] != got[plain], wide                    # the widened order reaches the solver
    assert _strip(run_tracking(p, SEQS, FRAMES, CORR, modes=modes, precision=precision, widen=widen, **KW)) == _strip(res)
    ties = run_tracking(p, SEQS, FRAMES, CORR, modes=("pai_wide_prev",), precision=precision, widen=widen, widen_primary="ties", **KW)
    assert ties["widen_primary"] == "ties" and all(np.isfinite(x) for x in _by_frame(ties)["pai_wide_prev"])


def test_a_window_wider_than_the_grid_is_refused_before_anything_runs():
    from jstsp19_amd.montecarlo import run_tracking
    p = _sp(**SMALL)
    with pytest.raises(ValueError, match="meets itself"):
        run_tracking(p, SEQS, FRAMES, CORR, modes=("pai_wide_prev",), **KW)          # the default (1, 1) on Gt = 2
    assert "widen" not in run_tracking(p, SEQS, FRAMES, CORR, modes=("pai_prev",), **KW)   # not asked for: not looked at


def test_the_old_modes_return_what_they_returned():
    from jstsp19_amd.montecarlo import run_tracking
    p = _sp(**SMALL)
    modes = ("cold", "warm", "pai", "pai_prev", "warm_pai_prev")
    base = run_tracking(p, SEQS, FRAMES, CORR, modes=modes, **KW)
    assert set(base) == TOOL_KEYS | {"drift"}
    same = run_tracking(p, SEQS, FRAMES, CORR, modes=modes, widen=(1, 0), widen_primary="ties", **KW)
    assert set(same) == set(base) and _strip(same) == _strip(base)
    mixed = run_tracking(p, SEQS, FRAMES, CORR, modes=modes + ("pai_wide_prev",), widen=(1, 0), **KW)
    assert _strip(mixed)[:len(base["results"])] == _strip(base)             # a wide chain beside them changes none of them
