"""montecarlo.run_tracking with the support refreshed inside the solver (refresh, warm_refresh, pai_prev_refresh; DESIGN.md
section 9r) at the small shape of tests/test_gpu_tracking_drift.py: finite, repeatable on the bits, different from the columns
they start from when the refresh binds, and - with the one refresh scheduled past the last iteration - the rows of cold, warm and
pai_prev."""
import numpy as np
import pytest

from test_gpu_tracking import RESULT_KEYS, TOOL_KEYS
from test_gpu_tracking_drift import CORR, DRIFT, FRAMES, KW, SEQS, _point, _strip

pytestmark = pytest.mark.gpu

NEW = ("refresh", "warm_refresh", "pai_prev_refresh")
OLD = ("cold", "warm", "pai_prev")


def _rows(res, modes):
    got = {(r["mode"], r["Imax"]): r for r in res["results"]}
    return [{k: v for k, v in got[(m, 3)].items() if k not in ("mode", "estimates_per_s")} for m in modes]


def test_the_refresh_modes_are_finite_repeat_and_bind():
    from jstsp19_amd.montecarlo import run_tracking
    p = _point()                                                # Gr*G2 = 32: at Imax 3 the mask holds 25 entries, so it binds
    res = run_tracking(p, SEQS, FRAMES, CORR, drift=DRIFT, modes=OLD + NEW, refresh=(1, 1), **KW)
    assert set(res) == TOOL_KEYS | {"drift", "refresh"} and res["refresh"] == [1, 1]
    assert [(r["mode"], r["Imax"]) for r in res["results"]] == [("cold", 3), ("cold", 6)] + [(m, 3) for m in ("warm", "pai_prev") + NEW]
    for r in res["results"]:
        assert set(r) == RESULT_KEYS and len(r["mean_nmse_by_frame"]) == FRAMES - 1 and r["estimates_per_s"] > 0
        assert all(np.isfinite(x) and 0.0 <= x <= 1.0 for x in r["mean_nmse_by_frame"])
    by_frame = [tuple(r["mean_nmse_by_frame"]) for r in _rows(res, OLD + NEW)]
    assert len(set(by_frame)) == 6                              # six different columns
    assert _strip(run_tracking(p, SEQS, FRAMES, CORR, drift=DRIFT, modes=OLD + NEW, refresh=(1, 1), **KW)) == _strip(res)
    every = run_tracking(p, SEQS, FRAMES, CORR, drift=DRIFT, modes=NEW, **KW)      # the default: a refresh in every iteration
    assert every["refresh"] == [0, 1] and _rows(every, NEW) != _rows(res, NEW)
    assert _rows(every, NEW)[0] == _rows(every, NEW)[2]         # ... so the order of the previous estimate is never in force


def test_a_refresh_past_the_last_iteration_gives_the_rows_it_starts_from():
    from jstsp19_amd.montecarlo import run_tracking
    p = _point()
    res = run_tracking(p, SEQS, FRAMES, CORR, drift=DRIFT, modes=OLD + NEW, refresh=(3, 0), **KW)
    assert _rows(res, NEW) == _rows(res, OLD)                   # float64: the same floats
    assert "refresh" not in run_tracking(p, SEQS, FRAMES, CORR, drift=DRIFT, modes=("cold",), refresh=(3, 0), **KW)
