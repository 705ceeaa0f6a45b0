"""The numpy reference of the widened support order (tests/wide_ref.py) against the plain order and on windows worked out by hand,
and the public surface of jstsp_support_order_wide_* without a GPU: the header, the ctypes table, the built library, the Python
names, and run_tracking's two wide modes and their keywords."""
import inspect
import os
import re

import numpy as np
import pytest

import drift_ref as D
import wide_ref as W
import jstsp19_amd as J
from jstsp19_amd import _lib
from test_drift_ref import continuous_trial, tie_trials

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE32, WIDE64 = "jstsp_support_order_wide_c32", "jstsp_support_order_wide_f64"
DTYPES = [pytest.param(np.complex64, np.float32, id="c32"), pytest.param(np.complex128, np.float64, id="f64")]


# ---- the reference --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("primary", W.PRIMARIES)
@pytest.mark.parametrize("cdtype,real", DTYPES)
def test_radius_zero_is_the_plain_order(cdtype, real, primary):
    for S in tie_trials().astype(cdtype):                       # 5 x 7: Gt = 7, L = 1
        np.testing.assert_array_equal(W.support_order_wide_ref(S, 7, 0, 0, primary, real), D.support_order_ref(S, real))
    S = continuous_trial().astype(cdtype)
    np.testing.assert_array_equal(W.support_order_wide_ref(S, 64, 0, 0, primary, real), D.support_order_ref(S, real))


def test_a_corner_spike_wraps_inside_its_own_delay_block():
    Gr, Gt, L = 6, 4, 3
    S = np.zeros((Gr, Gt * L), complex)
    S[0, Gt - 1] = 2.0                                          # row 0, the last transmit cell of delay block 0
    got = W.support_order_wide_ref(S, Gt, 1, 1, "neighbourhood", np.float64) - 1
    rows, cols = got % Gr, got // Gr
    assert (rows[0], cols[0]) == (0, 3)                         # the spike, then the rest of its window in index order
    assert sorted(zip(rows[:9].tolist(), cols[:9].tolist())) == sorted((r, c) for r in (5, 0, 1) for c in (2, 3, 0))
    np.testing.assert_array_equal(got[1:9], np.sort(got[1:9]))
    assert 4 not in cols[:9].tolist()                           # column 4 is block 1's first cell: no neighbour of column 3
    np.testing.assert_array_equal(got[9:], np.setdiff1d(np.arange(Gr * Gt * L), got[:9]))
    # "ties" keeps the spike first and orders the zeros the same way here: every zero's own key is equal
    np.testing.assert_array_equal(W.support_order_wide_ref(S, Gt, 1, 1, "ties", np.float64) - 1, got)


@pytest.mark.parametrize("cdtype,real", DTYPES)
def test_the_strongest_entry_is_followed_by_its_ring_window(cdtype, real):
    S = continuous_trial().astype(cdtype)
    got = W.support_order_wide_ref(S, 64, 1, 1, "neighbourhood", real) - 1
    top = int(D.support_order_ref(S, real)[0]) - 1
    r, c = top % 64, top // 64
    l, g = c // 64, c % 64
    window = {((r + dr) % 64) + 64 * (l * 64 + (g + dg) % 64) for dr in (-1, 0, 1) for dg in (-1, 0, 1)}
    assert got[0] == top and set(got[:9].tolist()) == window
    mag = np.abs(S.reshape(-1, order="F")[got[:9]])
    assert np.all(np.diff(mag) < 0)                             # the window in order of its entries' own magnitude
    plain = W.support_order_wide_ref(S, 64, 1, 1, "ties", real)
    np.testing.assert_array_equal(plain, D.support_order_ref(S, real))      # no equal own keys: "ties" is the plain order


def test_a_nan_propagates_to_its_window_and_key_order_is_magnitude_order():
    S = np.zeros((5, 7), complex)
    S[2, 3] = complex(np.nan, 0.0)
    S[0, 0] = complex(np.inf, 0.0)
    S[4, 6] = 3.0
    own, nbr = W.wide_keys(S, 7, 1, 1, np.float32)
    own2 = own.reshape(7, 5).T
    assert own2[2, 3] == 0 and 0 < own2[0, 0] < own2[4, 6] < own2[1, 1] == 0xFFFFFFFF
    nbr2 = nbr.reshape(7, 5).T
    assert np.all(nbr2[1:4, 2:5] == 0) and np.count_nonzero(nbr2 == 0) == 9
    assert nbr2[4, 0] == own2[0, 0] and nbr2[0, 6] == own2[0, 0]           # the Inf at (0, 0) reaches round both rings
    assert nbr2[3, 5] == own2[4, 6] and nbr2[3, 0] == own2[4, 6]


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def _prototype(name):
    h = open(os.path.join(ROOT, "include", "jstsp.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, h)
    assert m, "no prototype of %s" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")], h[:m.start()].rsplit("/*", 1)[1]


def test_header_declares_the_wide_entries_with_their_11_arguments():
    a32, _ = _prototype(WIDE32)
    a64, doc = _prototype(WIDE64)
    tail = ["int wr", "int wt", "int primary", "int32_t *indx_S", "int memspace"]
    assert a32 == ["jstsp_ctx *ctx", "int Gr", "int Gt", "int L", "int batch", "const jstsp_c32 *S"] + tail
    assert a64 == ["jstsp_ctx *ctx", "int Gr", "int Gt", "int L", "int batch", "const double *S"] + tail
    for word in ("JSTSP_E_SHAPE", "2^21", "JSTSP_E_ARG", "negative radius", "2*wr+1 > Gr", "primary not 0 or 1", "JSTSP_E_NULL",
                 "never crosses", "wideband_mmwave_channel.m:9-10"):
        assert word in doc, word


def test_signature_table_and_library_have_them():
    lib = J.load()
    for n in (WIDE32, WIDE64):
        res, args = _lib.SIGNATURES[n]
        assert res is _lib.c_int and len(args) == 11
        assert [a is _lib.c_int for a in args] == [False, True, True, True, True, False, True, True, True, False, True]
        assert hasattr(lib, n), n
        assert getattr(lib, n).argtypes == args


def test_support_order_wide_is_public():
    from jstsp19_amd import solvers
    for n in ("support_order_wide", "support_order_wide_f64"):
        assert n in solvers.__all__ and getattr(J, n) is getattr(solvers, n)
        sig = inspect.signature(getattr(solvers, n)).parameters
        assert list(sig) == ["S", "Gt", "wr", "wt", "primary", "ctx"]
        assert sig["wr"].default == 1 and sig["wt"].default == 1 and sig["primary"].default == "neighbourhood"
        assert sig["primary"].kind is inspect.Parameter.KEYWORD_ONLY and sig["ctx"].kind is inspect.Parameter.KEYWORD_ONLY
        assert sig["Gt"].default is inspect.Parameter.empty
    S = np.zeros((6, 12), dtype=np.complex64)
    with pytest.raises(ValueError, match="Gt"):                  # refused on the Python side, before anything touches a device
        solvers.support_order_wide(S, 5)
    with pytest.raises(ValueError, match="primary"):
        solvers.support_order_wide(S, 4, primary="index")
    with pytest.raises(ValueError, match="primary"):
        solvers.support_order_wide_f64(S.astype(np.complex128), 4, 1, 1, primary=0)


def test_run_tracking_takes_the_wide_modes_and_their_keywords():
    from jstsp19_amd import montecarlo
    from jstsp19_amd.system_model import SweepParams
    sig = inspect.signature(montecarlo.run_tracking).parameters
    assert sig["widen"].kind is inspect.Parameter.KEYWORD_ONLY and tuple(sig["widen"].default) == (1, 1)
    assert sig["widen_primary"].kind is inspect.Parameter.KEYWORD_ONLY and sig["widen_primary"].default == "neighbourhood"
    assert montecarlo.TRACKING_PAI_MODES[:3] == ("pai", "pai_prev", "warm_pai_prev")
    p = SweepParams(Nt=2, Nr=8, L=2, T=4, Mr=2)
    # the argument check accepts the new modes: with one of them the call gets past it and fails on the check that follows
    for mode in ("pai_wide_prev", "warm_pai_wide_prev"):
        with pytest.raises(ValueError, match="drift must be"):
            montecarlo.run_tracking(p, 2, 3, 0.5, modes=(mode,), drift=-1.0)
    with pytest.raises(ValueError, match="pai_wide_prev"):
        montecarlo.run_tracking(p, 2, 3, 0.5, modes=("hot",))
    for kw in (dict(widen=(-1, 0)), dict(widen=(0, -2)), dict(widen=3), dict(widen=(1, 1, 1)), dict(widen_primary="x")):
        with pytest.raises(ValueError, match="widen"):
            montecarlo.run_tracking(p, 2, 3, 0.5, modes=("pai_wide_prev",), **kw)
