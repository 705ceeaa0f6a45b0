"""The order of a support on the device (jstsp_support_order_c32 / _f64, csrc/support.hip; support_order, support_order_f64):
the builder's indx_S on its own Zbar, exact against the stable host argsort of tests/drift_ref.py on engineered ties, zeros, a NaN
and an Inf, a trial without ties and a solver's own sparse S, independent of batch and memspace, usable as the indx_S of
proposed_algorithm_angles_f64, and the refusals."""
import numpy as np
import pytest
import torch

import drift_ref as D
import jstsp19_amd as J
from test_drift_ref import continuous_trial, keys_are_separated, tie_trials
from test_gpu_tracking import SMALL, _sp

pytestmark = pytest.mark.gpu

E_NULL, E_SHAPE = -1, -2
FORMS = [pytest.param(J.support_order, np.complex64, np.float32, id="c32"),
         pytest.param(J.support_order_f64, np.complex128, np.float64, id="f64")]


def _dev(x):
    return J.colmajor(torch.from_numpy(np.ascontiguousarray(x)).cuda())


def _ref(S, real):
    S = np.asarray(S)
    return np.stack([D.support_order_ref(s, real) for s in (S if S.ndim == 3 else S[None])])


# ---- 1. the builder's own order -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,batch", [(SMALL, 4), (dict(Nt=64, Nr=64, L=8, T=2, Mr=8), 3)], ids=["small", "configs1_order"])
def test_support_order_of_zbar_is_the_builders_indx_s(kw, batch):
    from jstsp19_amd.system_model import build_trials
    p = _sp(**kw)
    out = build_trials(p, 1, batch, seed=9)
    Gr, G2 = p.solver_shape[2:]
    got = J.support_order(out["Zbar"])
    assert got.dtype == torch.int32 and got.shape == (batch, Gr * G2) and got.is_cuda
    assert torch.equal(got, out["indx_S"])
    wide = J.support_order_f64(J.colmajor(out["Zbar"].to(torch.complex128)))         # float64 keys of the same values
    np.testing.assert_array_equal(wide.cpu().numpy(), _ref(out["Zbar"].cpu().numpy().astype(complex), np.float64))


# ---- 2. exact against the host reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,cdtype,real", FORMS)
def test_engineered_ties_zeros_nan_and_inf(order, cdtype, real):
    trials = tie_trials().astype(cdtype)                        # (5, 5, 7): three tie trials, all zero, one NaN and one Inf
    want = _ref(trials, real)
    np.testing.assert_array_equal(want[3], np.arange(1, 36))
    for sel in (slice(0, 1), slice(0, 3), slice(None)):         # batch 1, 3 and 5
        np.testing.assert_array_equal(order(_dev(trials[sel])).cpu().numpy(), want[sel])
        np.testing.assert_array_equal(order(trials[sel]), want[sel])                 # numpy in: the host memspace
    one = order(_dev(trials[4]))                                # (Gr, G2) in: one trial
    assert one.shape == (1, 35)
    np.testing.assert_array_equal(one.cpu().numpy(), want[4:5])


@pytest.mark.parametrize("order,cdtype,real", FORMS)
def test_a_64_x_512_trial_without_ties(order, cdtype, real):
    S = continuous_trial().astype(cdtype)
    assert S.shape == (64, 512) and keys_are_separated(S, real)  # no fma contraction of x*x + y*y can reorder these keys
    want = _ref(S, real)
    np.testing.assert_array_equal(order(_dev(S)).cpu().numpy(), want)


# ---- 3. a solver's own S ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solved():
    from jstsp19_amd.system_model import build_trials
    p = _sp(Nt=4, Nr=32, L=4, T=5, Mr=4)
    inp = build_trials(p, 0, 3, seed=4)
    assert p.solver_shape[2:] == (32, 16)
    args = (inp["subY"], inp["Omega"], inp["A"], inp["B"], 5, inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())
    S = J.proposed_algorithm_f64(*args, want_ce=False)[0]                              # dense: the threshold zeroes nothing here
    Sm = J.proposed_algorithm_f64(*args, indx_S=inp["indx_S"], want_ce=False)[0]       # 35 of 512 entries inside the mask
    torch.cuda.synchronize()
    return p, inp, S, Sm


def test_the_order_of_a_float64_estimate(solved):
    p, inp, S, Sm = solved
    np.testing.assert_array_equal(J.support_order_f64(S).cpu().numpy(), _ref(S.cpu().numpy(), np.float64))
    got = J.support_order_f64(Sm).cpu().numpy()
    host = Sm.cpu().numpy()
    np.testing.assert_array_equal(got, _ref(host, np.float64))
    for t in range(3):
        v = host[t].reshape(-1, order="F")
        zeros = np.flatnonzero(v == 0) + 1
        assert 512 - 35 <= zeros.size < v.size                  # masked and soft-thresholded: sparse, not empty
        np.testing.assert_array_equal(got[t, -zeros.size:], zeros)                   # the trailing block: the zeros, ascending
        assert np.all(np.diff(np.abs(v[got[t, :-zeros.size] - 1])) <= 0)
    narrow = Sm.to(torch.complex64)
    np.testing.assert_array_equal(J.support_order(J.colmajor(narrow)).cpu().numpy(), _ref(narrow.cpu().numpy(), np.float32))


def test_an_order_does_not_depend_on_batch_or_memspace(solved):
    p, inp, S, _ = solved
    for order, x in ((J.support_order_f64, S), (J.support_order, J.colmajor(inp["Zbar"]))):
        full = order(x)
        for t in range(3):
            assert torch.equal(order(J.colmajor(x[t:t + 1]))[0], full[t])
        assert torch.equal(order(J.colmajor(x[1:3])), full[1:3])
        host = order(x.cpu().numpy())
        assert isinstance(host, np.ndarray) and host.dtype == np.int32
        np.testing.assert_array_equal(host, full.cpu().numpy())


def test_round_trip_through_proposed_algorithm_angles(solved):
    p, inp, _, _ = solved
    zb = J.colmajor(inp["Zbar"].to(torch.complex128))
    ix = J.support_order_f64(zb)
    args = (inp["subY"], inp["Omega"])
    rest = (inp["A"], inp["B"], 5, inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())
    a = J.proposed_algorithm_angles_f64(*args, ix, *rest, want_ce=False)
    b = J.proposed_algorithm_angles_f64(*args, inp["indx_S"], *rest, want_ce=False)
    c = J.proposed_algorithm_f64(*args, *rest, want_ce=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], c[0])                          # and the mask binds at Imax 5


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,size", [("jstsp_support_order_c32", 8), ("jstsp_support_order_f64", 16)])
def test_refusals_leave_the_output_untouched(entry, size):
    from jstsp19_amd import _lib
    ctx = _lib.default_context(0)
    ctx.use_torch_stream()
    fn = getattr(ctx._lib, entry)
    S = torch.zeros(2 * 12 * size // 8, dtype=torch.float64, device="cuda")
    ix = torch.full((24,), -7, dtype=torch.int32, device="cuda")
    hS, hix = np.zeros(2 * 12 * size // 8), np.full(24, -7, dtype=np.int32)
    for ms, s, o in ((_lib.DEVICE, S.data_ptr(), ix.data_ptr()), (_lib.HOST, hS.ctypes.data, hix.ctypes.data)):
        for dims in ((0, 4, 2), (3, -1, 2), (3, 4, 0), (65536, 32768, 1)):
            assert fn(ctx.handle, *dims, s, o, ms) == E_SHAPE, dims
            assert "support_order" in _lib.load().jstsp_last_error().decode()
        assert fn(ctx.handle, 3, 4, 2, None, o, ms) == E_NULL
        assert fn(ctx.handle, 3, 4, 2, s, None, ms) == E_NULL
        torch.cuda.synchronize()
        assert bool((ix == -7).all()) if ms == _lib.DEVICE else np.all(hix == -7)    # (the other one is filled by its own turn)
        assert fn(ctx.handle, 3, 4, 2, s, o, ms) == 0           # and the context then orders: all zero gives 1..12 per trial
        torch.cuda.synchronize()
    want = np.tile(np.arange(1, 13, dtype=np.int32), 2)
    np.testing.assert_array_equal(ix.cpu().numpy(), want)
    np.testing.assert_array_equal(hix, want)
